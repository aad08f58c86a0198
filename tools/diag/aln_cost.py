"""What asking for the alignments costs on BASELINE config 3 (100k synthetic proteins x 300 aa, seed 11111011111, aa9):
the same steps (index build + search) in three modes -- plain, with a CIGAR per row, with the aligned strings -- interleaved,
best and median per mode.

    python tools/diag/aln_cost.py [--steps K] [--warmup W] [--n N] [--modes plain,cigar,strings]

Prints one JSON line: ms per step for every mode, the ratios to the plain search, rows, the strings' bytes, the CIGARs' runs (total,
mean and maximum per row) and the bytes their download takes.  For the kernel table run it under rocprofv3 --kernel-trace --stats
(k_traceback<false> is the counting walk, k_traceback<true> the emitting one; k_cigar_count / k_cigar_emit code the runs).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from swiftortho_amd import fsearch, synthprot  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--n", type=int, default=100000)
ap.add_argument("--modes", default="plain,cigar,strings")
a = ap.parse_args()
modes = [m for m in a.modes.split(",") if m]
assert modes and set(modes) <= {"plain", "cigar", "strings"}, "--modes: plain, cigar, strings"
fa = synthprot.synthprot(a.n, 300)
s = fsearch.Searcher(ssd="11111011111", nr="AST,CFILMVY,DN,EQ,G,H,KR,P,W", ht=120000000, chk=50000, step=1, v=500, expect=1e-5, flt="T")
s.load_ref_bytes(fa)
s.load_queries_bytes(fa)
ms = {m: [] for m in modes}
info = {}
for it in range(a.warmup + a.steps):
    for m in modes:
        t = time.perf_counter()
        s.drop_index()
        s.build_index()
        h = s.search(alignments=m == "strings", cigar=m == "cigar")
        dt = (time.perf_counter() - t) * 1e3
        if m not in info:   # (outside the timed part of later steps)
            info[m] = {"rows": len(h)}
            if m == "strings":
                info[m]["aln_bytes"] = h.aln_bytes
            if m == "cigar":
                ops, off = h.cigar_buffer()
                per_row = off[1:] - off[:-1]
                info[m].update(runs=int(len(ops)), runs_per_row_mean=round(float(per_row.mean()), 3) if len(per_row) else 0.,
                               runs_per_row_max=int(per_row.max()) if len(per_row) else 0,
                               download_bytes=int(4 * len(ops) + 4 * (len(h) + 1)), bytes_per_row=round(4. * len(ops) / max(len(h), 1), 2))
        h.close()
        if it >= a.warmup:
            ms[m].append(dt)
s.close()
out = {"workload": "config 3, %d proteins" % a.n, "steps": a.steps}
for m in modes:
    out[m] = dict(info[m], ms_median=round(statistics.median(ms[m]), 2), ms_best=round(min(ms[m]), 2))
    if "plain" in modes and m != "plain":
        out[m]["ratio_median"] = round(statistics.median(ms[m]) / statistics.median(ms["plain"]), 3)
print(json.dumps(out))
