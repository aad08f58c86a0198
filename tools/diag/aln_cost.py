"""What asking for the alignments costs on BASELINE config 3 (100k synthetic proteins x 300 aa, seed 11111011111, aa9):
the same steps (index build + search) with alignments off and on, interleaved, best and median per mode.

    python tools/diag/aln_cost.py [--steps K] [--warmup W] [--n N]

Prints one JSON line: ms per step for both modes, their ratio, rows and alignment bytes.  For the kernel table run it under
rocprofv3 --kernel-trace --stats (k_traceback<false> is the counting walk, k_traceback<true> the emitting one).
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
a = ap.parse_args()
fa = synthprot.synthprot(a.n, 300)
s = fsearch.Searcher(ssd="11111011111", nr="AST,CFILMVY,DN,EQ,G,H,KR,P,W", ht=120000000, chk=50000, step=1, v=500, expect=1e-5, flt="T")
s.load_ref_bytes(fa)
s.load_queries_bytes(fa)
ms = {False: [], True: []}
rows = {}
for it in range(a.warmup + a.steps):
    for on in (False, True):
        t = time.perf_counter()
        s.drop_index()
        s.build_index()
        h = s.search(alignments=on)
        dt = (time.perf_counter() - t) * 1e3
        rows[on] = (len(h), h.aln_bytes)
        h.close()
        if it >= a.warmup:
            ms[on].append(dt)
s.close()
off, on = statistics.median(ms[False]), statistics.median(ms[True])
print(json.dumps({"workload": "config 3, %d proteins" % a.n, "steps": a.steps, "off_ms_median": round(off, 2), "on_ms_median": round(on, 2),
                  "off_ms_best": round(min(ms[False]), 2), "on_ms_best": round(min(ms[True]), 2), "ratio_median": round(on / off, 3),
                  "rows": rows[True][0], "rows_off": rows[False][0], "aln_bytes": rows[True][1]}))
