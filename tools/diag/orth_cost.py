"""The candidate stage of find_orth on BASELINE config 5's hit records (100k-protein self-search), host and device side by side, in one
process and alternating:  numpy candidates() | device_candidates() from host columns | device_candidates_from_records() on the records
the search left in HBM | relations_from_candidates() (what stays on the host either way); then orthology_from_search() with the device
stage off and on.   python tools/diag/orth_cost.py [proteins] [rounds] [--trace]
The yardstick is the `find_orth` time tools/diag/c5_stages.py prints for the parent commit on the same box in the same call.
--trace: only the search and three device calls, for a profiler run of its own (rocprofv3 --kernel-trace --stats -- python tools/diag/orth_cost.py 100000 3 --trace)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from swiftortho_amd import find_orth as fo, fsearch, pipeline, synthprot

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else 100000
rounds = int(args[1]) if len(args) > 1 else 5
trace = "--trace" in sys.argv
meta = json.load(open(os.path.join(ROOT, "tests", "golden", "pipe_c3.json" if n == 100000 else "pipe_c2.json")))
d = dict(zip(meta["find_hit_flags"][0::2], meta["find_hit_flags"][1::2]))
kw = dict(ssd=d["-s"], nr=d["-r"], ht=int(d["-M"]), chk=int(d["-c"]), step=int(d["-j"]), v=int(d["-v"]), expect=float(d["-e"]), flt=d["-F"])
fa = synthprot.synthprot(n, 300)
ids = fo.fasta_ids(fa)
s = fsearch.Searcher(**kw)
s.load_ref_bytes(fa)
s.load_queries_bytes(fa)
dev = s.search_device()
print("%d proteins, %d hit records resident (%d MB)" % (n, len(dev), len(dev) * 80 >> 20))
if trace:
    for _ in range(rounds):
        fo.device_candidates_from_records(dev, ids, ids)
    s.close()
    sys.exit(0)
rec = np.frombuffer(dev.tensor().cpu().numpy().tobytes(), dtype=np.dtype([(k, t) for k, t in (
    ("qidx", "<i8"), ("sidx", "<i8"), ("identity", "<f8"), ("evalue", "<f8"), ("aln", "<i4"), ("mis", "<i4"), ("gap", "<i4"), ("qst", "<i4"), ("qed", "<i4"),
    ("sst", "<i4"), ("sed", "<i4"), ("bit", "<i4"), ("qlen", "<i4"), ("slen", "<i4"), ("matches", "<i4"), ("ungapped", "<i4"))]))
t = time.time(); cols = fo.columns_from_records(rec, ids, ids); t_cols = time.time() - t
tax, taxa = fo._taxa(cols.names, "|")
stages = [("numpy candidates()", lambda: fo.candidates(cols)),
          ("device_candidates() from host columns", lambda: fo.device_candidates(cols)),
          ("device_candidates_from_records(), records resident", lambda: fo.device_candidates_from_records(dev, ids, ids))]
res = {}
times = {k: [] for k, _ in stages}
for r in range(rounds + 1):   # round 0 warms up (allocator, code objects)
    for k, f in stages:
        t = time.time(); res[k] = f(); dt = time.time() - t
        if r:
            times[k].append(dt)
base = res[stages[0][0]]
print("columns_from_records (host, once): %.3f s;  %d rows kept, %d runs, %d groups, %d names, %d taxa" % (t_cols, base.n_rows, base.n_runs, base.n_groups, len(cols.names), len(taxa)))
for k, _ in stages:
    same = all(np.array_equal(getattr(res[k], a).view(np.int64), getattr(base, a).view(np.int64)) for a in fo.Candidates.FIELDS)
    print("%-52s min %.4f s  median %.4f s  (%d rounds)  tables identical to numpy: %s" % (k, min(times[k]), sorted(times[k])[len(times[k]) // 2], rounds, same))
tt = []
for r in range(rounds):
    t = time.time(); lines = fo.relations_from_candidates(cols.names, tax, taxa, base); tt.append(time.time() - t)
print("%-52s min %.4f s  median %.4f s  (%d relations)" % ("relations_from_candidates() (host)", min(tt), sorted(tt)[len(tt) // 2], len(lines)))
tt = []
for r in range(rounds):
    t = time.time(); fo._record_maps(ids, ids); fo._taxa(cols.names, "|"); tt.append(time.time() - t)
print("%-52s min %.4f s  (name codes and taxa on the host: part of every records call above)" % ("_record_maps() + _taxa()", min(tt)))
# every array touched once per pass that needs it: 80 B per record read; the eight columns (56 B per row) written and read; the kept rows'
# q, s and score (16 B) written and read; the candidate lists -- one 16 B (key, score) entry per (run, subject) group, an in-paralog two, a
# self hit none: counted as one per group -- written by the run kernels, read by the sort, written sorted, read by the marking (the sort's
# own passes in between are not counted); the tables out
parts = (("records", len(dev) * 80), ("columns", len(dev) * 2 * 56), ("kept rows", base.n_rows * 2 * 16), ("candidate lists", base.n_groups * 4 * 16),
         ("tables", (len(base.ot_a) + len(base.ip_a)) * 24 + len(base.co_key) * 16))
traffic = sum(b for _, b in parts)
print("algorithmic traffic of the records call: %.1f MB = %.1f us at 8 TB/s  (%s)" % (traffic / 1e6, traffic / 8e6, ", ".join("%s %.1f" % (k, b / 1e6) for k, b in parts)))
s.close()
p = os.path.join(__import__("tempfile").mkdtemp(), "x.fsa")
open(p, "wb").write(fa)
print("== orthology_from_search(), device_stage off / on, alternating ==")
for r in range(3):
    for stage in (False, True):
        lines2, tm = pipeline.orthology_from_search(p, device_stage=stage, **kw)
        print("device_stage=%s" % stage, {k: round(v, 3) if isinstance(v, float) else v for k, v in tm.items()}, "relations identical:", lines2 == lines)
