"""The reciprocal-best-hit stage on BASELINE config 5's hit records (100k-protein self-search) in one warm process, alternating:
the device call on the records the search left in HBM (rbh.device_core_table_from_records: pairs and core table in ONE so_rbh_records
call) | the numpy definitions on the same records downloaded (reciprocal_best_hits + core_table) | the device call from host columns;
minimum and median of 9 rounds after a warm-up round, the share of runs and rows each tier of the winner stage took, and -- when
--reference DIR names a checkout of the reference -- its scripts/get_rbh.py on the .sc text of the same records.
    python tools/diag/rbh_cost.py [proteins] [rounds] [--reference DIR]"""
import json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from swiftortho_amd import _lib, find_orth as fo, fsearch, rbh, synthprot

argv = sys.argv[1:]
ref_dir = argv[argv.index("--reference") + 1] if "--reference" in argv else None
args = [a for k, a in enumerate(argv) if not a.startswith("--") and (k == 0 or argv[k - 1] != "--reference")]
n = int(args[0]) if args else 100000
rounds = int(args[1]) if len(args) > 1 else 9
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
rec = np.frombuffer(dev.tensor().cpu().numpy().tobytes(), dtype=np.dtype(_lib.SoHit))
t = time.time(); cols = fo.columns_from_records(rec, ids, ids); t_cols = time.time() - t


def numpy_stage():
    tab = rbh.core_table(cols, fa)
    tab.pairs = rbh.reciprocal_best_hits(cols)
    return tab


stages = [("device, records resident (so_rbh_records)", lambda: rbh.device_core_table_from_records(dev, ids, ids, fa)[1]),
          ("numpy definitions on the downloaded records", numpy_stage),
          ("device, from host columns (so_rbh_cols)", lambda: rbh.device_core_table(cols, fa))]
res, times = {}, {k: [] for k, _ in stages}
for r in range(rounds + 1):   # round 0 warms up (allocator, code objects)
    for k, f in stages:
        t = time.time(); res[k] = f(); dt = time.time() - t
        if r:
            times[k].append(dt)
base = res[stages[1][0]]
st = res[stages[0][0]].stats
print("columns_from_records (host, once): %.3f s;  %d rows, %d runs (%.1f rows per run), %d winners, %d names, %d taxa" %
      (t_cols, len(rec), st["n_runs"], len(rec) / max(st["n_runs"], 1), st["n_winners"], len(cols.names), len(base.slots)))
print("tiers: one wave per run %d runs (%.2f %%) / %d rows (%.2f %%); sorted tier %d runs / %d rows; host waits of the call: %d" %
      (st["n_runs"] - st["n_runs_long"], 100. * (st["n_runs"] - st["n_runs_long"]) / max(st["n_runs"], 1), len(rec) - st["n_rows_long"],
       100. * (len(rec) - st["n_rows_long"]) / max(len(rec), 1), st["n_runs_long"], st["n_rows_long"], st["waits"]))
print("%d pairs, %d core genes of %s, %d kept groups" % (len(base.pairs[0]), len(base.genes), base.reference.decode(), len(rbh.core_groups(cols.names, base))))
for k, _ in stages:
    g = res[k]
    same = (g.pairs[0].tolist() == base.pairs[0].tolist() and g.pairs[1].tolist() == base.pairs[1].tolist() and g.genes.tolist() == base.genes.tolist()
            and np.array_equal(g.fwd, base.fwd) and np.array_equal(g.rec, base.rec))
    print("%-48s min %.4f s  median %.4f s  (%d rounds)  identical to numpy: %s" % (k, min(times[k]), sorted(times[k])[len(times[k]) // 2], rounds, same))
tt = []
for r in range(rounds):
    t = time.time(); fo._record_maps(ids, ids); rbh._slot_codes(cols.names, fa, "", "|"); tt.append(time.time() - t)
print("%-48s min %.4f s  (name codes and taxon slots on the host: part of every device call above)" % ("_record_maps() + _slot_codes()", min(tt)))
if ref_dir and os.path.isfile(os.path.join(ref_dir, "scripts", "get_rbh.py")):
    with tempfile.TemporaryDirectory() as tmp:
        sc = os.path.join(tmp, "x.sc")
        arr, m = fsearch.hits_from_bytes(s, rec.view(np.uint8).copy())
        s._chk(s.L.so_write_sc(s.h, arr, m, os.fsencode(sc), b"w"))
        tt = []
        for r in range(3):
            t = time.time(); out = subprocess.run([sys.executable, os.path.join(ref_dir, "scripts", "get_rbh.py"), sc], stdout=subprocess.PIPE).stdout; tt.append(time.time() - t)
        print("%-48s min %.4f s  (3 rounds, process start included)  pairs identical: %s" %
              ("reference scripts/get_rbh.py on the .sc text", min(tt), out == rbh.rbh_lines(cols.names, *base.pairs)))
else:
    print("reference scripts/get_rbh.py on the .sc text: not timed (no --reference checkout on this machine)")
s.close()
