"""The pan-genome stage on a synthetic set of families in one warm process, alternating: the device call (pan.device_pan_genome: count
matrix, types and rarefaction in ONE so_pan_genome call) | the same call without the count matrix | the numpy definitions
(pan.count_matrix + row_types + rarefaction: the reference's arithmetic, its array passes per genome added); minimum and median of the
rounds after a warm-up round, the host coding of ids and taxa (pan.member_table_of, Python) beside them, the tier and the host waits.
    python tools/diag/pan_cost.py [rows] [taxa] [rounds] [numpy rounds] [--no-device]
Generator (numpy RandomState(7)): every family draws a class -- 70 % one member, 15 % each taxon with p = 0.02, 8 % with 0.2, 4 % with
0.6, 3 % with 0.99 -- and takes each taxon with its class's probability, and one more taxon drawn uniformly (so no family is empty);
a present taxon has one member.  Defaults: 200000 rows x 500 taxa, 9 rounds."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from swiftortho_amd import pan

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n_rows = int(args[0]) if args else 200000
n_taxa = int(args[1]) if len(args) > 1 else 500
rounds = int(args[2]) if len(args) > 2 else 9
np_rounds = int(args[3]) if len(args) > 3 else rounds
use_device = "--no-device" not in sys.argv

rng = np.random.RandomState(7)
cls = rng.choice(5, size=n_rows, p=[.70, .15, .08, .04, .03])
prob = np.array([0., .02, .2, .6, .99])[cls]
row, tax = [], []
for lo in range(0, n_rows, 20000):      # (in slabs: the rows x taxa draw is not held whole)
    hi = min(n_rows, lo + 20000)
    x = rng.rand(hi - lo, n_taxa) < prob[lo:hi, None]
    x[np.arange(hi - lo), rng.randint(n_taxa, size=hi - lo)] = True      # no family is empty
    r, t = np.nonzero(x)
    row.append(r + lo), tax.append(t)
row, tax = np.concatenate(row).astype(np.int32), np.concatenate(tax).astype(np.int32)
print("%d rows x %d taxa, %d members (%.1f per row); classes: %s" % (n_rows, n_taxa, len(row), len(row) / n_rows, np.bincount(cls, minlength=5).tolist()))

# host coding: the same table from ids, as the script and the pipeline get it (groups as lists of ids, every gene a FASTA record)
taxa = ["tx%03d" % t for t in range(n_taxa)]
ids = ["tx%03d|g%d" % (t, k) for k, t in enumerate(tax.tolist())]
starts = np.flatnonzero(np.concatenate([[True], row[1:] != row[:-1]])).tolist() + [len(row)]
groups = [ids[a:b] for a, b in zip(starts[:-1], starts[1:])]
t_host = []
for _ in range(3):
    t = time.time(); table = pan.member_table_of(groups, ids, taxa); t_host.append(time.time() - t)
assert table.n_rows == n_rows == table.n_file_rows and np.array_equal(table.row, row) and np.array_equal(table.taxon, tax)
del ids, groups
print("host coding (member_table_of: ids -> (row, taxon) pairs, Python)   min %.3f s  median %.3f s  (3 runs)" % (min(t_host), sorted(t_host)[1]))

ts, tc = .05, .95
spec_max, core_min = pan.type_thresholds(ts, tc, n_taxa)
t = time.time(); S, C = pan.step_thresholds(ts, tc, n_taxa); perm = pan.permutations(n_taxa); t_thr = time.time() - t
print("thresholds and the 20 orders (host, once): %.4f s" % t_thr)


def numpy_stage():
    counts = pan.count_matrix(row, tax, n_rows, n_taxa)
    types, totals = pan.row_types(counts, n_rows, spec_max, core_min)
    return pan.PanResult(counts, types, totals, *pan.rarefaction(counts, perm, S, C))


stages = [("numpy definitions", numpy_stage, np_rounds)]
if use_device:
    dev = lambda want: pan.device_pan_genome(row, tax, n_rows, n_rows, n_taxa, spec_max, core_min, perm, S, C, want_counts=want)
    stages = [("device call, with the count matrix", lambda: dev(True), rounds), ("device call, without the count matrix", lambda: dev(False), rounds)] + stages
res, times = {}, {k: [] for k, _, _ in stages}
for r in range(rounds + 1):     # round 0 warms up (allocator, code objects)
    for k, f, n in stages:
        if r > n:
            continue
        t = time.time(); res[k] = f(); dt = time.time() - t
        if r:
            times[k].append(dt)
    sys.stderr.write("round %d done\n" % r), sys.stderr.flush()
base = res["numpy definitions"]
for k, _, n in stages:
    g = res[k]
    same = (np.array_equal(g.types, base.types) and g.totals == base.totals and np.array_equal(g.core, base.core) and np.array_equal(g.spec, base.spec)
            and np.array_equal(g.panz, base.panz) and (g.counts is None or np.array_equal(g.counts, base.counts)))
    v = sorted(times[k])
    print("%-40s min %.4f s  median %.4f s  max %.4f s  (%d rounds)  identical to numpy: %s  %s" % (k, v[0], v[len(v) // 2], v[-1], len(v), same, g.stats or ""))
print("totals (core, share, specific): %s;  last curve point (j = %d, order 0): core %d new %d pan %d" %
      (base.totals, n_taxa, base.core[0, -1], base.spec[0, -1], base.panz[0, -1]))
