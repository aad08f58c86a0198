"""The supermatrix stage in one warm process, the device calls against the numpy definitions (swiftortho_amd/phy.py), on
(a) a synthetic case: `taxa` taxa x `families` families of 300 columns, every (family, taxon) block present with p = 0.9, a member's CIGAR
    three runs (M, one I or D of 1 .. 3, M) -- so_phy_build (matrix, gaps, kept columns, pair counts in ONE call) with and without the
    matrix copied back | fill_matrix + column_gaps + kept_columns + pair_counts; and so_phy_rows against pick_rows on as many wanted pairs
    as there are members, over four times as many hit rows;
(b) BASELINE config 5's hits (the 100k-protein self-search, here with a CIGAR on every row): the core table, then phy.supermatrix() with
    device_stage off and on -- host assembly of the tasks (Python) beside the two ways to build from them -- and the tree.  Where no family
    reaches the reference's 0.9 of the taxa, the families of all core genes are measured instead, and the output says so.
    python tools/diag/phy_cost.py [taxa] [families] [rounds] [proteins of (b), 0 = skip]
Defaults: 500 taxa x 1000 families (300000 columns, about 4e10 residue comparisons), 5 rounds (numpy: 1), 100000 proteins."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from swiftortho_amd import phy

args = sys.argv[1:]
T = int(args[0]) if args else 500
F = int(args[1]) if len(args) > 1 else 1000
rounds = int(args[2]) if len(args) > 2 else 5
n_prot = int(args[3]) if len(args) > 3 else 100000
ALEN = 300


def timed(f, n):
    out, tt = None, []
    for r in range(n + (1 if n > 1 else 0)):     # with several rounds the first warms up (allocator, code objects)
        t = time.time(); out = f(); dt = time.time() - t
        if r or n == 1:
            tt.append(dt)
    tt.sort()
    return out, tt


def line(name, tt, note=""):
    print("%-58s min %.4f s  median %.4f s  (%d rounds)  %s" % (name, tt[0], tt[len(tt) // 2], len(tt), note))
    sys.stdout.flush()


# ---- (a) synthetic ----
rng = np.random.RandomState(7)
present = rng.rand(F, T) < .9
fam, slot = np.nonzero(present)
n = len(fam)
a = rng.randint(50, 200, size=n)
g = rng.randint(1, 4, size=n)
op = rng.randint(1, 3, size=n)
c = ALEN - a - g - 10
runs = np.stack([a << 4, (g << 4) | op, c << 4], 1).astype(np.uint32).ravel()
res = phy.GAP + 20 + rng.randint(0, 20, size=n * ALEN).astype(np.uint8)        # 20 letters ('A' ..)
tk = phy.Tasks(T, np.arange(F + 1) * ALEN, fam, slot, np.zeros(n, dtype=np.uint8), np.arange(n, dtype=np.int64) * ALEN, np.full(n, ALEN), np.ones(n), np.ones(n),
               np.arange(n + 1) * 3, runs, res)
print("(a) %d taxa x %d families = %d columns, %d tasks, %d runs, %d MB of residues; about %.1e residue comparisons" %
      (T, F, F * ALEN, n, len(runs), len(res) >> 20, T * T * F * ALEN))
share = .2
stats = {}
dev, tt = timed(lambda: phy.device_build(tk, share, stats=stats), rounds)
line("so_phy_build, matrix copied back", tt, str(stats))
dev2, tt = timed(lambda: phy.device_build(tk, share, want_matrix=False), rounds)
line("so_phy_build, counts only", tt)
matrix, tt = timed(lambda: phy.fill_matrix(tk), 1)
line("numpy: fill_matrix (project() per task, Python)", tt)
(gaps, keep), tt = timed(lambda: (lambda gp: (gp, phy.kept_columns(gp, share, T)))(phy.column_gaps(matrix)), 1)
line("numpy: column_gaps + kept_columns", tt, "%d of %d columns kept at a gap share of %.2f" % (len(keep), len(gaps), share))
(cmp_, same), tt = timed(lambda: phy.pair_counts(matrix, keep), 1)
line("numpy: pair_counts (float32 products per byte value)", tt)
ok = (np.array_equal(dev[0], matrix) and np.array_equal(dev[1], gaps) and np.array_equal(dev[2], keep) and np.array_equal(dev[3], cmp_) and np.array_equal(dev[4], same)
      and np.array_equal(dev2[3], cmp_) and np.array_equal(dev2[4], same))
print("device identical to numpy: %s" % ok)
nrow = 4 * n
q, s = rng.randint(0, 1 << 20, size=nrow), rng.randint(0, 1 << 20, size=nrow)
sco = rng.randint(0, 400, size=nrow).astype(np.float64)
pick = rng.choice(nrow, size=n, replace=False)
pq, ps = q[pick], s[pick]
want, tt = timed(lambda: phy.pick_rows(q, s, sco, pq, ps), min(rounds, 3))
line("numpy: pick_rows, %d rows, %d wanted pairs" % (nrow, n), tt)
got, tt = timed(lambda: phy.device_pick_rows(q, s, sco, pq, ps), rounds)
line("so_phy_rows", tt, "identical to numpy: %s" % np.array_equal(got, want))
del matrix, dev, dev2, res, tk

# ---- (b) config 5 ----
if n_prot:
    from swiftortho_amd import find_orth as fo, fsearch, rbh, synthprot
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "pipe_c3.json" if n_prot == 100000 else "pipe_c2.json")))
    d = dict(zip(meta["find_hit_flags"][0::2], meta["find_hit_flags"][1::2]))
    kw = dict(ssd=d["-s"], nr=d["-r"], ht=int(d["-M"]), chk=int(d["-c"]), step=int(d["-j"]), v=int(d["-v"]), expect=float(d["-e"]), flt=d["-F"])
    fa = synthprot.synthprot(n_prot, 300)
    ids = fo.fasta_ids(fa)
    sr = fsearch.Searcher(**kw)
    sr.load_ref_bytes(fa)
    sr.load_queries_bytes(fa)
    t = time.time(); hits = sr.search(cigar=True); t_search = time.time() - t
    rec = hits.array()
    ops, off = hits.cigar_buffer()
    print("(b) %d proteins: %d hit rows, %d CIGAR runs; search with CIGARs %.2f s" % (n_prot, len(rec), len(ops), t_search))
    t = time.time(); cols = fo.columns_from_records(rec, ids, ids); t_cols = time.time() - t
    t = time.time(); table = rbh.device_core_table(cols, fa); t_tab = time.time() - t
    records = rbh.fasta_records(fa)
    rows = phy.RecordRows(cols, rec["qst"], rec["sst"], ops, off)
    print("columns_from_records %.2f s, core table (so_rbh_cols) %.2f s: %d core genes, %d kept families of %d taxa" %
          (t_cols, t_tab, len(table.genes), len(phy.families(table)), len(table.slots)))
    share = .9 if phy.families(table) else 0.
    if not share:
        print("no family reaches the reference's 0.9 of the taxa (every taxon holds a family with p = 0.8 in this set): measured on the families of ALL core genes instead")
    for name, stage in (("device", True), ("numpy", False)):
        (tk, anchors), tt = timed(lambda: phy.tasks_from_families(cols.names, table, records, rows, stage, min_share=share), 3)
        line("tasks_from_families, rows picked by %s" % name, tt, "%d tasks" % len(tk.fam))
    built, tt = timed(lambda: phy.build(tk, 1.), 3)
    line("numpy: build() from the tasks", tt, "%d columns" % len(built[1]))
    devb, tt = timed(lambda: phy.device_build(tk, 1.), rounds)
    line("so_phy_build from the tasks", tt, "identical to numpy: %s" % all(np.array_equal(x, y) for x, y in zip(devb, built)))
    nwk, tt = timed(lambda: phy.neighbor_joining(phy.distances(devb[3], devb[4], "p", table.slots), table.slots), 3)
    line("distances + neighbor_joining (host)", tt, "%d taxa, %d bytes of Newick" % (len(table.slots), len(nwk)))
    hits.close()
    sr.close()
