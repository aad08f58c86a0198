"""The substitution counts and the LogDet tree in one warm process: so_phy_subst (coding pass + the product N = E E^T on the matrix cores)
against the numpy definitions of swiftortho_amd/phy.py, on
(a) a synthetic supermatrix of `taxa` taxa x `columns` kept columns (taxa in groups of 20 that share a group ancestor, 30 % of the sites
    changed per level, 5 % gaps -- the matrix of tools/diag/phy_boot_cost.py): the tensor with and without the copy back, the two passes
    split by events, subst_counts in numpy, the host's determinants (distances(model='logdet')), one bootstrap replicate each way, and the
    whole bootstrap of B replicates under logdet on the device path;
(b) BASELINE config 5's families (the 100k-protein self-search with a CIGAR on every row, as tools/diag/phy_cost.py builds them): the
    tensor and the LogDet tree of that supermatrix.
The product's rate is given against the int8 matrix-core rate (twice the dense bf16 rate: 2 x 2.5e15 operations a second), over the
multiply-adds of the tiles the kernel walks.
    python tools/diag/phy_subst_cost.py [taxa] [columns] [rounds] [B, 0 = no bootstrap] [proteins of (b), 0 = skip] [boot: of (a) the bootstrap only]
Defaults: 500 taxa x 300000 columns, 5 rounds, B = 100, 100000 proteins."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from swiftortho_amd import phy

boot_only = sys.argv[-1] == "boot"
args = [int(x) for x in sys.argv[1:len(sys.argv) - boot_only]]
T = args[0] if args else 500
K = args[1] if len(args) > 1 else 300000
rounds = args[2] if len(args) > 2 else 5
B = args[3] if len(args) > 3 else 100
n_prot = args[4] if len(args) > 4 else 100000
SEED = 1
I8_PEAK = 2 * 2.5e15          # operations a second (a multiply-add is two)


def timed(f, n):
    out, tt = None, []
    for r in range(n + (1 if n > 1 else 0)):     # with several rounds the first warms up (allocator, code objects)
        t = time.time(); out = f(); dt = time.time() - t
        if r or n == 1:
            tt.append(dt)
    tt.sort()
    return out, tt


def line(name, tt, note=""):
    print("%-62s min %.4f s  median %.4f s  (%d rounds)  %s" % (name, tt[0], tt[len(tt) // 2], len(tt), note))
    sys.stdout.flush()


def tune(name):
    import re
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, open(os.path.join(ROOT, "swiftortho_amd", "csrc", "tune.h")).read()).group(1))


def device_tensor(matrix, keep, name):
    """the device call with and without the copy back, the passes by events -> the tensor"""
    T = len(matrix)
    N, tt = timed(lambda: phy.device_subst_counts(matrix, keep), rounds)
    line("so_phy_subst, tensor copied back (%s)" % name, tt, "%d MB" % (N.nbytes >> 20))
    ev = []

    def bare():
        st = {}
        phy._device_subst("phy_subst_cost", matrix, keep, 0, 0, 0, 0, st, want=False, timed=True)
        ev.append((st["product_ms"], st["code_ms"]))
    _, tt = timed(bare, rounds)
    prod, code = min(ev[1:] or ev)
    tile = tune("PHS_TILE")
    nt = (20 * T + tile - 1) // tile
    macs = nt * (nt + 1) // 2 * tile * tile * ((len(keep) + 31) & ~31)
    line("so_phy_subst, no copy back (%s)" % name, tt, "events: coding pass %.2f ms, product %.2f ms = %.1f T multiply-adds/s over the %.2e of the walked tiles, %.1f %% of the int8 rate"
         % (code, prod, macs / prod / 1e9, macs, 100. * 2 * macs / (prod / 1e3) / I8_PEAK))
    return N


# ---- (a) synthetic ----
rng = np.random.RandomState(7)
AA = np.frombuffer(phy.AA20, dtype=np.uint8)


def mutate(seq, share):
    out = seq.copy()
    at = rng.random_sample(out.shape) < share
    out[at] = AA[rng.randint(0, 20, size=int(at.sum()))]
    return out


root = AA[rng.randint(0, 20, size=K)]
matrix = np.empty((T, K), dtype=np.uint8)
for g0 in range(0, T, 20):
    anc = mutate(root, .3)
    for t in range(g0, min(T, g0 + 20)):
        matrix[t] = mutate(anc, .3)
matrix[rng.random_sample((T, K)) < .05] = phy.GAP
keep = np.arange(K, dtype=np.int64)
P = T * (T - 1) // 2
print("(a) %d taxa x %d kept columns (%d MB), %d pairs; N = E E^T is %.1e multiply-adds in full" % (T, K, matrix.nbytes >> 20, P, (20. * T) ** 2 * K))
phy.device_subst_counts(matrix[:2, :1], keep[:1])       # warm-up: the library, the device, the code objects
N = phy.device_subst_counts(matrix, keep) if boot_only else device_tensor(matrix, keep, "synthetic")
if not boot_only:
    want, tt = timed(lambda: phy.subst_counts(matrix, keep), 1)
    line("numpy: subst_counts (float32 one-hot products)", tt, "device identical to numpy: %s" % np.array_equal(N, want))
    del want


class Sm:
    pass


sm = Sm()
sm.matrix, sm.keep, sm.taxa, sm.subst, sm.stats = matrix, keep, [b"t%d" % t for t in range(T)], N, {}
tk = phy.Tasks(T, [0, K], np.zeros(T, dtype=np.int32), np.arange(T), np.ones(T, dtype=np.uint8), np.arange(T, dtype=np.int64) * K, np.full(T, K), np.ones(T), np.ones(T),
               np.zeros(T + 1, dtype=np.int64), np.zeros(0, dtype=np.uint32), matrix.reshape(-1))
sm.cmp, sm.same = phy.device_build(tk, 1., want_matrix=False)[3:]
if not boot_only:
    D, tt = timed(lambda: phy.distances(sm.cmp, sm.same, "logdet", sm.taxa, N), min(rounds, 2))
    line("host: the %d determinants (distances, model logdet)" % P, tt, "%.1f us a pair" % (tt[0] / P * 1e6))
    t = time.time(); c, s = phy.device_boot_counts(matrix, keep, SEED, 0, 1); t_c = time.time() - t
    t = time.time(); sub = phy.device_boot_subst(matrix, keep, SEED, 0, 1); t_s = time.time() - t
    t = time.time(); Db, good = phy.boot_distances(c[0], s[0], "logdet", sub[0]); t_d = time.time() - t
    t = time.time(); sp = phy.device_nj_splits(Db[None]) if good else None; t_n = time.time() - t
    print("one replicate, device path: so_phy_boot_counts %.3f s, so_phy_subst %.3f s, determinants (host) %.3f s, so_phy_nj_splits %.3f s -> %.2f s; kept: %s" %
          (t_c, t_s, t_d, t_n, t_c + t_s + t_d + t_n, good))
    t = time.time(); c2, s2 = phy.boot_counts(matrix, keep, SEED, 0); h_c = time.time() - t
    t = time.time(); sub2 = phy.boot_subst(matrix, keep, SEED, 0); h_s = time.time() - t
    t = time.time(); Dh, good2 = phy.boot_distances(c2, s2, "logdet", sub2); h_d = time.time() - t
    t = time.time(); sph = phy.nj_splits(Dh) if good2 else None; h_n = time.time() - t
    print("one replicate, numpy: boot_counts %.3f s, boot_subst %.3f s, determinants %.3f s, nj_splits %.3f s -> %.2f s; identical to the device path: %s" %
          (h_c, h_s, h_d, h_n, h_c + h_s + h_d + h_n, np.array_equal(sub[0], sub2) and Db.tobytes() == Dh.tobytes() and (sp is None or np.array_equal(sp[0], sph))))
    sys.stdout.flush()
    del sub, sub2
if B > 0:
    st = {}
    t = time.time(); count, valid, ok, _ = phy.bootstrap_replicates(sm, B, SEED, "logdet", device_stage=True, stats=st, want_splits=False); t_b = time.time() - t
    print("bootstrap under logdet, device path, B = %d: %.1f s (%d device calls, %d replicates kept) = %.2f s a replicate; linear in B: 1000 replicates about %.0f s" %
          (B, t_b, st.get("calls", 0), valid, t_b / B, 1000. * t_b / B))
    sys.stdout.flush()
del matrix, N, sm, tk

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
    hits = sr.search(cigar=True)
    rec = hits.array()
    ops, off = hits.cigar_buffer()
    cols = fo.columns_from_records(rec, ids, ids)
    table = rbh.device_core_table(cols, fa)
    rows = phy.RecordRows(cols, rec["qst"], rec["sst"], ops, off)
    share = .9 if phy.families(table) else 0.
    tk, _ = phy.tasks_from_families(cols.names, table, rbh.fasta_records(fa), rows, True, min_share=share)
    hits.close()
    sr.close()
    m5, gaps, keep5, cmp5, same5 = phy.device_build(tk, 1.)
    print("(b) %d proteins: %d families%s, %d taxa x %d kept columns" % (n_prot, len(tk.col_off) - 1, "" if share else " (of ALL core genes: none reaches 0.9 of the taxa)", len(m5), len(keep5)))
    N5 = device_tensor(m5, keep5, "config 5")
    want, tt = timed(lambda: phy.subst_counts(m5, keep5), 1)
    line("numpy: subst_counts", tt, "device identical to numpy: %s" % np.array_equal(N5, want))
    try:
        D5, tt = timed(lambda: phy.distances(cmp5, same5, "logdet", table.slots, N5), min(rounds, 2))
        line("host: the %d determinants" % len(N5), tt)
        nwk, tt = timed(lambda: phy.neighbor_joining(D5, table.slots), 1)
        line("neighbor_joining (host)", tt, "%d bytes of Newick" % len(nwk))
    except phy.DistanceRefused as e:
        print("logdet refuses this supermatrix: %s" % e)
