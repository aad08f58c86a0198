"""The bootstrap of the species tree in one warm process: so_phy_boot (the fused path of the p distance: drawn columns, pair counts,
distances, a neighbour-joining walk per replicate and the comparison with the printed tree, all in device memory) against the numpy
definitions of swiftortho_amd/phy.py, on a synthetic supermatrix of `taxa` taxa x `columns` kept columns (taxa in groups of 20 that share
a group ancestor, 30 % of the sites changed per level, 5 % gaps).
The device call is run for every B given, its three stages split by events (counts = gather + pair counts + distances, trees, support);
the numpy definition is timed on two replicates, stage by stage -- it is linear in B, a replicate costs what these two cost.
    python tools/diag/phy_boot_cost.py [taxa] [columns] [B ...]
Defaults: 500 taxa x 300000 columns, B = 100 and 1000."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from swiftortho_amd import phy

args = [int(x) for x in sys.argv[1:]]
T = args[0] if args else 500
K = args[1] if len(args) > 1 else 300000
Bs = args[2:] or [100, 1000]
SEED = 1

rng = np.random.RandomState(7)
AA = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)


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
print("%d taxa x %d kept columns (%d MB), seed %d; W = %d words per split" % (T, K, matrix.nbytes >> 20, SEED, (T + 63) // 64))
phy.device_boot_counts(matrix[:, :1], keep[:1], 0, 0, 1)       # warm-up: the library, the device, the code objects


def whole_counts():
    """the pair counts of the whole matrix, for the printed tree: so_phy_build over one family whose every row is given as it is"""
    n = T
    tk = phy.Tasks(T, [0, K], np.zeros(n, dtype=np.int32), np.arange(n), np.ones(n, dtype=np.uint8), np.arange(n, dtype=np.int64) * K, np.full(n, K), np.ones(n), np.ones(n),
                   np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.uint32), matrix.reshape(-1))
    return phy.device_build(tk, 1., want_matrix=False)


D0 = phy.distances(*whole_counts()[3:], "p")
t = time.time(); ref = phy.tree_splits(D0); t_ref = time.time() - t
print("the printed tree: tree_splits (host, neighbor_joining's walk) %.3f s" % t_ref)

first = None
for B in Bs:
    stats = {}
    t = time.time()
    count, valid, ok, splits = phy.device_boot(matrix, keep, SEED, B, ref, want_splits=first is None, stats=stats, timed=True)
    wall = time.time() - t
    if first is None:
        first = splits[:2].copy()
    del splits
    print("so_phy_boot B = %-5d wall %.3f s | events: counts %.3f s, trees %.3f s, support %.4f s | %d batches, %d waits, %d valid | support: min %.3f median %.3f max %.3f" %
          (B, wall, stats["counts_ms"] / 1e3, stats["trees_ms"] / 1e3, stats["support_ms"] / 1e3, stats["batches"], stats["waits"], valid,
           count.min() / valid, float(np.median(count)) / valid, count.max() / valid))
    sys.stdout.flush()

same_splits = True
tt = {"boot_counts": [], "boot_distances": [], "nj_splits": []}
for b in range(2):
    t = time.time(); c, s = phy.boot_counts(matrix, keep, SEED, b); tt["boot_counts"].append(time.time() - t)
    t = time.time(); D, good = phy.boot_distances(c, s, "p"); tt["boot_distances"].append(time.time() - t)
    t = time.time(); sp = phy.nj_splits(D); tt["nj_splits"].append(time.time() - t)
    same_splits = same_splits and good and np.array_equal(sp, first[b])
per = sum(min(v) for v in tt.values())
print("numpy, two replicates: boot_counts %.3f / %.3f s, boot_distances %.4f / %.4f s, nj_splits %.3f / %.3f s -> %.2f s per replicate; linear in B: B = 100 about %.0f s, B = 1000 about %.0f s" %
      (tt["boot_counts"][0], tt["boot_counts"][1], tt["boot_distances"][0], tt["boot_distances"][1], tt["nj_splits"][0], tt["nj_splits"][1], per, 100 * per, 1000 * per))
print("the device's splits of replicates 0 and 1 identical to numpy's: %s" % same_splits)
