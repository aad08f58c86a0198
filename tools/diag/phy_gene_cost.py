"""The gene concordance factors of the species tree in one warm process: so_phy_gene (the fused path of the p distance: the families'
kept columns, their pair counts, distances and presence, a neighbour-joining walk per family over the taxa it holds and the comparison
with the printed tree, all in device memory) against the numpy definitions of swiftortho_amd/phy.py, on a synthetic supermatrix of `taxa`
taxa x `families` families of about `columns` columns each (taxa in groups of 20 that share a group ancestor, 30 % of the sites changed
per level, 5 % gaps; every family lacks a random 0 - 10 % of the taxa: their rows are '-' over its block).
The device call is run twice (the second one without the splits in the result), its three stages split by events (counts = gather + pair
counts + distances and presence, trees, concordance); the numpy definition is timed on the first `host_families` families, stage by
stage -- it is linear in the families, the figure for all of them is scaled from these.
    python tools/diag/phy_gene_cost.py [taxa] [families] [columns] [host_families]
Defaults: 500 taxa x 1000 families x about 300 columns, 20 families on the host."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from swiftortho_amd import phy

args = [int(x) for x in sys.argv[1:]]
T = args[0] if args else 500
F = args[1] if len(args) > 1 else 1000
C = args[2] if len(args) > 2 else 300
H = min(F, args[3] if len(args) > 3 else 20)

rng = np.random.RandomState(11)
AA = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)


def mutate(seq, share):
    out = seq.copy()
    at = rng.random_sample(out.shape) < share
    out[at] = AA[rng.randint(0, 20, size=int(at.sum()))]
    return out


width = rng.randint(C - C // 10, C + C // 10 + 1, size=F)
col_off = np.concatenate([[0], np.cumsum(width)]).astype(np.int64)
K = int(col_off[-1])
root = AA[rng.randint(0, 20, size=K)]
matrix = np.empty((T, K), dtype=np.uint8)
for g0 in range(0, T, 20):
    anc = mutate(root, .3)
    for t in range(g0, min(T, g0 + 20)):
        matrix[t] = mutate(anc, .3)
matrix[rng.random_sample((T, K)) < .05] = phy.GAP
lacking = 0
for f in range(F):
    gone = rng.choice(T, size=rng.randint(0, T // 10 + 1), replace=False)
    matrix[gone, col_off[f]:col_off[f + 1]] = phy.GAP
    lacking += len(gone)
keep = np.arange(K, dtype=np.int64)
print("%d taxa x %d families of %d .. %d columns, %d kept columns (%d MB); a family lacks %.1f taxa on average; W = %d words per split" %
      (T, F, width.min(), width.max(), K, matrix.nbytes >> 20, lacking / float(F), (T + 63) // 64))
fam_off = phy.family_ranges(keep, col_off)
phy.device_gene_counts(matrix[:, :1], keep[:1], np.array([0, 1]))       # warm-up: the library, the device, the code objects

t = time.time(); cmp_, same = phy.pair_counts(matrix, keep); t_pairs = time.time() - t
t = time.time(); ref = phy.tree_splits(phy.distances(cmp_, same, "p")); t_ref = time.time() - t
print("the printed tree: pair_counts (host) %.3f s, tree_splits (host, neighbor_joining's walk) %.3f s" % (t_pairs, t_ref))

first = None
for want in (True, False):
    stats = {}
    t = time.time()
    dec, con, ok, npres, present, splits = phy.device_gene(matrix, keep, fam_off, ref, want_splits=want, stats=stats, timed=True)
    wall = time.time() - t
    if want:
        first = (present[:H].copy(), splits[:H].copy())
    del present, splits
    decided = dec > 0
    gcf = con[decided] / dec[decided].astype(np.float64)
    print("so_phy_gene (%s) wall %.3f s | events: counts %.3f s, trees %.3f s, concordance %.4f s | %d batches, %d waits, tier %d, %d of %d families kept | decisive: min %d median %d max %d | gcf: min %.3f median %.3f max %.3f" %
          ("with every family's splits" if want else "counts only", wall, stats["counts_ms"] / 1e3, stats["trees_ms"] / 1e3, stats["concord_ms"] / 1e3, stats["batches"], stats["waits"], stats["nj_tier"],
           int(ok.sum()), F, dec.min(), int(np.median(dec)), dec.max(), gcf.min() if len(gcf) else 0., float(np.median(gcf)) if len(gcf) else 0., gcf.max() if len(gcf) else 0.))
    sys.stdout.flush()

tt = {"family_counts": 0., "gene_distances": 0., "nj_splits_subset": 0., "concordance": 0.}
S, W = T - 3, (T + 63) // 64
hp, hs, hok = np.zeros((H, W), dtype=np.uint64), np.zeros((H, S, W), dtype=np.uint64), np.zeros(H, dtype=bool)
for f in range(H):
    t = time.time(); c, s = phy.pair_counts(matrix, keep[fam_off[f]:fam_off[f + 1]]); hp[f] = phy.family_present(c); tt["family_counts"] += time.time() - t
    t = time.time(); D, hok[f] = phy.gene_distances(c, s, hp[f], "p"); tt["gene_distances"] += time.time() - t
    t = time.time()
    if hok[f]:
        hs[f] = phy.nj_splits_subset(D, hp[f])
    tt["nj_splits_subset"] += time.time() - t
t = time.time(); hdec, hcon = phy.concordance(ref, hp, hs, hok); tt["concordance"] = time.time() - t
per = sum(tt.values()) / H
print("numpy, %d families: family_counts %.3f s, gene_distances %.3f s, nj_splits_subset %.3f s, concordance %.3f s -> %.3f s per family; linear in the families: %d families about %.0f s (scaled, not run)" %
      (H, tt["family_counts"], tt["gene_distances"], tt["nj_splits_subset"], tt["concordance"], per, F, F * per))
print("the device's present words and splits of the first %d families identical to numpy's: %s" % (H, np.array_equal(first[0], hp) and np.array_equal(first[1], hs)))
if H == F:
    print("the device's decisive and concordant identical to numpy's: %s" % (np.array_equal(dec, hdec) and np.array_equal(con, hcon)))
