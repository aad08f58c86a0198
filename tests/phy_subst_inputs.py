"""Designed matrices for the substitution counts (swiftortho_amd/phy.py subst_counts, boot_subst; csrc/phy.hip k_phy_code, k_phy_subst) and
for the Kimura and LogDet distances made from them; literal restatements of the definitions.  Shared by tests/test_phy_subst.py (CPU) and
tests/test_gpu_phy_subst.py (device)."""
import functools
import os
import re

import numpy as np

AA20 = b"ARNDCQEGHILKMFPSTWYV"
AA = np.frombuffer(AA20, dtype=np.uint8)
GAP = 45
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tune(name):
    """a #define of csrc/tune.h as an int"""
    text = open(os.path.join(ROOT, "swiftortho_amd", "csrc", "tune.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)u?\b" % name, text).group(1))


CHUNK_COLS = tune("PHS_CHUNK_COLS")      # columns of one LDS chunk of k_phy_subst; a single tile's columns are cut into two ranges beyond it
TILE_ROWS = tune("PHS_TILE")             # rows of E per workgroup: 6.4 taxa
K_STEP = 32                              # columns of one v_mfma_i32_32x32x32_i8

# 20 T: 2, 3 below two MFMA tiles, 4 inside one wave's 64 rows, 7 just across TILE_ROWS = 128 (a second workgroup tile and a second set of
# staged taxa, of 12 rows), 8 on a 32-row boundary, 9, 13 across 256, and several workgroup tiles with a ragged last one (33, 65)
TAXA = (2, 3, 4, 7, 8, 9, 13, 33, 65)
COLS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, CHUNK_COLS + 1)


def asym(T, K):
    """taxon t holds AA20[(k * (t + 1) + t) % 20] at column k: every pair's table is far from symmetric -- the input that tells a swapped
    row / column map of the product, or of its store, from the right one"""
    k, t = np.arange(K, dtype=np.int64)[None, :], np.arange(T, dtype=np.int64)[:, None]
    return AA[(k * (t + 1) + t) % 20]


def mixed(T, K, seed=0):
    """random bytes over the 20 letters plus '-', X, B, Z, U, '*', lower-case letters, 0x00 and 0xFF; row 1 is all '-', row 2 (T > 2) all X"""
    rng = np.random.RandomState(1000 + seed)
    other = np.frombuffer(b"-XBZU*arndv\x00\xff", dtype=np.uint8)
    m = AA[rng.randint(0, 20, size=(T, K))]
    few = rng.randint(0, 4, size=(T, K))                    # a share of the columns over four letters only: equal residues do occur
    m = np.where(rng.random_sample((T, K)) < .5, AA[few], m)
    at = rng.random_sample((T, K)) < .25
    m[at] = other[rng.randint(0, len(other), size=int(at.sum()))]
    m[1] = GAP
    if T > 2:
        m[2] = ord("X")
    return np.ascontiguousarray(m)


def pure(T, K, seed=0):
    """only the 20 letters and '-': a random ancestor, taxon t a copy with a share of .08 + .02 (t % 8) of its columns redrawn and 5 % '-'.
    Related rows: every pair's table is diagonally dominant once K is a few hundred, so LogDet distances exist"""
    rng = np.random.RandomState(2000 + seed)
    anc = AA[rng.randint(0, 20, size=K)]
    m = np.tile(anc, (T, 1))
    for t in range(T):
        at = rng.random_sample(K) < .08 + .02 * (t % 8)
        m[t, at] = AA[rng.randint(0, 20, size=int(at.sum()))]
        m[t, rng.random_sample(K) < .05] = GAP
    return np.ascontiguousarray(m)


def jc_pair(a, b):
    """two rows of 20 a + 380 b columns whose table is exactly a I + b (J - I): LogDet distance -(19 / 20) log((a - b) / (a + 19 b))"""
    r0, r1 = [], []
    for x in range(20):
        for y in range(20):
            n = a if x == y else b
            r0 += [AA20[x]] * n
            r1 += [AA20[y]] * n
    return np.array([r0, r1], dtype=np.uint8)


def jc_distance(a, b):
    return -(19. / 20.) * np.log((a - b) / float(a + 19 * b))


def literal_pairs(T):
    return [(i, j) for i in range(T) for j in range(i + 1, T)]


def literal_subst(matrix, keep):
    """the definition as a triple loop"""
    code = {b: a for a, b in enumerate(AA20)}
    T = len(matrix)
    rows = [bytes(r) for r in np.asarray(matrix, dtype=np.uint8)]
    out = np.zeros((T * (T - 1) // 2, 20, 20), dtype=np.int32)
    for p, (i, j) in enumerate(literal_pairs(T)):
        for k in np.asarray(keep).tolist():
            a, b = code.get(rows[i][k]), code.get(rows[j][k])
            if a is not None and b is not None:
                out[p, a, b] += 1
    return out


def strict_subset(K, seed=0):
    """an ascending strict subset of the K columns (K > 1), about two thirds of them, the last column among them"""
    rng = np.random.RandomState(3000 + seed)
    keep = np.flatnonzero(rng.random_sample(K) < .66)
    return np.unique(np.append(keep[keep != 0], K - 1)).astype(np.int64)


class Sm:
    """what tree() and bootstrap() read of a phy.Supermatrix, `subst` included (None until logdet asks for it)"""

    def __init__(self, matrix, keep=None):
        from swiftortho_amd import phy
        self.matrix = np.ascontiguousarray(matrix, dtype=np.uint8)
        self.taxa = [b"t%d" % k for k in range(len(self.matrix))]
        self.keep = np.arange(self.matrix.shape[1], dtype=np.int64) if keep is None else np.asarray(keep, dtype=np.int64)
        self.cmp, self.same = phy.pair_counts(self.matrix, self.keep)
        self.subst = None
        self.stats = {}


@functools.lru_cache(maxsize=None)
def tree_case():
    """-> (matrix, B, seed) for the end-to-end trees: a `pure` supermatrix of 7 taxa x 700 columns.  The designed `conflict` case of
    tests/phy_boot_inputs.py does not survive logdet (its columns hold two letters: 18 residues never occur), so this one stands in;
    tests/test_phy_subst.py asserts on the CPU that under logdet at most a third of its 12 replicates are dropped"""
    return pure(7, 700, 5), 12, 2 ** 64 - 1
