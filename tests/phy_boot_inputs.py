"""Designed inputs of the bootstrap of the species tree (swiftortho_amd/phy.py boot_columns .. bootstrap, csrc/phy.hip so_phy_boot*) and
the literal restatements its tests compare with: Python-int splitmix64, a neighbour-joining walk over Python floats and lists, the
bootstrap replicate by replicate.  Shared by tests/test_phy_boot.py (numpy definitions) and tests/test_gpu_phy_boot.py (device == numpy).

The wide inputs (NJ_WIDE_TAXA, cherries, wide_boot_case) take k_phy_nj past one pass of its 256 lanes and to both sides of its LDS limit.
Not run, on purpose:
  * 4096 taxa, the end of the u16 live list.  The numpy walk is cubic: 0.08 s per matrix at 257 taxa, 1.3 s at 641, 5.9 s at 1025, so
    about 5.9 * 4 ** 3 = 380 s at 4096 -- per matrix, before the device is asked anything.  641 is the widest input here.
  * a finite D so large that (n - 2) * D overflows.  Every Q is then inf or NaN; numpy's argmin over an all-inf Q gives its first entry,
    (0, 0), where the kernel starts from (inf, 0, 1) and never replaces it: the two disagree and neither is a tree.  Out of scope."""
import functools

import numpy as np

import phy_inputs as pin

M64 = (1 << 64) - 1
GAP = 45


# ---------------------------------------------------------------------------------------------------------
# literal restatements
# ---------------------------------------------------------------------------------------------------------
def literal_columns(seed, b, K):
    out = []
    for k in range(K):
        z = (seed + ((b << 32) + k + 1) * 0x9E3779B97F4A7C15) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        out.append(((z >> 32) * K) >> 32)
    return out


def canonical(members, T):
    """a set of taxa -> the split as a tuple of W words: the side without taxon 0"""
    c = sum(1 << t for t in members)
    if c & 1:
        c = ~c & ((1 << T) - 1)
    return tuple((c >> (64 * w)) & M64 for w in range((T + 63) // 64))


def literal_nj_splits(D):
    """the walk of nj_splits over Python floats and lists -> [tuple of W words] in join order"""
    T = len(D)
    D = [[float(x) for x in row] for row in D]
    clade = [{t} for t in range(T)]
    out = []
    n = T
    while n > 3:
        r = []
        for i in range(n):
            s = 0.0
            for k in range(n):
                s = s + D[i][k]
            r.append(s)
        best = None
        for i in range(n):
            for j in range(i + 1, n):
                q = ((n - 2) * D[i][j] - r[i]) - r[j]
                if best is None or q < best[0]:
                    best = (q, i, j)
        _, i, j = best
        dij = D[i][j]
        new = [((D[i][k] + D[j][k]) - dij) / 2. for k in range(n)]
        for k in range(n):
            D[i][k] = new[k]
            D[k][i] = new[k]
        D[i][i] = 0.0
        del D[j]
        for row in D:
            del row[j]
        clade[i] = clade[i] | clade[j]
        del clade[j]
        out.append(canonical(clade[i], T))
        n -= 1
    return out


def as_tuples(splits):
    return [tuple(int(x) for x in row) for row in np.asarray(splits).tolist()]


def literal_bootstrap(matrix, keep, B, seed, ref):
    """-> (count per ref split, ok list, splits per replicate): p distances, literal loops throughout"""
    T = len(matrix)
    ok, reps = [], []
    for b in range(B):
        cols = [int(keep[d]) for d in literal_columns(seed, b, len(keep))]
        cmp_, same = pin.literal_pair_counts(matrix, cols)
        good = all(cmp_[x][y] != 0 for x in range(T) for y in range(T))
        ok.append(good)
        reps.append(literal_nj_splits([[1. - float(same[x][y]) / float(cmp_[x][y]) for y in range(T)] for x in range(T)]) if good else None)
    count = [sum(1 for b in range(B) if ok[b] and s in reps[b]) for s in as_tuples(ref)]
    return count, ok, reps


# ---------------------------------------------------------------------------------------------------------
# distance matrices
# ---------------------------------------------------------------------------------------------------------
def additive(T, seed=0):
    """-> (edges, D float64[T, T]) of a random tree with integer branch lengths"""
    edges, D = pin.random_tree(np.random.RandomState(100 + 7 * T + seed), T)
    return edges, D.astype(np.float64)


def all_equal(T):
    D = np.ones((T, T))
    np.fill_diagonal(D, 0.)
    return D


def duplicated(T, seed=0):
    """an additive tree on T // 2 taxa, every taxon twice (T odd: the first three times): zero distances off the diagonal"""
    h = max(T // 2, 2)
    _, D = additive(h, seed)
    of = [k % h for k in range(T)]
    return D[np.ix_(of, of)].copy()


def two_minima():
    """two cherries with the same Q in different rows: (0, 1) and (2, 3) of a six-taxon tree that is symmetric in them"""
    D = np.array([[0, 2, 6, 6, 7, 7], [2, 0, 6, 6, 7, 7], [6, 6, 0, 2, 7, 7], [6, 6, 2, 0, 7, 7], [7, 7, 7, 7, 0, 4], [7, 7, 7, 7, 4, 0]], dtype=np.float64)
    return D


def random_symmetric(T, seed=0):
    """no tree at all, fractions that round: every sum order gives other last bits"""
    rng = np.random.RandomState(500 + 3 * T + seed)
    U = np.triu(rng.random_sample((T, T)) + .1, 1)
    return U + U.T


def nj_cases():
    """-> [(key, D)]"""
    out = [("two_minima", two_minima())]
    for T in (3, 4, 5, 9):
        out.append(("additive_T%d" % T, additive(T)[1]))
        out.append(("equal_T%d" % T, all_equal(T)))
    for T in (4, 5, 9):
        out.append(("duplicated_T%d" % T, duplicated(T)))
        out.append(("random_T%d" % T, random_symmetric(T)))
    return out


NJ_GPU_TAXA = (4, 5, 63, 64, 65, 128, 129)


def nj_gpu_stack(T, nb):
    """nb matrices of T taxa: random, additive, all equal (every step a tie), duplicated taxa (zero distances), random again"""
    kinds = [random_symmetric(T, 1), additive(T)[1], all_equal(T), duplicated(T), random_symmetric(T, 2), additive(T, 3)[1], duplicated(T, 5)]
    return np.stack([kinds[k % len(kinds)] for k in range(nb)])


# ---------------------------------------------------------------------------------------------------------
# wide matrices: beyond one pass of the walk's 256 lanes, and its LDS limit
# ---------------------------------------------------------------------------------------------------------
NJ_THREADS = 256          # csrc/tune.h PHY_NJ_THREADS
NJ_LDS_BYTES = 61440      # csrc/tune.h PHY_NJ_LDS_BYTES
NJ_WIDE_TAXA = (255, 256, 257, 513, 640, 641)   # one below, at and one above a pass; a third pass of one column; the two sides of the LDS limit
NJ_WIDE_KINDS = ("random", "additive", "all_equal", "duplicated")


def nj_lds_bytes(T, in_lds=True):
    """csrc/phy.hip nj_lds_bytes: the row sums (T doubles), the clade bit sets (T * W words, where they are in the LDS), two u16 live lists"""
    W = (T + 63) // 64
    return T * 8 + (T * W * 8 if in_lds else 0) + T * 4


def nj_tier(T, forced_global=False):
    """what so_phy_boot_result.nj_tier must say: 0 no walk, 1 clades in the LDS, 2 in global scratch"""
    if T < 4:
        return 0
    return 1 if not forced_global and nj_lds_bytes(T) <= NJ_LDS_BYTES else 2


def nj_wide_stack(T):
    """four matrices of T taxa, NJ_WIDE_KINDS: random (every rounding counts), additive (the tree is known), all equal (every step a tie),
    duplicated taxa (zero distances)"""
    return np.stack([random_symmetric(T, 1), additive(T)[1], all_equal(T), duplicated(T)])


@functools.lru_cache(maxsize=None)
def nj_wide_want(T, k):
    """phy.nj_splits of member k of nj_wide_stack(T), computed once per process: uint64[T - 3, W], not to be written to"""
    from swiftortho_amd import phy
    out = phy.nj_splits(nj_wide_stack(T)[k])
    out.setflags(write=False)
    return out


def additive_inner_splits(T):
    """the inner edges of the tree additive(T) was made from, as canonical word tuples"""
    edges, _ = additive(T)
    return {canonical(s, T) for s in pin.tree_splits(edges, T) if 1 < len(s) < T - 1}


def cherries(T, pairs):
    """a star of T leaves at distance 10 from the centre; each pair (x, y) is a cherry: two leaves of length 1 on a node 9 from the centre.
    D is 2 inside a cherry and 20 everywhere else off the diagonal: small integers, every Q exact, two cherries tie bit for bit"""
    D = np.full((T, T), 20.)
    np.fill_diagonal(D, 0.)
    for x, y in pairs:
        D[x, y] = D[y, x] = 2.
    return D


# (pairs, the first join, the second join): two tied cherries, the lexicographically lowest (row, column) first.  The joins are written down
# from the definition, not taken from an implementation.  At T = 600 a lane of the walk owns the columns b, b + 256, b + 512:
CHERRY_T = 600
CHERRY_CASES = (
    (((300, 301), (5, 557)), {5, 557}, {300, 301}),     # columns 301 and 557 are one lane's (45 mod 256): it meets the loser first
    (((5, 301), (300, 557)), {5, 301}, {300, 557}),     # the same lane: it meets the winner first
    (((7, 520), (8, 264)), {7, 520}, {8, 264}),         # the same lane (8 mod 256): the larger column wins on the lower row
    (((7, 450), (8, 70)), {7, 450}, {8, 70}),           # lanes 194 and 70, waves 3 and 1: the reduction across waves decides
)
# the same relative layouts on 12 taxa, for the literal walk
CHERRY_SMALL_T = 12
CHERRY_SMALL_CASES = (
    (((6, 7), (1, 11)), {1, 11}, {6, 7}),
    (((1, 7), (6, 11)), {1, 7}, {6, 11}),
    (((2, 10), (3, 5)), {2, 10}, {3, 5}),
    (((2, 9), (3, 4)), {2, 9}, {3, 4}),
)
assert all(x % NJ_THREADS == y % NJ_THREADS for (_, x), (_, y) in (c[0] for c in CHERRY_CASES[:3]))
assert [[(y % NJ_THREADS) // 64 for _, y in c[0]] for c in CHERRY_CASES[3:]] == [[3, 1]]


@functools.lru_cache(maxsize=None)
def cherry_want(k):
    """phy.nj_splits of cherries(CHERRY_T, CHERRY_CASES[k][0]), computed once per process; not to be written to"""
    from swiftortho_amd import phy
    out = phy.nj_splits(cherries(CHERRY_T, CHERRY_CASES[k][0]))
    out.setflags(write=False)
    return out


def first_difference(got, want):
    """-> (join, got words, want words) of the first row where two split arrays differ, None where they are equal"""
    bad = np.flatnonzero((np.asarray(got) != np.asarray(want)).any(axis=1))
    if not len(bad):
        return None
    j = int(bad[0])
    return j, [hex(int(x)) for x in got[j]], [hex(int(x)) for x in want[j]]


# ---------------------------------------------------------------------------------------------------------
# matrices to draw columns from
# ---------------------------------------------------------------------------------------------------------
class Sm:
    """what bootstrap() reads of a phy.Supermatrix"""

    def __init__(self, matrix, keep=None):
        from swiftortho_amd import phy
        self.matrix = np.ascontiguousarray(matrix, dtype=np.uint8)
        self.taxa = [b"t%d" % k for k in range(len(self.matrix))]
        self.keep = np.arange(self.matrix.shape[1], dtype=np.int64) if keep is None else np.asarray(keep, dtype=np.int64)
        self.cmp, self.same = phy.pair_counts(self.matrix, self.keep)
        self.stats = {}


def split_columns(T, sides, copies):
    """`copies` columns per side (a set of taxa): 'A' on the side, 'R' off it"""
    cols = []
    for side in sides:
        col = np.full(T, ord("R"), dtype=np.uint8)
        col[sorted(side)] = ord("A")
        cols += [col] * copies
    return np.stack(cols, axis=1)


def one_tree_matrix(T=9, copies=40, seed=2):
    """every column backs one tree: `copies` columns per edge of a random tree, the leaves' edges included -> (matrix, the tree's splits)"""
    edges, _ = pin.random_tree(np.random.RandomState(seed), T)
    sides = [s for s in pin.tree_splits(edges, T)]
    inner = {canonical(s, T) for s in sides if 1 < len(s) < T - 1}
    return split_columns(T, sides, copies), inner


def conflict_matrix():
    """six taxa; the leaves and the cherry (4, 5) well backed; of the ten columns that place taxon 1, 70 % back (1, 2) | rest and 30 % back
    (1, 3) | rest: few enough that some replicates draw more of the minority"""
    T = 6
    base = split_columns(T, [{k} for k in range(T)] + [{4, 5}], 25)
    return np.concatenate([base, split_columns(T, [{1, 2}], 7), split_columns(T, [{1, 3}], 3)], axis=1)


def sparse_matrix():
    """five taxa over 12 columns; taxa 3 and 4 share ONE compared column (column 0): a replicate that does not draw it has no distance for them"""
    rng = np.random.RandomState(9)
    m = pin.AA[rng.randint(0, 2, size=(5, 12))]
    m[:, 0] = pin.AA[0]
    m[3, 1:7] = GAP
    m[4, 7:] = GAP
    return m


@functools.lru_cache(maxsize=None)
def boot_cases():
    """-> ((key, Sm, B, seed, every replicate valid), ...); B = 7 for the batch edges of the device"""
    holes = pin.gap_matrix(np.random.RandomState(21), 9, 400, .15)
    gaps = (holes == GAP).sum(0)
    return (("one_tree", Sm(one_tree_matrix()[0]), 7, 1, True),
            ("conflict", Sm(conflict_matrix()), 20, 3, True),
            ("sparse", Sm(sparse_matrix()), 12, 5, False),
            ("kept_with_holes", Sm(holes, np.flatnonzero(gaps <= 1)), 7, M64, True),
            ("T65", Sm(pin.gap_matrix(np.random.RandomState(22), 65, 333, .1)), 7, 0, True),
            ("T4", Sm(pin.gap_matrix(np.random.RandomState(23), 4, 50, .1)), 7, 2, True),
            ("T3", Sm(pin.gap_matrix(np.random.RandomState(24), 3, 50, .1)), 7, 2, True))


WIDE_BOOT = ((257, 96, 8), (641, 80, 3))      # (taxa, columns, replicates), seed 1


@functools.lru_cache(maxsize=None)
def wide_boot_case(T, K, seed=1):
    """T taxa over K columns, 5 % gaps; column 0 holds one residue in every row, taxon T - 2 is gapped over columns 1 .. K / 2 - 1 and
    taxon T - 1 from column K / 2 on: the two share exactly ONE compared column, and a replicate that does not draw it is dropped
    -> Sm (with .seed)"""
    m = pin.gap_matrix(np.random.RandomState(40 + T), T, K, .05)
    m[:, 0] = pin.AA[0]
    m[T - 2, 1:K // 2] = GAP
    m[T - 1, K // 2:] = GAP
    sm = Sm(m)
    sm.seed = seed
    return sm


@functools.lru_cache(maxsize=None)
def wide_boot_want(T, K, B, model="p"):
    """-> (Sm, seed, phy.bootstrap_replicates on the host), computed once per process"""
    from swiftortho_amd import phy
    sm = wide_boot_case(T, K)
    return sm, sm.seed, phy.bootstrap_replicates(sm, B, sm.seed, model)


COUNT_TAXA = (2, 63, 64, 65, 129)
COUNT_COLS = (1, 15, 16, 17, 4097)


def count_matrix(T, L, seed=0):
    """random residues with gaps and few letters, row 1 all '-' (T = 2: the one pair shares no column)"""
    m = pin.pair_matrix(T, L, seed)
    m[1] = GAP
    return m


# ---------------------------------------------------------------------------------------------------------
# a hit file of five taxa for scripts/rbh2phy.py
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def script_case(families=3, length=30):
    """-> (FASTA, 17-column .sc text): taxa A .. E with a gene per family, diverged along ((A, B), (C, D), E); every pair of a family
    aligned end to end (`30M`), the score the identical columns; A holds one gene more and is the reference"""
    rng = np.random.RandomState(31)
    taxa = [b"A", b"B", b"C", b"D", b"E"]

    def mutate(seq, n):
        seq = seq.copy()
        at = rng.choice(len(seq), size=n, replace=False)
        seq[at] = pin.AA[(np.searchsorted(np.sort(pin.AA), seq[at]) + 1 + rng.randint(0, 18, size=n)) % 20]
        return seq

    fasta, rows = [], []
    for f in range(families):
        root = pin.AA[rng.randint(0, 20, size=length)]
        ab, cd = mutate(root, 5), mutate(root, 5)
        seqs = [mutate(ab, 3), mutate(ab, 3), mutate(cd, 3), mutate(cd, 3), mutate(root, 6)]
        for t, s in zip(taxa, seqs):
            fasta.append(b">" + t + b"|f%d\n" % f + s.tobytes() + b"\n")
        for x in range(5):
            for y in range(5):
                if x != y:
                    same = int((seqs[x] == seqs[y]).sum())
                    rows.append(b"\t".join([taxa[x] + b"|f%d" % f, taxa[y] + b"|f%d" % f, b"%.2f" % (100. * same / length), b"%d" % length, b"%d" % (length - same), b"0",
                                            b"1", b"%d" % length, b"1", b"%d" % length, b"1e-20", b"%d" % same, b"%d" % length, b"%d" % length, b"%d" % same, b"%d" % length,
                                            b"%dM" % length]) + b"\n")
    fasta.append(b">A|extra\n" + pin.AA[rng.randint(0, 20, size=length)].tobytes() + b"\n")
    return b"".join(fasta), b"".join(rows)
