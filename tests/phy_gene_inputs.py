"""Designed inputs for the gene concordance factors (swiftortho_amd/phy.py family_counts .. gene_concordance; csrc/phy.hip so_phy_gene*).

A family's block is built directly from SPLIT COLUMNS: for a planted tree over the taxa the family holds, a column per split carries one
residue on one side and another on the other side; absent taxa are '-'.  With several columns per inner split and a column per leaf the
p-distances are an additive metric with no zero off the diagonal, so neighbour joining recovers the planted tree, and what a family
decides and holds is known in closed form (expected_concordance: Python sets, none of the code under test).

DROPPED FAMILIES.  A family is dropped when two of its present taxa share no compared column.  Every input says how many it drops
(`.dropped`), tests/test_phy_gene.py asserts that number from the numpy definitions, and it is zero wherever dropping is not the point:
    hand_case()            1   (the family named "disjoint")
    edge_case(T)           1   (the one named "dropped"), for every T of GPU_TAXA
    wide_case(T)           0   for the T of WIDE_TAXA
    width_case()           0
    batch_case(F)          0
    ghost_case()           0
    script_case()          0
    script_case("all_dropped")   2 of 2
"""
import functools

import numpy as np

import phy_inputs as pin

GAP = 45
GPU_TAXA = (4, 5, 63, 64, 65, 130)          # the tile (64) and word (64) edges of the kernels
WIDE_TAXA = (640, 641)                      # the two sides of the walk's LDS tier
WIDTHS = (0, 1, 15, 16, 17, 63, 64, 65, 3000)   # kept columns of a family: the 16-byte padding, a neighbour's bytes, more than one LDS chunk (128 columns)
FORCED_BATCH = 3                            # SOHIT_PHY_GENE_BATCH of the batch tests: F = 1, 3 and 4


# ---------------------------------------------------------------------------------------------------------
# planted trees and their columns
# ---------------------------------------------------------------------------------------------------------
def caterpillar(order):
    """the inner splits of the caterpillar ((o0, o1), o2, .., o[n-1]): {o0, o1}, {o0, o1, o2}, .. up to n - 2 members -> [frozenset]"""
    return [frozenset(order[:k]) for k in range(2, len(order) - 1)]


def nni(order):
    """the caterpillar one nearest-neighbour interchange away: o1 and o2 change places, so {o0, o2} stands where {o0, o1} stood"""
    order = list(order)
    order[1], order[2] = order[2], order[1]
    return order


def letters(k):
    """two different residues for column k"""
    return pin.AA[k % 20], pin.AA[(k + 1 + (k // 20) % 19) % 20]


def planted_block(T, order, copies=3, first=0):
    """uint8[T, n_cols]: `copies` columns per inner split of caterpillar(order), one column per leaf; taxa outside `order` are '-'.  Column
    numbers from `first` choose the residues, so no two columns of a table look alike"""
    order = list(order)
    sides = [s for s in caterpillar(order) for _ in range(copies)] + [frozenset([t]) for t in order]
    m = np.full((T, len(sides)), GAP, dtype=np.uint8)
    for c, side in enumerate(sides):
        on, off = letters(first + c)
        m[order, c] = off
        m[sorted(side), c] = on
    return m


class Case:
    """a supermatrix of planted families: what gene_concordance() reads of a phy.Supermatrix, and what is known about it"""

    def __init__(self, T, blocks, names=None, keep=None, dropped=0):
        from swiftortho_amd import phy
        self.matrix = np.ascontiguousarray(np.concatenate([b for b in blocks if b.shape[1]] or [np.zeros((T, 0), dtype=np.uint8)], axis=1))
        self.col_off = np.concatenate([[0], np.cumsum([b.shape[1] for b in blocks])]).astype(np.int64)
        self.taxa = [b"t%d" % k for k in range(T)]
        self.keep = np.arange(self.matrix.shape[1], dtype=np.int64) if keep is None else np.asarray(keep, dtype=np.int64)
        self.cmp, self.same = phy.pair_counts(self.matrix, self.keep)
        self.stats = {}
        self.names = names or ["f%d" % k for k in range(len(blocks))]
        self.dropped = dropped


def canonical(side, present):
    """the side of a split of the present taxa that does not hold their lowest taxon"""
    side, present = frozenset(side) & frozenset(present), frozenset(present)
    return present - side if min(present) in side else side


def expected_concordance(ref_sides, families):
    """closed form.  ref_sides: the clades of the printed tree, join by join (sets); families: [(present taxa, inner splits of the planted
    tree, dropped)] -> (decisive, concordant) lists"""
    dec, con = [0] * len(ref_sides), [0] * len(ref_sides)
    for present, splits, dropped in families:
        if dropped:
            continue
        present = frozenset(present)
        held = {canonical(s, present) for s in splits}
        for k, side in enumerate(ref_sides):
            a, b = frozenset(side) & present, present - frozenset(side)
            if len(a) >= 2 and len(b) >= 2:
                dec[k] += 1
                con[k] += canonical(a, present) in held
    return dec, con


def words_sets(splits, T):
    """uint64[S, W] -> [frozenset of taxa]"""
    return [frozenset(t for t in range(T) if (int(row[t >> 6]) >> (t & 63)) & 1) for row in np.asarray(splits, dtype=np.uint64)]


# ---------------------------------------------------------------------------------------------------------
# the hand table: eight taxa
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hand_case():
    """eight taxa, tree A the caterpillar 0 .. 7.  Families (name: present taxa, planted tree):
        A_all      all, A                     A_all2     all, A (so that A outvotes B in the supermatrix)
        B_all      all, B = nni(A): holds {0, 2} for {0, 1}
        no_taxon0  1 .. 7, A                  its lowest present taxon is 1
        three      {2, 5, 6}, -               decisive for nothing
        no_1       all but 1, A               the split {0, 1} turns trivial for it ({0}): not decisive there
        B_no_2     all but 2, B               B without 2 holds {0, 1} again
        empty      no kept column
        disjoint   {3, 4, 5, 6, 7}, A, but taxa 3 and 4 share no column: DROPPED
    -> (Case, [(present, splits, dropped)] per family)"""
    T = 8
    A = list(range(T))
    fams, blocks, names, first = [], [], [], 0

    def add(name, order, tree_order=None, block=None):
        nonlocal first
        b = planted_block(T, tree_order or order, first=first) if block is None else block
        first += b.shape[1]
        blocks.append(b), names.append(name)
        fams.append((frozenset(order), caterpillar(tree_order or order) if len(order) >= 4 else [], name == "disjoint"))

    add("A_all", A)
    add("A_all2", A)
    add("B_all", A, nni(A))
    add("no_taxon0", A[1:])
    add("three", [2, 5, 6])
    add("no_1", [0] + A[2:])
    add("B_no_2", [0, 1] + A[3:], [t for t in nni(A) if t != 2])       # B without taxon 2: the caterpillar 0, 1, 3, ..
    add("empty", [], block=np.zeros((T, 0), dtype=np.uint8))
    d = planted_block(T, [3, 4, 5, 6, 7], first=first)
    d = np.concatenate([d, d], axis=1)
    d[3, d.shape[1] // 2:] = GAP                             # taxon 3 keeps the first copy ..
    d[4, :d.shape[1] // 2] = GAP                             # .. taxon 4 the second: no column holds both
    add("disjoint", [3, 4, 5, 6, 7], block=d)
    return Case(T, blocks, names, dropped=1), fams


@functools.lru_cache(maxsize=None)
def ghost_case():
    """eight taxa, three families on tree A and one, "ghost", on A without taxon 5 -- whose block begins with a column that is NOT kept and
    holds the only residue taxon 5 has there.  Presence comes from the kept columns: taxon 5 is absent from ghost, and nothing is dropped"""
    T = 8
    A = list(range(T))
    blocks = [planted_block(T, A, first=40 * k) for k in range(3)]
    ghost = np.full((T, 1), GAP, dtype=np.uint8)
    ghost[5, 0] = pin.AA[7]
    blocks.append(np.concatenate([ghost, planted_block(T, [t for t in A if t != 5], first=120)], axis=1))
    total = sum(b.shape[1] for b in blocks)
    at = total - blocks[-1].shape[1]
    return Case(T, blocks, ["A0", "A1", "A2", "ghost"], keep=[c for c in range(total) if c != at])


# ---------------------------------------------------------------------------------------------------------
# the families every kernel edge needs, at T taxa
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_case(T):
    """T taxa, tree A the caterpillar 0 .. T - 1; families on A over all taxa (twice), on B, lacking taxon 0, lacking the last taxon of a
    word (63 where there is one, else T - 1), with exactly 3 and exactly 4 present taxa, with no kept column, and one DROPPED (its first two
    present taxa share no column)"""
    A = list(range(T))
    last = 63 if T > 64 else T - 1
    plans = [("A_all", A, A), ("A_all2", A, A), ("B_all", A, nni(A) if T >= 5 else A), ("no_taxon0", A[1:], A[1:]), ("no_word_end", [t for t in A if t != last], None),
             ("three", A[-3:], None), ("four", ([0] + A[-3:]) if T > 4 else A, None), ("empty", [], None), ("dropped", A[-4:], None)]
    blocks, names, fams, first = [], [], [], 0
    for name, order, tree_order in plans:
        tree_order = tree_order or order
        if not order:
            b = np.zeros((T, 0), dtype=np.uint8)
        elif len(order) < 4:
            b = planted_block(T, order, first=first)
        else:
            b = planted_block(T, tree_order, first=first)
        if name == "dropped":
            b = np.concatenate([b, b], axis=1)
            b[order[0], b.shape[1] // 2:] = GAP
            b[order[1], :b.shape[1] // 2] = GAP
        first += b.shape[1]
        blocks.append(b), names.append(name)
        fams.append((frozenset(order), caterpillar(tree_order) if len(order) >= 4 else [], name == "dropped"))
    return Case(T, blocks, names, dropped=1), fams


@functools.lru_cache(maxsize=None)
def wide_case(T):
    """T taxa on both sides of the walk's LDS tier, three families on the caterpillar: every taxon; 200 taxa without taxon 0 and without
    taxon 63, the last of the first word; 70 taxa from 300 on.  (Few families: the numpy walk of 640 taxa takes a second.)"""
    orders = [list(range(T)), [t for t in range(1, 202) if t != 63], list(range(300, 370))]
    blocks, first = [], 0
    for order in orders:
        blocks.append(planted_block(T, order, copies=1, first=first))
        first += blocks[-1].shape[1]
    return Case(T, blocks)


@functools.lru_cache(maxsize=None)
def width_case(T=65):
    """families of WIDTHS kept columns side by side on a random table with few letters and a tenth of gaps, whose rows all differ; kept
    columns are every column but each family's first (so keep has holes and a family of width 0 owns one dropped column).  No family
    is dropped: every pair of taxa shares a column in each (asserted on the CPU)"""
    rng = np.random.RandomState(5)
    blocks, keep, at = [], [], 0
    for w in WIDTHS:
        b = pin.AA[rng.randint(0, 4, size=(T, w + 1))]
        b[rng.random_sample(b.shape) < (.1 if w >= 15 else 0.)] = GAP
        if w == 1:
            b[T // 2:, 1] = GAP                 # the family of one column holds half of the taxa
        if w >= 15:
            b[:, 1] = pin.AA[rng.randint(0, 4, size=T)]   # a column without a gap: every pair shares it
        blocks.append(b)
        keep += list(range(at + 1, at + w + 1))
        at += w + 1
    c = Case(T, blocks, ["w%d" % w for w in WIDTHS], keep=keep)
    assert len({r.tobytes() for r in c.matrix}) == T
    return c


@functools.lru_cache(maxsize=None)
def batch_case(F, T=9):
    """F families over nine taxa, alternately on A, on B and on A without taxon F % T"""
    A = list(range(T))
    blocks, first = [], 0
    for f in range(F):
        order = [A, nni(A), [t for t in A if t != (f + 1) % T]][f % 3]
        blocks.append(planted_block(T, order, first=first))
        first += blocks[-1].shape[1]
    return Case(T, blocks)


# ---------------------------------------------------------------------------------------------------------
# a hit file for scripts/rbh2phy.py: ten taxa, families that lack one
# ---------------------------------------------------------------------------------------------------------
SCRIPT_TAXA = [b"A", b"B", b"C", b"D", b"E", b"F", b"G", b"H", b"I", b"J"]


@functools.lru_cache(maxsize=None)
def script_case(kind="plain", length=40):
    """-> (FASTA, 17-column .sc text).  Ten taxa diverged along a caterpillar; a gene per taxon and family, every pair of a family aligned
    (the score the identical columns); A holds one gene more and is the reference.
    plain: four families; family 1 lacks J, family 2 lacks B (nine of ten taxa: the core table keeps them).
    all_dropped: two families; in family 0 the rows of B cover the anchor's first half and those of C its second half, in family 1 D and E
    do the same -- every family has two present taxa without a shared column, the supermatrix as a whole has none"""
    rng = np.random.RandomState(61)
    n = len(SCRIPT_TAXA)

    def mutate(seq, k):
        seq = seq.copy()
        at = rng.choice(len(seq), size=k, replace=False)
        seq[at] = pin.AA[(np.searchsorted(np.sort(pin.AA), seq[at]) + 1 + rng.randint(0, 18, size=k)) % 20]
        return seq

    if kind == "plain":
        plans = [({}, None), ({}, 9), ({}, 1), ({}, None)]
    else:
        h = length // 2
        plans = [({1: (1, h), 2: (h + 1, length)}, None), ({3: (1, h), 4: (h + 1, length)}, None)]
    fasta, rows = [], []
    for f, (spans, missing) in enumerate(plans):
        node = pin.AA[rng.randint(0, 20, size=length)]
        seqs = []
        for t in range(n):                     # the caterpillar: every taxon leaves the trunk after two more changes on it
            seqs.append(mutate(node, 2))
            node = mutate(node, 2)
        here = [t for t in range(n) if t != missing]
        for t in here:
            fasta.append(b">" + SCRIPT_TAXA[t] + b"|f%d\n" % f + seqs[t].tobytes() + b"\n")
        for x in here:
            for y in here:
                if x == y:
                    continue
                lo, hi = spans.get(y if x == 0 else x if y == 0 else -1, (1, length))
                same = int((seqs[x][lo - 1:hi] == seqs[y][lo - 1:hi]).sum())
                ln = hi - lo + 1
                rows.append(b"\t".join([SCRIPT_TAXA[x] + b"|f%d" % f, SCRIPT_TAXA[y] + b"|f%d" % f, b"%.2f" % (100. * same / ln), b"%d" % ln, b"%d" % (ln - same), b"0",
                                        b"%d" % lo, b"%d" % hi, b"%d" % lo, b"%d" % hi, b"1e-20", b"%d" % same, b"%d" % length, b"%d" % length, b"%d" % same, b"%d" % ln,
                                        b"%dM" % ln]) + b"\n")
    fasta.append(b">A|extra\n" + pin.AA[rng.randint(0, 20, size=length)].tobytes() + b"\n")
    return b"".join(fasta), b"".join(rows)
