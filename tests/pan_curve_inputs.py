"""Designed inputs of the pan-genome device call at the edges of its kernels (csrc/pan.hip k_pan_curve, k_pan_type), for
tests/test_pan_curve_inputs.py (CPU: the inputs hold what they claim) and tests/test_gpu_pan_curve.py (the device against numpy).

A case is everything so_pan_genome takes: the member pairs, the rows and file rows, the taxa, the two type thresholds, the genome orders
and the step thresholds S and C -- any orders and any thresholds, not only those pan.permutations and pan.step_thresholds make.  The
module also restates the three definitions (count matrix, row types, rarefaction) in plain Python loops over rows, orders and steps:
loop_counts, loop_types, loop_curves.  Nothing here comes from swiftortho_amd/pan.py or from tests/test_pan.py curves_text; the CPU test
holds the two statements against each other, and against the real script's output on the goldens u0 and l_huge.

What the kernels' bounds are, mirrored (the CPU test reads them from csrc/tune.h and csrc/pan.hip): a tile is 64 rows; a workgroup of
k_pan_curve serves 4 orders, a wave each; the LDS tier takes LDS_BYTES_PER_TAXON * T - LDS_BYTES_OFF bytes of LDS and is chosen while
that is at most PAN_LDS_BYTES; the tiles are cut into at most PAN_TILE_RANGES ranges of ceil(W / PAN_TILE_RANGES) tiles.

table(): no two taxa have the same presence column (taxon t is present with a probability of its own, rising with t), row 0 holds
every taxon, every 7th row (r % 7 == 3) is all zero, the last row holds the first and the last taxon whatever its number, about a seventh of the present pairs is listed twice and some three times, the
pairs come in any order.  The orders and thresholds of the groups are chosen so that two different orders never give the same curve.
"""
import functools
import random

import numpy as np

TILE_ROWS = 64
WAVES = 4                    # orders per workgroup of k_pan_curve
PAN_LDS_BYTES = 65536
PAN_TILE_RANGES = 256
LDS_BYTES_PER_TAXON = 80     # 8 (the tile's word) + 4 x 4 (four orders) + 8 (S, C) + 12 x 4 (counters per step, one step fewer than taxa)
LDS_BYTES_OFF = 48           # ... the counters of the step that is not there
I32_MAX = 2147483647


def lds_bytes(n_taxa):
    return LDS_BYTES_PER_TAXON * n_taxa - LDS_BYTES_OFF if n_taxa > 0 else 0


LDS_MAX_TAXA = (PAN_LDS_BYTES + LDS_BYTES_OFF) // LDS_BYTES_PER_TAXON      # the most taxa the LDS tier holds


def tile_grid(n_rows):
    """-> (W, tiles per range, ranges) as the host cuts the row tiles"""
    W = (n_rows + TILE_ROWS - 1) // TILE_ROWS
    tiles = (W + PAN_TILE_RANGES - 1) // PAN_TILE_RANGES
    return W, tiles, (W + tiles - 1) // tiles if tiles else 0


# ---------------------------------------------------------------------------------------------------------
# the definitions, in loops
# ---------------------------------------------------------------------------------------------------------
def loop_counts(row, taxon, n_rows, n_taxa):
    """-> counts[r][t]: how often the pair (r, t) is listed"""
    counts = [[0] * n_taxa for _ in range(n_rows)]
    for r, t in zip(np.asarray(row).tolist(), np.asarray(taxon).tolist()):
        counts[r][t] += 1
    return counts


def loop_types(counts, n_file_rows, spec_max, core_min):
    """-> (type per row: 0 Specific, 1 Share, 2 Core; [core, share, specific] among the file rows)"""
    types, totals = [], [0, 0, 0]
    for r, line in enumerate(counts):
        if r >= n_file_rows:
            types.append(0)
            continue
        thr = 0
        for c in line:
            if c > 0:
                thr += 1
        if thr <= spec_max:
            ty = 0
        elif thr < core_min:
            ty = 1
        else:
            ty = 2
        types.append(ty)
        totals[2 - ty] += 1
    return types, totals


def loop_curves(counts, perm, S, C):
    """-> (core, spec, panz), each [order][step - 1]: a row at a time, an order at a time, a genome at a time"""
    perm, S, C = np.asarray(perm).tolist(), np.asarray(S).tolist(), np.asarray(C).tolist()
    n_taxa = len(S)
    core, spec, panz = ([[0] * max(n_taxa - 1, 0) for _ in perm] for _ in range(3))
    if n_taxa < 2:
        return core, spec, panz
    for line in counts:
        here = [1 if c > 0 else 0 for c in line]
        for p, order in enumerate(perm):
            ys = here[order[0]]
            cp, sp, zp = core[p], spec[p], panz[p]
            for i in range(1, n_taxa):
                yn = here[order[i]]
                if yn and ys <= S[i]:
                    sp[i - 1] += 1
                ys += yn
                if ys >= C[i]:
                    cp[i - 1] += 1
                if ys > 0:
                    zp[i - 1] += 1
    return core, spec, panz


# ---------------------------------------------------------------------------------------------------------
# tables, orders, thresholds
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(n_rows, n_taxa, seed=0):
    """-> (row, taxon) int32, read-only"""
    rng = np.random.RandomState(7919 * seed + 31 * n_rows + n_taxa)
    p = 0.15 + 0.7 * np.arange(n_taxa) / max(n_taxa - 1, 1)
    present = rng.rand(n_rows, n_taxa) < p[None, :]
    present[np.arange(n_rows) % 7 == 3] = False
    present[:1] = True
    present[-1, [0, n_taxa - 1]] = True      # the last row, which may be all a last tile holds, counts
    times = np.where(present, 1 + (rng.rand(n_rows, n_taxa) < 0.15) + (rng.rand(n_rows, n_taxa) < 0.05), 0)
    r, t = np.nonzero(present)
    r, t = np.repeat(r, times[r, t]), np.repeat(t, times[r, t])
    order = rng.permutation(len(r))
    row, tax = r[order].astype(np.int32), t[order].astype(np.int32)
    row.setflags(write=False), tax.setflags(write=False)
    return row, tax


def shuffled_orders(n_taxa, size):
    """the orders the script walks: seed 42, `size` successive shuffles of one list"""
    rng, idx, out = random.Random(42), list(range(n_taxa)), []
    for _ in range(size):
        rng.shuffle(idx)
        out.append(list(idx))
    return np.asarray(out, dtype=np.int32).reshape(size, n_taxa)


def steps_SC(n_taxa):
    """thresholds that move with the step: new while a row is in at most a third of the genomes so far, core from two thirds on.  Entry 0,
    which no step reads, holds values that would show"""
    S, C = np.zeros(n_taxa, dtype=np.int32), np.zeros(n_taxa, dtype=np.int32)
    for i in range(1, n_taxa):
        S[i], C[i] = (i + 1) // 3, max(1, (2 * (i + 1) + 2) // 3)
    if n_taxa:
        S[0], C[0] = I32_MAX, -I32_MAX
    return S, C


class Case:
    def __init__(self, name, n_rows, n_taxa, perm, n_file_rows=None, S=None, C=None, types=None, seed=0):
        self.name, self.n_rows, self.n_taxa = name, n_rows, n_taxa
        self.row, self.taxon = table(n_rows, n_taxa, seed)
        self.n_file_rows = n_rows if n_file_rows is None else n_file_rows
        self.perm = np.asarray(perm, dtype=np.int32).reshape(-1, n_taxa)
        s, c = steps_SC(n_taxa)
        self.S = s if S is None else np.full(n_taxa, S, dtype=np.int32)
        self.C = c if C is None else np.full(n_taxa, C, dtype=np.int32)
        self.spec_max, self.core_min = types if types is not None else (n_taxa // 3, max(1, (2 * n_taxa + 2) // 3))
        self.size = len(self.perm)
        self.fits_lds = lds_bytes(n_taxa) <= PAN_LDS_BYTES

    def args(self):
        """the arguments of pan.device_pan_genome, in its order"""
        return (self.row, self.taxon, self.n_rows, self.n_file_rows, self.n_taxa, self.spec_max, self.core_min, self.perm, self.S, self.C)


# ---- orders per workgroup: every remainder of size modulo 4, one and several workgroups; 0: no curve at all
SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 21)
SIZE_ROWS, SIZE_TAXA = 130, 6


def size_case(size):
    return Case('size%d' % size, SIZE_ROWS, SIZE_TAXA, shuffled_orders(SIZE_TAXA, size), n_file_rows=SIZE_ROWS - 3)


# ---- designed orders
ORDER_ROWS, ORDER_TAXA = 130, 9


def order_cases():
    T = ORDER_TAXA
    ident, sh = list(range(T)), shuffled_orders(T, 4).tolist()
    out = [Case('identity', ORDER_ROWS, T, [ident]), Case('reversed', ORDER_ROWS, T, [ident[::-1]]),
           Case('identity_reversed', ORDER_ROWS, T, [ident, ident[::-1]]),
           Case('four_alike', ORDER_ROWS, T, [sh[0]] * 4),
           Case('fifth_is_first', ORDER_ROWS, T, sh + [sh[0]]),
           Case('last_taxon_first', ORDER_ROWS, T, [[T - 1] + ident[:-1], ident])]
    for t in (2, 3):
        for size in (1, 5):
            out.append(Case('taxa%d_size%d' % (t, size), ORDER_ROWS, t, shuffled_orders(t, size)))
    return out


# ---- the row mask of the last tile, and the extreme thresholds
MASK_ROWS = (1, 63, 64, 65, 127, 128, 129)
MASK_TAXA, MASK_SIZE = 5, 5
# name -> (S, C, what the answer is): one of the two at an extreme, the other as steps_SC has it
EXTREMES = {'C0': (None, 0, 'core_all'), 'C-5': (None, -5, 'core_all'), 'C-max': (None, -I32_MAX, 'core_all'), 'C+max': (None, I32_MAX, 'core_none'),
            'S-1': (-1, None, 'spec_none'), 'S+max': (I32_MAX, None, 'spec_all')}


def mask_case(n_rows, extreme):
    S, C, _ = EXTREMES[extreme]
    return Case('rows%d_%s' % (n_rows, extreme), n_rows, MASK_TAXA, shuffled_orders(MASK_TAXA, MASK_SIZE), S=S, C=C)


# ---- the LDS bound
LDS_ROWS, LDS_SIZE = 130, 5
LDS_TAXA = (LDS_MAX_TAXA - 1, LDS_MAX_TAXA, LDS_MAX_TAXA + 1)


def lds_case(n_taxa):
    return Case('taxa%d' % n_taxa, LDS_ROWS, n_taxa, shuffled_orders(n_taxa, LDS_SIZE))


# ---- tile ranges: W tiles -- one tile per range up to 256, two up to 512, three at 513; a full, a nearly full and a one-row last tile
TILE_W = (1, 255, 256, 257, 512, 513)
TILE_TAXA, TILE_SIZE = 5, 5


def tile_rows(W):
    return (64 * W, 64 * W - 1, 64 * W - 63)


def tile_case(n_rows):
    return Case('rows%d' % n_rows, n_rows, TILE_TAXA, shuffled_orders(TILE_TAXA, TILE_SIZE), n_file_rows=max(n_rows - 3, 0))


# ---- types
TYPE_ROWS, TYPE_TAXA = 129, 5
TYPE_FILE_ROWS = (0, 63, 64, 65, 129)
TYPE_THRESHOLDS = ((5, 6), (0, 0), (0, 6), (2, 2), (-1, 3))


def type_case(n_file_rows, thresholds):
    return Case('file%d_%d_%d' % ((n_file_rows,) + thresholds), TYPE_ROWS, TYPE_TAXA, shuffled_orders(TYPE_TAXA, 2), n_file_rows=n_file_rows, types=thresholds)


# ---- shape after shape, in one process: large, tiny, the most LDS, one order
def sequence_cases():
    return [tile_case(tile_rows(TILE_W[-1])[0]), Case('one_row', 1, 2, shuffled_orders(2, 5)), lds_case(LDS_MAX_TAXA), size_case(1)]


# ---- the grid's height: 4 orders per workgroup row; GRID_ORDERS when the device's own limit takes too long to serve
GRID_ROWS, GRID_TAXA = 70, 2
GRID_ORDERS = 4 * 4096 + 1


ARG_NAMES = ('row', 'taxon', 'n_rows', 'n_file_rows', 'n_taxa', 'spec_max', 'core_min', 'perm', 'S', 'C')


def grid_case(size):
    """two taxa have two orders: every third order is (1, 0), the others (0, 1) -- a period no group of 4 shares"""
    p = np.arange(size)
    return Case('grid%d' % size, GRID_ROWS, GRID_TAXA, np.where((p % 3 == 0)[:, None], [1, 0], [0, 1]))


def served_size_limit(device_pan_genome):
    """-> the largest `size` a call serves on this device (4 x the height of a grid), as the refusal of 2^20 orders names it: a height
    of 2^18 is more than any device of this kind takes, and nothing is launched to find out"""
    import re
    try:
        device_pan_genome(*grid_case(1 << 20).args())
    except RuntimeError as e:
        m = re.search(r'the largest size served is (\d+)\)$', str(e))
        assert m and ' orders are more than one call serves' in str(e), str(e)
        limit = int(m.group(1))
        assert limit % WAVES == 0 and 0 < limit < 1 << 20
        return limit
    raise AssertionError('2^20 orders of two taxa were served: the grid height this test is about has no bound here')


def all_cases():
    """every case above but the grid's, once"""
    out = [size_case(s) for s in (0,) + SIZES] + order_cases()
    out += [mask_case(n, e) for n in MASK_ROWS for e in sorted(EXTREMES)]
    out += [lds_case(t) for t in LDS_TAXA]
    out += [tile_case(n) for W in TILE_W for n in tile_rows(W)]
    out += [type_case(f, th) for f in TYPE_FILE_ROWS for th in TYPE_THRESHOLDS]
    out += [sequence_cases()[1]]
    return out
