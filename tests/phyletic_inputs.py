"""Designed inputs of the phyletic-profile tests (tests/test_phyletic.py, tests/test_gpu_phyletic.py) and the literal model the numpy
definition swiftortho_amd/phyletic.py `linked_pairs()` is held to.  Every designed input has a *_facts() function that asserts its
promise from numpy alone, so it runs in the CPU suite; the GPU tests compare the device call with linked_pairs() on the same inputs.

What the kernel's edges are, mirrored: a tile is 64 eligible rows a side, a lane holds 4 x 4 cells, a chunk is PP_CHUNK taxon words
(read out of csrc/tune.h), a taxon word is 64 taxa."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 64


def tune_define(name):
    """a #define of csrc/tune.h as an int"""
    text = open(os.path.join(ROOT, "swiftortho_amd", "csrc", "tune.h")).read()
    return int(re.search(r"^#define\s+%s\s+(\d+)u?\b" % name, text, re.M).group(1))


class Table:
    """what pan.MemberTable holds (the tests need no more of it)"""

    def __init__(self, row, taxon, n_rows, n_file_rows):
        self.row, self.taxon, self.n_rows, self.n_file_rows = row, taxon, n_rows, n_file_rows


def table_of_bits(bits, n_file_rows=None, twice=3, seed=11):
    """bool[R, T] -> Table: the members in an order that is not the table's, every `twice`-th of them listed twice (0: none)"""
    bits = np.asarray(bits, dtype=bool)
    r, t = np.nonzero(bits)
    if twice and len(r):
        r, t = np.concatenate([r, r[::twice]]), np.concatenate([t, t[::twice]])
    order = np.random.RandomState(seed).permutation(len(r))
    return Table(r[order].astype(np.int32), t[order].astype(np.int32), len(bits), len(bits) if n_file_rows is None else n_file_rows)


# ---- the literal model -------------------------------------------------------------------------------------------------------------------
def loop_links(table, T, n_min, n_max, k_min, num, den, deviate=None):
    """linked_pairs() as a double loop over Python sets -> (a, b, shared) as lists of ints.  deviate: one of DEVIATIONS, a single change"""
    sets = [set() for _ in range(table.n_rows)]
    for r, t in zip(np.asarray(table.row).tolist(), np.asarray(table.taxon).tolist()):
        assert 0 <= t < T
        sets[r].add(t)
    el = [r for r in range(table.n_file_rows) if n_min <= len(sets[r]) <= n_max]
    out = ([], [], [])
    for x, a in enumerate(el):
        for y in range(x + 1, len(el)):
            b = el[y]
            k = len(sets[a] & sets[b])
            u = len(sets[a]) + len(sets[b]) - (0 if deviate == "u without - k" else k)
            linked = k >= k_min and (k * den > num * u if deviate == "> for >=" else k * den >= num * u)
            if linked:
                out[0].append(x if deviate == "compacted rows" else a), out[1].append(y if deviate == "compacted rows" else b), out[2].append(k)
    return out


DEVIATIONS = ("> for >=", "u without - k", "compacted rows")


def as_lists(links):
    return (links.a.tolist(), links.b.tolist(), links.shared.tolist())


# ---- the module table --------------------------------------------------------------------------------------------------------------------
MODULE_CHECKED = ((129, 64), (200, 130), (323, 193))       # (E, T) at which module_facts holds


@functools.lru_cache(maxsize=None)
def module_bits(E, T, M=7, seed=5):
    """-> bool[E, T]: family e carries module e % M's random profile (every taxon with probability 1 / 2) with taxon (e // M) % T flipped:
    the families of a module differ in two taxa at most, those of two modules in about T / 2"""
    prof = np.random.RandomState(seed).rand(M, T) < .5
    bits = prof[np.arange(E) % M].copy()
    flip = (np.arange(E) // M) % T
    bits[np.arange(E), flip] ^= True
    bits.setflags(write=False)
    return bits


def module_table(E, T, M=7):
    return table_of_bits(module_bits(E, T, M))


def tiles_hit(a, b, el):
    """the tile pairs (I, J) that hold a linked pair; el: the eligible rows, ascending"""
    pos = np.searchsorted(np.asarray(el), np.asarray(a)) // TILE, np.searchsorted(np.asarray(el), np.asarray(b)) // TILE
    return set(zip(pos[0].tolist(), pos[1].tolist()))


def tiles_with_two_rows(E, M=7):
    """the tile pairs that hold two distinct rows of one module: all of them, but a diagonal tile of M rows or fewer (consecutive rows
    are of different modules: the last tile of 323 rows holds rows 320 .. 322 alone, the last of 129 a single row)"""
    nt = (E + TILE - 1) // TILE
    rows = lambda I: min(TILE, E - I * TILE)
    return {(I, J) for I in range(nt) for J in range(I, nt) if (I != J or rows(I) > M)}


def module_facts(ph):
    """at 3/4 and k_min = 2 the families of one module are all linked and no others (200 x 130: 2758 of 19 900 pairs = 4 C(29, 2) + 3 C(28, 2)),
    and the linked pairs hit every tile pair that holds two rows of one module -- every pair of different tiles and every full tile"""
    for E, T in MODULE_CHECKED:
        L = ph.linked_pairs(module_table(E, T), T, 1, T, 2, 3, 4)
        assert L.n_eligible == E
        same = (L.a % 7) == (L.b % 7)
        sizes = np.bincount(np.arange(E) % 7)
        assert same.all() and len(L.a) == int((sizes * (sizes - 1) // 2).sum())
        assert tiles_hit(L.a, L.b, np.arange(E)) == tiles_with_two_rows(E)
        if (E, T) == (200, 130):
            assert len(L.a) == 2758


# ---- shapes: E eligible rows among ineligible ones -----------------------------------------------------------------------------------------
SHAPE_E = (0, 1, 2, 63, 64, 65, 127, 128, 129, 323)
SHAPE_T = (1, 2, 63, 64, 65, 128, 129, 193)


class Shaped:
    """`table`, `T`, the thresholds `args` = (n_min, n_max, k_min, num, den) and `eligible`, the rows the construction means to be eligible"""

    def __init__(self, table, T, args, eligible):
        self.table, self.T, self.args, self.eligible = table, T, args, eligible


@functools.lru_cache(maxsize=None)
def shaped(E, T):
    """E eligible rows with ineligible ones between them -- after every two eligible file rows one that holds n_min - 1 taxa or (where
    n_max < T) n_max + 1 -- and behind the file rows copies of the first eligible rows, which would link with them.  From 63 taxa on the
    eligible rows are module_bits (thresholds 3/4, k_min 2, 2 <= present <= T - 2); below, family e holds taxon e % T alone (threshold 1,
    k_min 1, present = 1)"""
    if T >= 63:
        n_min, n_max, k_min, num, den = 2, T - 2, 2, 3, 4
        good = module_bits(E, T)
    else:
        n_min, n_max, k_min, num, den = 1, 1, 1, 1, 1
        good = np.zeros((E, T), dtype=bool)
        good[np.arange(E), np.arange(E) % T] = True
    low, high = np.zeros(T, dtype=bool), np.zeros(T, dtype=bool)
    low[:n_min - 1] = True
    high[:n_max + 1] = True
    rows, eligible = [], []
    for e in range(E):
        eligible.append(len(rows))
        rows.append(good[e])
        if e % 2 == 1:
            rows.append(high if (e // 2) % 2 and n_max < T else low)
    if not rows:
        rows.append(low)
    n_file = len(rows)
    rows += [good[e] for e in range(min(E, 5))]             # behind the file rows: never eligible
    bits = np.stack(rows)
    return Shaped(table_of_bits(bits, n_file), T, (n_min, n_max, k_min, num, den), eligible)


def shaped_facts(ph, E, T):
    """the eligible rows are the E meant ones (so about every third row is not, and compaction matters); from two rows of one module or
    one taxon on there are linked pairs; none of them touches a row behind the file rows"""
    s = shaped(E, T)
    L = ph.linked_pairs(s.table, T, *s.args)
    assert L.n_eligible == E and ph.eligible_rows(L.present, s.table.n_file_rows, *s.args[:2]).tolist() == s.eligible
    assert s.table.n_rows - E >= E // 2 and (E < 3 or s.eligible != list(range(E)))
    if E >= 8:
        assert len(L.a) > 0
    assert len(L.a) == 0 or int(L.b.max()) < s.table.n_file_rows
    return L


# ---- hand tables -------------------------------------------------------------------------------------------------------------------------
def hand_threshold():
    """rows 0 {0,1,2}, 1 {0,1,2,3}, 2 {0,1,3,4}, 3 {0,1,2} with every member listed twice; 6 taxa, 1 <= present <= 6.  At 3/4: (0, 1) has
    k = 3, u = 4 -- equality, linked --, (0, 2) k = 2, u = 5 and (1, 2) k = 3, u = 5 are not; row 3 equals row 0"""
    sets = [(0, 1, 2), (0, 1, 2, 3), (0, 1, 3, 4), (0, 1, 2, 0, 1, 2)]
    row = np.array([r for r, s in enumerate(sets) for _ in s], dtype=np.int32)
    tax = np.array([t for s in sets for t in s], dtype=np.int32)
    return Table(row, tax, 4, 4), 6


HAND_THRESHOLD_LINKS = {2: ([0, 0, 1], [1, 3, 3], [3, 3, 3]), 3: ([0, 0, 1], [1, 3, 3], [3, 3, 3]), 4: ([], [], [])}      # by k_min, at 3/4


def hand_bounds():
    """rows of 1, 2, 4 and 5 taxa, nested ({0}, {0,1}, {0..3}, {0..4}), then a copy of the row of 2 behind the file rows; n_min = 2,
    n_max = 4, threshold 1/2, k_min 1.  Only (1, 2) is linked: (0, 1) k = 1, u = 2 and (2, 3) k = 4, u = 5 would be but rows 0 and 3 lie
    one outside the bounds, and row 4 equals row 1 but is no file row"""
    bits = np.zeros((5, 6), dtype=bool)
    for r, n in enumerate((1, 2, 4, 5, 2)):
        bits[r, :n] = True
    return table_of_bits(bits, 4, twice=0), 6, (2, 4, 1, 1, 2)


HAND_BOUNDS_LINKS = ([1], [2], [2])


# ---- designed device inputs ---------------------------------------------------------------------------------------------------------------
def dense(E=130, T=70):
    """E families with one profile: at num = den = 1 all E (E - 1) / 2 pairs are linked, 16 per lane of a full tile"""
    bits = np.zeros((E, T), dtype=bool)
    bits[:, ::2] = True
    return table_of_bits(bits), T, (1, T, 1, 1, 1)


def lonely(E=129, T=70):
    """E eligible families of which no two have the same profile: at num = den = 1 nothing is linked"""
    bits = np.random.RandomState(3).rand(E, T) < .5
    assert len({b.tobytes() for b in bits}) == E
    return table_of_bits(bits), T, (1, T, 1, 1, 1)


def full_rows(T=4096, short=False):
    """three rows of all T taxa (short: row 1 lacks the last taxon)"""
    bits = np.ones((3, T), dtype=bool)
    if short:
        bits[1, T - 1] = False
    return table_of_bits(bits, twice=0), T


def dense_facts(ph):
    tb, T, args = dense()
    L = ph.linked_pairs(tb, T, *args)
    assert len(L.a) == 130 * 129 // 2 == 8385 and (L.shared == 35).all()
    tb, T, args = lonely()
    L = ph.linked_pairs(tb, T, *args)
    assert L.n_eligible == 129 and len(L.a) == 0


def width_facts(ph):
    """both sides of the test reach 4096 * (2^20 - 1), just under 2^32: equality links, one taxon fewer does not; and k * den above 2^31
    against a small right side (a signed comparison would part here)"""
    big = (1 << 20) - 1
    tb, T = full_rows()
    assert as_lists(ph.linked_pairs(tb, T, 1, T, 1, big, big)) == ([0, 0, 1], [1, 2, 2], [4096] * 3)
    assert as_lists(ph.linked_pairs(tb, T, 1, T, 1, 1, big)) == ([0, 0, 1], [1, 2, 2], [4096] * 3)
    tb, T = full_rows(short=True)
    assert as_lists(ph.linked_pairs(tb, T, 1, T, 1, big, big)) == ([0], [2], [4096])
    assert 4096 * big < 2 ** 32 and 4095 * big < 4096 * big


@functools.lru_cache(maxsize=None)
def larger():
    """about 2000 eligible rows x 500 taxa in 32 tile rows: 2100 families in 150 modules, of which those whose flipped profile leaves
    the bounds 230 .. 270 are not eligible -> (table, T, args)"""
    T = 500
    return table_of_bits(module_bits(2100, T, 150, seed=9)), T, (230, 270, 2, 4, 5)


STRIDE_E, STRIDE_T, STRIDE_M = 6016, 130, 61


@functools.lru_cache(maxsize=None)
def strided():
    """6016 eligible rows x 130 taxa in 61 modules: 94 full tiles a side, 4465 tile pairs -- more than twice the workgroups 256 CUs hold at eight a CU,
    the most there can be, so every workgroup walks two pairs at least, most of them in different rows of tiles.  A tile's 64 consecutive rows
    hold every module, so every tile pair, diagonal ones included, holds linked pairs: each walk emits again and again -> (table, T, args)"""
    return table_of_bits(module_bits(STRIDE_E, STRIDE_T, STRIDE_M, seed=13)), STRIDE_T, (1, STRIDE_T, 2, 3, 4)


def strided_facts(ph):
    tb, T, args = strided()
    L = ph.linked_pairs(tb, T, *args)
    nt = (STRIDE_E + TILE - 1) // TILE
    assert L.n_eligible == STRIDE_E and nt * (nt + 1) // 2 == 4465 > 2 * 8 * 256
    assert ((L.a % STRIDE_M) == (L.b % STRIDE_M)).all() and len(L.a) > 250000
    assert tiles_hit(L.a, L.b, np.arange(STRIDE_E)) == {(I, J) for I in range(nt) for J in range(I, nt)}
    return L
