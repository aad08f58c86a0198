"""TEST INFRASTRUCTURE -- entry lists aimed at the edges of the affinity-propagation kernels (swiftortho_amd/csrc/apc.hip): rows and
columns at the lane / wave split and at the 64-entry chunk bounds, ties at named positions, directed lists, rows with two diagonal
entries, a column whose sum depends on its order, non-finite / denormal / signed-zero scores.  Raw (row, col, score, n_genes) for
find_cluster.device_apc and apc_numpy_oracle.numpy_apc -- no text parsing.  tests/test_apc_edges.py asserts from the oracle alone that
every input holds what its name promises; tests/test_gpu_apc_edges.py runs them on the device."""
import functools
import os
import re

import numpy as np

from conftest import ROOT

W = 64                                  # entries per chunk of the wave kernels = lanes of a wave


def _lane_max():
    src = open(os.path.join(ROOT, "swiftortho_amd", "csrc", "apc.hip")).read()
    m = re.search(r"^#define\s+APC_LANE_MAX\s+(\d+)u?\b", src, re.M)
    if not m:
        raise RuntimeError("APC_LANE_MAX not found in swiftortho_amd/csrc/apc.hip")
    return int(m.group(1))


LM = _lane_max()                        # longest row / column one lane walks alone
LENGTHS = (LM, LM + 1, W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 3 * W + 1)
ALL_DAMPS = (0.0, 0.5, 0.9, 0.999, 1.0)
ROUNDS = (1, 2, 3, 10)


def same_bits(x, y):
    """float32 arrays equal bit for bit -- the sign of a zero included -- where neither is a NaN, and NaN at the same positions (the
    payload and sign of a NaN are not compared: x86 and the GPU give different default NaNs for inf - inf)"""
    x, y = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)
    if x.shape != y.shape:
        return False
    nx, ny = np.isnan(x), np.isnan(y)
    return bool(np.array_equal(nx, ny) and np.array_equal(x.view(np.uint32)[~nx], y.view(np.uint32)[~ny]))


def _pack(entries, n):
    row = np.array([e[0] for e in entries], dtype=np.int32)
    col = np.array([e[1] for e in entries], dtype=np.int32)
    with np.errstate(over="ignore"):
        score = np.array([e[2] for e in entries], dtype=np.float64).astype(np.float32)
    assert len(row) == 0 or (0 <= min(row.min(), col.min()) and max(row.max(), col.max()) < n)
    return row, col, score, int(n)


def _mirrored(pairs, prefs):
    """(X, Y, w) -> (X, Y, w), (Y, X, w) as fc2mat writes them, then one preference entry per gene in number order"""
    out = []
    for x, y, w in pairs:
        out += [(x, y, w), (y, x, w)]
    return out + [(g, g, p) for g, p in enumerate(prefs)]


# ---- A: one hub whose row and column hold exactly L entries -----------------------------------------------------------------------
HEAVY_POSITIONS = (0, LM - 1, LM, W - 2, W - 1, W, W + 1)


def star_leaves(L, hub):
    """the hub's leaves in the order of its row: position j of the hub's row (and column) is leaf star_leaves(L, hub)[j]; position
    L - 1 is the hub's preference entry"""
    return [g for g in range(L) if g != hub]


def star(L, hub=0, heavy=(), weight=1.0, heavy_weight=4.0, pref=-3.0):
    """L genes: `hub` and L - 1 leaves of equal weight, leaf entries in gene order, the leaves at the row positions in `heavy`
    (those that exist) with a larger weight; the hub's row and column end with its preference entry"""
    leaves = star_leaves(L, hub)
    pairs = [(hub, g, heavy_weight if j in heavy else weight) for j, g in enumerate(leaves)]
    return _mirrored(pairs, [pref] * L), L


def heavy_of(L):
    return tuple(sorted({p for p in HEAVY_POSITIONS + (L - 2,) if 0 <= p < L - 1}))


# ---- B: two hubs sharing most leaves ---------------------------------------------------------------------------------------------
def two_hub_pairs(L1, L2, seed, private=4):
    """gene 0 a bystander (its preference entry only), hubs 1 and 2 with L1 - 1 and L2 - 1 leaves, all but `private` of the shorter
    hub's shared, weights drawn from (1, 2.5, 2.5, 10), one extra gene hanging on the first leaf; pairs in a seeded order
    -> (pairs with x < y, number of genes)"""
    rng = np.random.default_rng(seed)
    shared = min(L1, L2) - 1 - private
    first = 3
    sh = list(range(first, first + shared))
    own1 = list(range(first + shared, first + shared + L1 - 1 - shared))
    own2 = list(range(own1[-1] + 1, own1[-1] + 1 + L2 - 1 - shared))
    extra = own2[-1] + 1
    pairs = [(1, g) for g in sh + own1] + [(2, g) for g in sh + own2] + [(sh[0], extra)]
    ws = rng.choice([1.0, 2.5, 2.5, 10.0], len(pairs)).tolist()
    order = rng.permutation(len(pairs)).tolist()
    return [(pairs[o][0], pairs[o][1], ws[o]) for o in order], extra + 1


def two_hubs(L, seed, pref=-20.0):
    pairs, n = two_hub_pairs(L, L, seed)
    return _mirrored(pairs, [pref] * n), n


# ---- C: directed lists -----------------------------------------------------------------------------------------------------------
def one_column(L, seed=5):
    """C1: column 0 holds exactly L entries -- its own diagonal in the middle of the list and L - 1 rows i -> 0 of one entry, every
    third with a preference entry of its own (two entries): a column for the wave next to rows for the lane"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(1, L):
        out.append((i, 0, float(rng.choice([0.5, 2.0, 2.0, 7.0]))))
        if i % 3 == 0:
            out.append((i, i, -1.5))
        if i == L // 2:
            out.append((0, 0, -2.5))
    return out, L


def one_row(L, seed=5):
    """C2: the transpose of C1 -- row 0 of L entries next to columns of one or two"""
    e, n = one_column(L, seed)
    return [(k, i, s) for i, k, s in e], n


def odd_genes():
    """C3: hub 2 with a row of W + 1 entries and no diagonal entry, gene 3 without any entry, hub 4 with LM + 1 entries, its preference
    among them, gene 6 only ever a column, gene 0 only ever a row; the other genes point at both hubs, some without a preference"""
    n = W + 12
    others = [g for g in range(n) if g not in (0, 2, 3, 4)]
    out = [(0, 2, 1.0), (0, 4, 2.0)]
    for j, g in enumerate(others[:W + 1]):
        out.append((2, g, (1.0, 2.5, 2.5)[j % 3]))
    for j, g in enumerate(others[:LM]):
        out.append((4, g, (2.5, 1.0)[j % 2]))
        if j == 7:
            out.append((4, 4, -2.0))
    for j, g in enumerate(others):
        if g == 6:
            continue
        out.append((g, 2, (1.0, 2.5, 2.5)[j % 3]))
        if j % 2:
            out.append((g, 4, 1.0))
        if j % 4:
            out.append((g, g, -2.0))
    return out, n


def ring(n):
    """C4: n rows and n columns of two entries each"""
    out = []
    for i in range(n):
        out += [(i, i, -1.0 - (i % 3)), (i, (i + 1) % n, (1.0, 2.5)[i % 2])]
    return out, n


def full(n=LM + 2, seed=9):
    """C5: the complete graph with preferences, every row and column n > LM entries: nothing for the lane kernels"""
    rng = np.random.default_rng(seed)
    pairs = [(i, j, float(rng.choice([1.0, 2.5, 2.5, 10.0, 0.25]))) for i in range(n) for j in range(i + 1, n)]
    order = rng.permutation(len(pairs)).tolist()
    return _mirrored([pairs[o] for o in order], [-4.0] * n), n


# ---- D: a row with two diagonal entries ------------------------------------------------------------------------------------------
def two_diag(L, swap=False, leaf=0.01, diags=(-3.0, 0.75), pref=-5.0):
    """hub 1 with L - 2 leaves of a small weight and two diagonal entries of different scores: the first at position 5 of its row, the
    second -- not the preference -- the row's last entry (for L > W: in another chunk).  The leaf weights are small enough that
    d5 + d4 - max(0, R) stays below 0, so which diagonal entry `diag5` comes from shows in A."""
    d = diags[::-1] if swap else diags
    leaves = [g for g in range(L - 1) if g != 1]
    assert len(leaves) == L - 2
    out = []
    for j, g in enumerate(leaves):
        if j == 5:
            out.append((1, 1, d[0]))
        out += [(1, g, leaf), (g, 1, leaf)]
    out += [(g, g, pref) for g in leaves] + [(1, 1, d[1])]
    return out, L - 1


# ---- E: a column whose sum shows the order of its entries ---------------------------------------------------------------------------
TINY, QUARTER_ULP = 3 * 2.0 ** -55, 2.0 ** -24


def ordered_column(n, tiny_at, small_at, one_at):
    """column 0: rows i -> 0 at column positions 0 .. n - 1, all of score 0 except 3 * 2^-55 at the two positions `tiny_at`, 2^-24
    at `small_at` and 1.0 at `one_at`; then the diagonal entry (0, 0, 0.0).  After one round R = (1 - damp) * s exactly, and the
    diagonal's A is the float32 of (1 - damp) * the float64 sum in entry order: tiny + tiny + 2^-24 + 1 rounds up to 1 + 2^-23,
    1 + 2^-24 + tiny + tiny rounds to 1."""
    s = [0.0] * n
    s[tiny_at[0]] = s[tiny_at[1]] = TINY
    s[small_at], s[one_at] = QUARTER_ULP, 1.0
    return [(i + 1, 0, v) for i, v in enumerate(s)] + [(0, 0, 0.0)], n + 1


def e_cases():
    """name -> (builder arguments, bits of the diagonal's A after one round at damp 0, at damp 0.5)"""
    up, down = (0x3F800001, 0x3E800001), (0x3F800000, 0x3E800000)
    out = {}
    for tag, n, lo in (("lane", LM - 1, LM - 3), ("w", W + 6, W - 1), ("2w", 2 * W + 6, 2 * W - 1)):
        hi = lo + 1                                                     # lo | hi straddle a chunk bound (lane: the column's end)
        out["E_%s_tiny_first" % tag] = ((n, (0, 1), lo, hi), up)
        out["E_%s_one_first" % tag] = ((n, (lo, hi), 1, 0), down)
        out["E_%s_tiny_straddle" % tag] = ((n, (lo, hi), hi + 1, hi + 2) if tag != "lane" else (n, (lo - 2, lo - 1), lo, hi), up)
        out["E_%s_one_straddle" % tag] = ((n, (hi + 1, hi + 2), hi, lo) if tag != "lane" else (n, (lo, hi), lo - 1, lo - 2), down)
    out["E_w_head_tiny_first"] = ((W + 6, (0, 1), 2, 3), up)            # all four inside the first chunk
    out["E_w_head_one_first"] = ((W + 6, (2, 3), 1, 0), down)
    return out


# ---- F: non-finite and extreme scores ------------------------------------------------------------------------------------------------
F_HUB = 3


def f_base(L):
    return star(L, F_HUB, heavy=(10, W - 1, W))


def with_scores(entries, changes):
    """entries with the scores of the (row, col) pairs in `changes` replaced (every entry of that pair)"""
    return [(i, k, changes.get((i, k), s)) for i, k, s in entries]


def f_cases():
    inf, nan = float("inf"), float("nan")
    out = {}
    for L in (W + 6, 20):
        base, n = f_base(L)
        leaves = star_leaves(L, F_HUB)
        tag = "F%d" % L
        spots = [p for p in (0, 10, W) if p < L - 1]                  # lane 0 of both chunks of the hub's row, and an inner lane
        for name, v in (("pinf", inf), ("ninf", -inf), ("nan", nan)):
            for p in spots:
                out["%s_%s_at%d" % (tag, name, p)] = (with_scores(base, {(F_HUB, leaves[p]): v}), n)
        out[tag + "_nan_both_ways"] = (with_scores(base, {(F_HUB, leaves[1]): nan, (leaves[1], F_HUB): nan}), n)
        out[tag + "_nan_lane0_each_chunk"] = (with_scores(base, {(F_HUB, leaves[p]): nan for p in (0, W) if p < L - 1}), n)
        out[tag + "_pinf_pref"] = (with_scores(base, {(F_HUB, F_HUB): inf}), n)
        out[tag + "_nan_pref"] = (with_scores(base, {(leaves[2], leaves[2]): nan, (F_HUB, F_HUB): nan}), n)
        blind = {(F_HUB, g): (nan, -inf)[j % 2] for j, g in enumerate(leaves)}
        blind[(F_HUB, F_HUB)] = -inf
        blind[(leaves[4], F_HUB)], blind[(leaves[4], leaves[4])] = nan, -inf
        out[tag + "_blind_rows"] = (with_scores(base, blind), n)
        big = {(F_HUB, leaves[p]): 3e38 for p in spots}
        big.update({(leaves[p], F_HUB): 3e38 for p in spots})
        big.update({(g, g): -3e38 for g in range(n)})
        out[tag + "_overflow"] = (with_scores(base, big), n)
        out[tag + "_parsed_1e39"] = (with_scores(base, {(F_HUB, leaves[5]): 1e39, (leaves[5], F_HUB): 1e39}), n)
        rng = np.random.default_rng(L)
        tiny = {}
        for j, g in enumerate(leaves):
            tiny[(F_HUB, g)] = tiny[(g, F_HUB)] = float(10 ** rng.uniform(-44, -39))
        tiny.update({(g, g): -float(10 ** rng.uniform(-44, -39)) for g in range(n)})
        out[tag + "_tiny"] = (with_scores(base, tiny), n)
        zeros = {(F_HUB, g): -0.0 for j, g in enumerate(leaves) if j % 2}
        zeros.update({(g, F_HUB): -0.0 for j, g in enumerate(leaves) if j % 3 == 0})
        zeros.update({(g, g): -0.0 for j, g in enumerate(leaves) if j % 4 == 0})
        out[tag + "_signed_zeros"] = (with_scores(base, zeros), n)
    return out


F_DAMPS = {"overflow": (0.0, 0.5), "tiny": (0.5, 0.9), "signed_zeros": (0.0, 0.5, 0.9)}


# ---- the registry ----------------------------------------------------------------------------------------------------------------------
def _registry():
    """name -> (family, thunk giving (entries, n_genes), damping factors)"""
    reg = {}
    for L in LENGTHS:
        for hub in (0, 5):
            reg["A_L%d_hub%d_ties" % (L, hub)] = ("A", functools.partial(star, L, hub), ALL_DAMPS)
            reg["A_L%d_hub%d_heavy" % (L, hub)] = ("A", functools.partial(star, L, hub, heavy_of(L)), ALL_DAMPS)
    for L, seed in ((LM + 1, 1), (W + 1, 2), (2 * W + 1, 3)):
        reg["B_L%d" % L] = ("B", functools.partial(two_hubs, L, seed), ALL_DAMPS)
    for L in LENGTHS:
        reg["C1_L%d" % L] = ("C", functools.partial(one_column, L), (0.5,))
        reg["C2_L%d" % L] = ("C", functools.partial(one_row, L), (0.5,))
    reg["C3_odd_genes"] = ("C", odd_genes, (0.5, 0.9))
    for n in (255, 256, 257):
        reg["C4_ring%d" % n] = ("C", functools.partial(ring, n), (0.5,))
    reg["C5_full"] = ("C", full, (0.5, 0.9))
    for L in (20, W + 6, 2 * W + 1):
        for swap in (False, True):
            reg["D_L%d%s" % (L, "_swapped" if swap else "")] = ("D", functools.partial(two_diag, L, swap), (0.0, 0.5, 0.9))
    for name, (args, _) in e_cases().items():
        reg[name] = ("E", functools.partial(ordered_column, *args), (0.0, 0.5))
    for name, case in f_cases().items():
        kind = name.split("_", 1)[1]
        reg[name] = ("F", (lambda c=case: c), F_DAMPS.get(kind, (0.5, 1.0)))
    return reg


REGISTRY = _registry()
NAMES = sorted(REGISTRY)
RUNS = [(name, damp) for name in NAMES for damp in REGISTRY[name][2]]          # every (input, damping factor) that is run


def family(name):
    return REGISTRY[name][0]


def rounds_of(name):
    """the hub at W + 1 and the two-hub graphs also run the reference's full 100 rounds"""
    if family(name) == "B" or name.startswith("A_L%d_" % (W + 1)):
        return ROUNDS + (100,)
    return ROUNDS


@functools.lru_cache(maxsize=None)
def entries(name):
    e, n = REGISTRY[name][1]()
    return _pack(e, n)


@functools.lru_cache(maxsize=None)
def permuted(name):
    """the same entries in a second, seeded order"""
    row, col, score, n = entries(name)
    o = np.random.default_rng(len(row) + 17).permutation(len(row))
    return row[o], col[o], score[o], n


@functools.lru_cache(maxsize=None)
def snapshots(name, damp, perm=False):
    """the oracle's (labels, R, A) after each round asked of this input, from ONE run (a run of t rounds is the first t of a longer
    one) -- computed once and shared; nobody writes to it"""
    from apc_numpy_oracle import apc_rounds
    row, col, score, n = (permuted if perm else entries)(name)
    want = (1, 2, 3) if perm else rounds_of(name)
    out = {}
    for t, snap in enumerate(apc_rounds(row, col, score, n, damp, max(want))):
        if t + 1 in want or t + 1 <= 3:
            for x in snap:
                x.setflags(write=False)
            out[t + 1] = snap
    return out


def row_lengths(row, n):
    return np.bincount(row, minlength=n)


def plan(row, col, n):
    """which rows and columns so_apc gives to the lane kernels and which to the wave kernels, restated from LM: groups of 1 .. LM
    entries / of more; empty ones to neither -> (short rows, long rows, short columns, long columns)"""
    rl, cl = np.bincount(row, minlength=n), np.bincount(col, minlength=n)
    pick = lambda ln, long_: [g for g in range(n) if ln[g] and (ln[g] > LM) == long_]
    return pick(rl, False), pick(rl, True), pick(cl, False), pick(cl, True)
