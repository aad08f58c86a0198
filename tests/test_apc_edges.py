"""The inputs of tests/apc_edge_inputs.py, checked without a GPU.  (1) Every builder's promise -- lengths, ties, NaN / inf / denormal
counts, observable orders -- is asserted from the oracle (tests/apc_numpy_oracle.py) alone.  (2) The four kernels of
swiftortho_amd/csrc/apc.hip are restated in Python AS WRITTEN -- the wave forms lane by lane: the log-step shuffle scan with apc_max as
spelled, the ballots, last updater, first candidate, the column sum chunk by chunk -- and that restatement equals the oracle on every
input.  (3) Single deviations of the restatement, one line each, are each told from the oracle by named inputs: the table DEVIATIONS
keeps the discriminating power of the inputs under test.  The GPU runs the same inputs in tests/test_gpu_apc_edges.py."""
import functools

import numpy as np
import pytest

import apc_edge_inputs as X
from apc_edge_inputs import LM, W, same_bits

INF = float("inf")


# ---- the kernels, restated ---------------------------------------------------------------------------------------------------------
def apc_max(a, b):
    return b if a < b else a                     # b only when strictly above; a NaN a stays


def shfl_up(v, o):
    return [v[l - o] if l >= o else v[l] for l in range(W)]       # a lane without a source keeps its own value


def scan_max(v):
    o = 1
    while o < W:
        u = shfl_up(v, o)
        v = [apc_max(u[l], v[l]) if l >= o else v[l] for l in range(W)]
        o <<= 1
    return v


def ballot(bits):
    return [l for l in range(W) if bits[l]]


def f32(values):
    with np.errstate(over="ignore"):
        return np.array(values, dtype=np.float64).astype(np.float32)


def restated_rounds(row, col, score, n, damp, rounds, dev=None):
    """yields (labels, R, A) in entry order after every round, computed the way so_apc's kernels compute them; `dev` names ONE
    deviation from the kernels as written"""
    I, K = [int(x) for x in row], [int(x) for x in col]
    S = np.asarray(score, dtype=np.float32).astype(np.float64).tolist()
    N, damp = len(I), float(damp)
    beta = 1. - damp
    rows, cols = [[] for _ in range(n)], [[] for _ in range(n)]
    for e in range(N):                                                  # stable grouping: entry order survives inside a group
        rows[I[e]].append(e), cols[K[e]].append(e)
    R, A = [0.] * N, [0.] * N
    m1, m2, d5, k1, lab = [0.] * n, [0.] * n, [0.] * n, [-1 if dev == "k1_minus1" else 0] * n, list(range(n))

    def ra_of(p):
        return R[p] + A[p]

    def change_lane(i, idx):
        ras = m1[i] if dev == "change_seeded" else -INF
        for p in idx:
            ra = ra_of(p)
            if ras < ra:
                ras, lab[i] = ra, K[p]

    def change_wave(i, idx):
        ras = m1[i] if dev == "change_seeded" else -INF
        for c in range(0, len(idx), W):
            ch = idx[c:c + W]
            have = [l < len(ch) for l in range(W)]
            ra = [ra_of(ch[l]) if have[l] else -INF for l in range(W)]
            if dev != "nan_kept":
                ra = [-INF if x != x else x for x in ra]
            inc = scan_max(ra)
            before = shfl_up(inc, 1)
            if dev != "lane0_before":
                before[0] = -INF
            up = ballot([have[l] and ra[l] > apc_max(ras, before[l]) for l in range(W)])
            if up:
                at = up[0] if dev == "first_label" else up[-1]
                ras, lab[i] = ra[at], K[ch[at]]

    def update_lane(i, idx, Rn):
        a, b, k = m1[i], m2[i], k1[i]
        for p in idx:
            ra = ra_of(p)
            if a < ra:
                a, k = ra, K[p]
            elif b < ra:
                b = ra
        m1[i], m2[i], k1[i] = a, b, k
        seen = False
        for p in idx:
            r = S[p] - (a if K[p] != k else b)
            Rn[p] = R[p] * damp + beta * r
            if K[p] == i and not (seen and dev == "first_diag"):
                seen, d5[i] = True, Rn[p]

    def update_wave(i, idx, Rn):
        a, b, k = m1[i], m2[i], k1[i]
        for c in range(0, len(idx), W):
            ch = idx[c:c + W]
            have = [l < len(ch) for l in range(W)]
            ra = [ra_of(ch[l]) if have[l] else -INF for l in range(W)]
            if dev != "nan_kept":
                ra = [-INF if x != x else x for x in ra]
            inc = scan_max(ra)
            before = shfl_up(inc, 1)
            if dev != "lane0_before":
                before[0] = -INF
            if dev == "ge_updater":
                updater = [have[l] and ra[l] >= apc_max(a, before[l]) for l in range(W)]
            else:
                updater = [have[l] and ra[l] > apc_max(a, before[l]) for l in range(W)]
            up = ballot(updater)
            if up:
                at = up[0] if dev == "first_updater" else up[-1]
                a, k = ra[at], K[ch[at]]
            mine = [ra[l] if have[l] and not updater[l] else -INF for l in range(W)]
            cm = list(mine)
            o = W // 2
            while o:                                                    # butterfly: every lane ends with the maximum of all
                cm = [apc_max(cm[l], cm[l ^ o]) for l in range(W)]
                o >>= 1
            if b < cm[0]:
                at = ballot([have[l] and not updater[l] and mine[l] == cm[l] for l in range(W)])
                b = mine[at[-1] if dev == "last_candidate" else at[0]]
        m1[i], m2[i], k1[i] = a, b, k
        seen = False
        for c in range(0, len(idx), W):
            ch = idx[c:c + W]
            for p in ch:
                r = S[p] - (a if K[p] != k else b)
                Rn[p] = R[p] * damp + beta * r
            dg = [p for p in ch if K[p] == i]
            if dg and not (seen and dev == "first_diag"):
                seen, d5[i] = True, Rn[dg[0] if dev == "first_diag" else dg[-1]]

    def new_a(p, off_diag, d4, dk):
        an = A[p] * damp
        if off_diag:
            r = R[p]
            x = (dk + d4) + -(r if r > 0. else 0.)
            add = x if x < 0. else 0.
        else:
            add = d4
        return an + beta * add

    def col_pass(k, idx, An, wave):
        def term(q):
            r = R[q]
            return r if (I[q] != k or dev == "diag_in_sum") and r > 0. else 0.
        d4 = 0.
        if not wave:
            for q in idx:
                if term(q) > 0.:
                    d4 = d4 + term(q)
        else:
            for c in range(0, len(idx), W):
                ch = idx[c:c + W]
                if dev == "rev_first_chunk" and c == 0:
                    ch = ch[::-1]
                for q in ch:
                    d4 = d4 + term(q)
        for q in idx:
            An[q] = new_a(q, I[q] != k, d4, d5[k])

    for _ in range(rounds):
        if dev == "reset_m1":
            m1 = [0.] * n
        if dev == "reset_m2":
            m2 = [0.] * n
        Rn = list(R)
        for i in range(n):
            if rows[i]:
                (update_wave if len(rows[i]) > LM else update_lane)(i, rows[i], Rn)
        R = f32(Rn).astype(np.float64).tolist()
        An = list(A)
        for k in range(n):
            if cols[k]:
                col_pass(k, cols[k], An, len(cols[k]) > LM)
        A = f32(An).astype(np.float64).tolist()
        for i in range(n):
            if rows[i]:
                (change_wave if len(rows[i]) > LM else change_lane)(i, rows[i])
        yield np.array(lab, dtype=np.int64), f32(R), f32(A)


def same_state(got, want):
    return bool(np.array_equal(got[0], want[0]) and same_bits(got[1], want[1]) and same_bits(got[2], want[2]))


@functools.lru_cache(maxsize=None)
def restated(name, damp, dev=None, upto=10):
    row, col, score, n = X.entries(name)
    return {t + 1: s for t, s in enumerate(restated_rounds(row, col, score, n, damp, upto, dev))}


def first_difference(name, damp, dev, upto=10):
    """the first round at which the restatement with deviation `dev` leaves the oracle on this input, or None"""
    want = X.snapshots(name, damp)
    for t, got in restated(name, damp, dev, upto).items():
        if t in want and not same_state(got, want[t]):
            return t
    return None


# ---- the comparison itself -----------------------------------------------------------------------------------------------------------
def test_same_bits_sees_what_array_equal_cannot():
    z, nz, nan = np.float32(0.), np.float32(-0.), np.float32("nan")
    other_nan = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]
    assert np.array_equal([z], [nz]) and not same_bits([z], [nz])                     # the sign of a zero
    assert not np.array_equal([nan], [nan]) and same_bits([nan], [nan])               # a NaN equals a NaN ...
    assert same_bits([nan, z], [other_nan, z])                                         # ... whatever its sign and payload
    assert not same_bits([nan, z], [z, nan]) and not same_bits([nan], [np.float32(INF)])
    assert not same_bits([z], [z, z])
    assert not same_bits([np.float32(1e-45)], [z]) and same_bits([np.float32(1e-45)], [np.float32(1e-45)])


def test_constants_mirror_the_kernel():
    assert LM == 32 and X.LENGTHS == (32, 33, 63, 64, 65, 127, 128, 129, 193)        # apc.hip as it stands; a change of APC_LANE_MAX
    assert len(X.NAMES) == len(set(X.NAMES))                                         # moves every input with it, and shows here
    for name in X.NAMES:
        row, col, score, n = X.entries(name)
        assert len(row) <= 1500 and row.dtype == np.int32 and score.dtype == np.float32
        assert row.min() >= 0 and col.min() >= 0 and max(row.max(), col.max()) < n   # nothing here can make the device fault


# ---- promises ------------------------------------------------------------------------------------------------------------------------
def lengths(name):
    row, col, _, n = X.entries(name)
    return np.bincount(row, minlength=n), np.bincount(col, minlength=n)


def hub_ra(name, damp, hub, t):
    """R + A of the hub's row in row order, as round t reads it (the float32 stores of round t - 1)"""
    row, _, _, _ = X.entries(name)
    _, r, a = X.snapshots(name, damp)[t - 1]
    at = np.flatnonzero(row == hub)
    return r[at].astype(np.float64) + a[at].astype(np.float64)


@pytest.mark.parametrize("L", X.LENGTHS)
def test_star_lengths_and_ties(L):
    for hub in (0, 5):
        for kind in ("ties", "heavy"):
            name = "A_L%d_hub%d_%s" % (L, hub, kind)
            row, col, score, n = X.entries(name)
            rl, cl = lengths(name)
            assert rl[hub] == L and cl[hub] == L and n == L
            assert sorted(np.delete(rl, hub).tolist()) == [2] * (L - 1)
            at = np.flatnonzero(row == hub)
            assert col[at[-1]] == hub and col[at].tolist()[:-1] == X.star_leaves(L, hub)       # stated order, preference last
            assert (0 in col[at][:-1]) == (hub != 0)                                            # gene 0: the hub, or one of its leaves
            heavy = X.heavy_of(L) if kind == "heavy" else ()
            assert [j for j in range(L - 1) if score[at[j]] != 1.0] == list(heavy)
            if kind == "heavy":
                assert set(heavy) == {p for p in (0, LM - 1, LM, W - 2, W - 1, W, W + 1, L - 2) if p < L - 1} and {0, L - 2} <= set(heavy)
            for t in (2, 3):                                                                    # the row maximum is tied ...
                ra = hub_ra(name, 0.5, hub, t)
                top = np.flatnonzero(ra[:-1] == ra[:-1].max()).tolist()
                assert top == (list(heavy) if heavy else list(range(L - 1))) and len(top) >= 2  # ... exactly at the named positions


def test_two_hubs_promise():
    for name in [m for m in X.NAMES if m.startswith("B_")]:
        L = int(name[3:])
        row, col, score, n = X.entries(name)
        rl, cl = lengths(name)
        assert rl[1] == L and rl[2] == L and cl[1] == L and cl[2] == L and rl[0] == 1 and rl[n - 1] == 2
        assert set(score[row != col].tolist()) == {1.0, 2.5, 10.0}
        at = np.flatnonzero(row == 1)
        assert col[at[:-1]].tolist() != sorted(col[at[:-1]].tolist())                           # permuted pair order
        lab = X.snapshots(name, 0.5)[10][0]
        assert len(set(lab.tolist())) >= 3
        for t in (2, 3):
            for hub in (1, 2):
                ra = hub_ra(name, 0.5, hub, t)[:-1]                                             # the leaves of a long row:
                assert (np.unique(ra, return_counts=True)[1] > 1).sum() >= 2                    # tied values (DEVIATIONS: they decide)


@pytest.mark.parametrize("L", X.LENGTHS)
def test_directed_lengths(L):
    rl, cl = lengths("C1_L%d" % L)
    assert cl[0] == L and rl[0] == 1 and set(rl[1:].tolist()) == {1, 2} and cl[1:].max() == 1
    rl, cl = lengths("C2_L%d" % L)
    assert rl[0] == L and cl[0] == 1 and set(cl[1:].tolist()) == {1, 2} and rl[1:].max() == 1


def test_hub_edges_golden_holds_the_edge_rows():
    """tests/golden/apc_hub_edges.orth (tools/refharness/make_apc_goldens.py; its expected outputs come from the real reference and
    are compared in tests/test_find_cluster_apc.py): after fc2mat's doubling and preference entries the two hubs' rows and columns hold
    LM + 1 and W + 1 entries, and the weights are tied"""
    import os
    from conftest import GOLD
    from swiftortho_amd import find_cluster as fc
    names, row, col, score, n = fc.apc_entries(open(os.path.join(GOLD, "apc_hub_edges.orth")))
    rl, cl = np.bincount(row, minlength=n), np.bincount(col, minlength=n)
    assert sorted(rl.tolist())[-3:] == [4, LM + 1, W + 1] and np.array_equal(rl, cl)
    assert sorted(set(score[row != col].tolist())) == [1.0, 2.5, 10.0] and score[row == col].tolist() == [-40.0] * n
    assert len(X.plan(row, col, n)[1]) == len(X.plan(row, col, n)[3]) == 2                 # both hubs go to the wave kernels


def test_odd_genes_ring_and_full_promises():
    row, col, score, n = X.entries("C3_odd_genes")
    rl, cl = lengths("C3_odd_genes")
    diag = set(row[row == col].tolist())
    assert rl[2] == W + 1 and 2 not in diag and rl[4] == LM + 1 and 4 in diag
    assert rl[3] == 0 and cl[3] == 0 and rl[6] == 0 and cl[6] == 2 and cl[0] == 0 and rl[0] == 2
    assert len([g for g in range(n) if rl[g] and g not in diag]) >= 10
    for m in (255, 256, 257):
        rl, cl = lengths("C4_ring%d" % m)
        assert len(rl) == m and set(rl.tolist()) == {2} and set(cl.tolist()) == {2}
    rl, cl = lengths("C5_full")
    assert rl.min() == cl.min() == rl.max() == LM + 2


def test_plan_restatement_sends_each_length_where_it_belongs():
    """the lane / wave split of so_apc (split_by_length), restated from LM"""
    for L in X.LENGTHS:
        rs, rlong, cs, clong = X.plan(*[X.entries("A_L%d_hub5_ties" % L)[j] for j in (0, 1, 3)])
        assert (rlong, clong) == (([5], [5]) if L > LM else ([], [])) and len(rs) == len(cs) == L - (L > LM)
        rs, rlong, cs, clong = X.plan(*[X.entries("C1_L%d" % L)[j] for j in (0, 1, 3)])
        assert rlong == [] and clong == ([0] if L > LM else []) and len(rs) == L                # column wave next to row lanes
        rs, rlong, cs, clong = X.plan(*[X.entries("C2_L%d" % L)[j] for j in (0, 1, 3)])
        assert clong == [] and rlong == ([0] if L > LM else []) and len(cs) == L
    rs, rlong, cs, clong = X.plan(*[X.entries("C5_full")[j] for j in (0, 1, 3)])
    assert rs == [] and cs == [] and len(rlong) == len(clong) == LM + 2                          # nrs == 0 and ncs == 0
    for m in (255, 256, 257):
        rs, rlong, cs, clong = X.plan(*[X.entries("C4_ring%d" % m)[j] for j in (0, 1, 3)])
        assert len(rs) == len(cs) == m and not rlong and not clong                               # one block, one full, one and a lane
    rs, rlong, cs, clong = X.plan(*[X.entries("C3_odd_genes")[j] for j in (0, 1, 3)])
    assert rlong == [2, 4] and 3 not in rs + cs + clong and 6 in cs and 6 not in rs and clong == [2, 4]
    row, col, _, n = X.entries("E_w_tiny_first")
    assert X.plan(row, col, n)[3] == [0] and X.plan(*[X.entries("E_lane_tiny_first")[j] for j in (0, 1, 3)])[3] == []


@pytest.mark.parametrize("L", [20, W + 6, 2 * W + 1])
def test_two_diag_shows_which_diagonal_entry_counts(L):
    row, col, score, n = X.entries("D_L%d" % L)
    at = np.flatnonzero(row == 1)
    dg = [j for j in range(len(at)) if col[at[j]] == 1]
    assert len(at) == L and dg == [5, L - 1] and score[at[5]] == -3.0 and score[at[-1]] == 0.75
    assert (5 // W != (L - 1) // W) == (L > W)                                                   # in different chunks
    srow, scol, sscore, _ = X.entries("D_L%d_swapped" % L)
    assert np.array_equal(row, srow) and np.array_equal(col, scol) and (score != sscore).sum() == 2
    for damp in (0.0, 0.5, 0.9):
        a, b = X.snapshots("D_L%d" % L, damp)[3], X.snapshots("D_L%d_swapped" % L, damp)[3]
        differing = int((a[2].view(np.uint32) != b[2].view(np.uint32)).sum())
        print("two_diag", L, damp, "A values differing under the swap after 3 rounds:", differing)
        assert differing >= L - 2


@pytest.mark.parametrize("name", sorted(X.e_cases()))
def test_ordered_column_shows_its_order(name):
    args, bits = X.e_cases()[name]
    row, col, score, n = X.entries(name)
    assert np.bincount(col, minlength=n)[0] == args[0] + 1 and (args[0] + 1 <= LM) == ("lane" in name)
    diag = int(np.flatnonzero((row == 0) & (col == 0))[0])
    assert diag == len(row) - 1
    for damp, want in zip((0.0, 0.5), bits):
        _, r, a = X.snapshots(name, damp)[1]
        assert same_bits(r, (score.astype(np.float64) * (1 - damp)).astype(np.float32))          # R = (1 - damp) * s exactly
        assert int(a[diag:].view(np.uint32)[0]) == want
    twin = name.replace("tiny", "one") if "tiny" in name else name.replace("one", "tiny")
    assert X.e_cases()[twin][1] != bits and sorted(X.entries(twin)[2].tolist()) == sorted(score.tolist())


def _f(name):
    return [m for m in X.NAMES if m.startswith("F") and m.endswith(name)]


def test_non_finite_inputs_promise():
    """the NaN-valued R + A of round 2 sits where the name says; overflow makes an inf no score held; blind rows keep their label"""
    for name in [m for m in X.NAMES if "_nan_at" in m or "_nan_lane0" in m]:
        row, _, score, _ = X.entries(name)
        at = np.flatnonzero(row == X.F_HUB)
        where = np.flatnonzero(np.isnan(hub_ra(name, 0.5, X.F_HUB, 2))).tolist()
        assert where == np.flatnonzero(np.isnan(score[at])).tolist()
        assert where == ([0, W] if "lane0" in name and len(at) > W else [0] if "lane0" in name else [int(name.rsplit("at", 1)[1])])
    assert {tuple(np.flatnonzero(np.isnan(hub_ra(m, 0.5, X.F_HUB, 2))).tolist()) for m in _f("_nan_at0") + _f("_nan_at10") + _f("_nan_at64")} \
        == {(0,), (10,), (W,)}
    for name in [m for m in X.NAMES if m.startswith("F")]:
        kind = name.split("_", 1)[1]
        row, col, score, n = X.entries(name)
        for damp in X.REGISTRY[name][2]:
            lab, r, a = X.snapshots(name, damp)[3]
            both = np.concatenate([r, a])
            if kind.startswith(("pinf", "ninf", "nan", "blind", "parsed")):
                assert np.isnan(both).sum() + np.isinf(both).sum() > 0
            if kind.startswith(("pinf", "ninf", "parsed")) and damp == 1.0:
                assert np.isnan(r).sum() > 0                                                     # beta = 0, and 0 * inf
            if kind == "parsed_1e39":
                assert np.isinf(score).sum() == 2
            if kind == "overflow":
                r2 = X.snapshots(name, damp)[2 if damp == 0.0 else 3][1]                         # -3e38 - 3e38, rounded on store
                assert np.isfinite(score).all() and np.isinf(r2).sum() > 0 and not np.isnan(r2).any()
            if kind == "tiny":
                sub = lambda v: int(((v != 0) & (np.abs(v) < np.finfo(np.float32).tiny)).sum())
                assert sub(score) == len(score) and sub(r) + sub(a) > len(r)               # more than half of all stores
            if kind == "signed_zeros":
                assert np.signbit(score[score == 0]).sum() > 10
            if kind == "blind_rows":
                leaf = X.star_leaves(n, X.F_HUB)[4]
                for t in (1, 2, 3, 10):
                    lab_t, r_t, a_t = X.snapshots(name, damp)[t]
                    for g in (X.F_HUB, leaf):
                        ra = r_t[row == g].astype(np.float64) + a_t[row == g]
                        assert np.all(np.isnan(ra) | (ra == -INF)) and lab_t[g] == g


def test_some_input_leaves_a_negative_zero():
    """the comparison's sign-of-zero half is not idle: the oracle's own stores hold -0.0 on these inputs"""
    hits = [(name, damp) for name, damp in X.RUNS if X.family(name) == "F" and name.endswith(("_tiny", "_signed_zeros"))
            for t in (1, 2, 3) for s in [X.snapshots(name, damp)[t]] if any(np.signbit(v[v == 0]).any() for v in s[1:])]
    print("inputs whose R or A holds -0.0 after round 1, 2 or 3:", hits)
    assert hits


# ---- the restatement equals the oracle; its deviations do not ---------------------------------------------------------------------------
@pytest.mark.parametrize("fam", "ABCDEF")
def test_restatement_equals_oracle(fam):
    for name, damp in X.RUNS:
        if X.family(name) != fam:
            continue
        want, got = X.snapshots(name, damp), restated(name, damp)
        for t in X.ROUNDS:
            if t in got:
                assert same_state(got[t], want[t]), (name, damp, t)


# deviation -> the (input, damping factor, first round that differs) that tell it from the oracle
DEVIATIONS = {
    "ge_updater": [("B_L33", 0.5, 2), ("B_L129", 0.5, 2), ("A_L127_hub0_heavy", 0.5, 2)],        # `>=` for `>` in the updater test
    "first_updater": [("B_L33", 0.5, 2), ("A_L33_hub5_heavy", 0.5, 2), ("C2_L64", 0.5, 2)],      # m1 / k1 from the first updater
    "first_label": [("B_L33", 0.5, 1), ("A_L33_hub0_ties", 0.5, 1), ("C2_L129", 0.5, 1)],        # the label from the first updater
    "lane0_before": [("B_L129", 0.5, 1), ("D_L129", 0.5, 2), ("F70_nan_at64", 1.0, 1)],          # lane 0 keeps what the shuffle left it
    "nan_kept": [("F70_nan_lane0_each_chunk", 0.5, 2), ("F70_nan_at0", 1.0, 1)],                 # a NaN R + A enters the scan
    "first_diag": [("D_L129", 0.5, 1), ("D_L70_swapped", 0.5, 1), ("D_L20", 0.5, 1)],            # diag5 from the first diagonal entry
    "diag_in_sum": [("D_L129", 0.5, 1), ("D_L20", 0.5, 1), ("F70_pinf_pref", 0.5, 1)],           # the diagonal counted in the column sum
    "rev_first_chunk": [("E_w_head_one_first", 0.0, 1), ("E_w_head_tiny_first", 0.5, 1)],        # a long column's first chunk backwards
    "reset_m1": [("A_L127_hub5_ties", 0.0, 3), ("B_L33", 0.5, 3)],                               # m1 back to 0 every round
    "reset_m2": [("A_L127_hub0_heavy", 0.5, 3), ("B_L129", 0.5, 3)],                             # m2 back to 0 every round
    "change_seeded": [("B_L33", 0.5, 1), ("A_L127_hub0_ties", 1.0, 1), ("C4_ring256", 0.5, 1)],  # get_change from the carried maximum
}

# first for last candidate for m2: the candidates reaching the maximum compare equal, so they differ in the sign of a zero at most, and
# k1_minus1: while k1 holds its start value m1 and m2 are both still +0.0 (see the test below) -- the two that no input can show
UNOBSERVABLE = ("last_candidate", "k1_minus1")


@pytest.mark.parametrize("dev", sorted(DEVIATIONS))
def test_named_inputs_tell_the_deviation_from_the_oracle(dev):
    for name, damp, t in DEVIATIONS[dev]:
        assert first_difference(name, damp, dev, t) == t, (dev, name, damp)


@pytest.mark.parametrize("dev", UNOBSERVABLE)
def test_the_two_deviations_no_input_can_show(dev):
    """`last_candidate` (m2 from the last instead of the first candidate reaching the maximum): the candidates compare equal, so they
    differ in the sign of a zero at most, and a zero never exceeds the carried m2 >= +0.0 -- m2 cannot take it.  `k1_minus1` (k1
    starting at no gene instead of gene 0): k1 leaves its start value in the very step in which m1 first leaves +0.0, and until then
    no R + A exceeded 0, so m2 is +0.0 as well -- whichever of m1 and m2 an entry in column 0 subtracts, it subtracts +0.0.  Both hold
    for the reference's loop as for the kernels, so neither is a property an input could pin; this test records that on the inputs
    that come closest (gene 0 as hub, as leaf and as bystander; zeros of both signs), and would show a change of that."""
    for name, damp in X.RUNS:
        if damp == 0.5 and (X.family(name) in "AB" or name.endswith(("signed_zeros", "tiny"))):
            assert first_difference(name, damp, dev) is None, (name, damp)
