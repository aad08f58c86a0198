"""The Markov-cluster kernels (swiftortho_amd/csrc/mcl.hip, so_mcl) at their table and scratch boundaries, against the scipy oracle
in its "exact" power mode (tests/mcl_scipy_oracle.py): the device inflates with the double-precision pow rounded once, and an oracle
that does the same is compared BIT FOR BIT -- indptr, indices and data `array_equal` -- so one misordered sum or one swapped pair of
columns shows.  The CPU tests check that the fixtures hold what the GPU tests rely on: the products per row sit exactly on the tier
boundaries of the expansion kernel (128 / 1024 / 2048, and one beyond each), the rows of x_old at the convergence checks are longer
than the 1024 entries the LDS tables of k_mcl_diff take, and no inflated value of a run that is compared bit for bit lies near a
float32 rounding boundary (`midpoint_hits == 0`), where the host's and the device's double pow could disagree in the last bit."""
import functools

import numpy as np
import pytest

from mcl_scipy_oracle import scipy_mcl

KS = [127, 128, 129, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 2500]   # around MCL_SMALL_P, MCL_LDS_P, MCL_BIG_P of mcl.hip
POOL = 2600
LDS_P = 1024      # MCL_LDS_P: rows above it get global scratch from Mcl::plan()
# chosen on the CPU so that no bit-for-bit case has a value near a rounding boundary (test_no_bit_exact_case_is_near_a_rounding_boundary;
# at inflation 2.0 a float32 of at most 12 significant bits squares to an exact tie, about one value in 10^4: most seeds have one)
SEEDS = {"plain": 119, "small": 146, "self": 151, "peak1024": 1, "peak1025": 1, "peak1026": 1}
SMALL_PER_ROW = 3
PEAK_SCALE = 4.0  # "peak<k>": the weights of the probe row of k entries times this, which puts the maximum of the convergence test there
MAX_ROW_CASE = ("plain", 1.5, 1, 0)
# SOHIT_MCL_SCRATCH budgets (u32 words), worked out in test_plan_restatement_splits_the_long_rows
SPLIT_BUDGET = 20500            # >= the longest row's 18884 words: {1025, 1026}, {2047, 2048}, {2049}, {2500} products
ROW_TOO_BIG_BUDGET = 18883      # one word less than the 2500-product row needs
CONV_TOO_BIG_BUDGET = 50000     # every x_old row fits (3 * 8192 words at the most), all of them together (98304) do not


@functools.lru_cache(maxsize=None)
def probe_matrix(variant, seed=None):
    """A directed CSR block of len(KS) probe rows scattered among POOL pool rows, columns in shuffled storage order, weights uniform in
    [0.5, 2).  A pool row holds only its self loop (in "self" a heavy one, 5 to 20: with light ones the pool's diagonal is within a few
    float32 steps of 1 by the third round, and 1 - k * 2^-24 to the power 1.5 lies on a rounding boundary for every odd k).
    "plain": probe row p holds KS[p] entries into the pool: exactly KS[p] products in round 0 and KS[p] stored entries afterwards.
    "small": the same, but SMALL_PER_ROW weights of every probe row are 1e-3: their normalised, inflated value falls below the pruning
             threshold in round 0, so round 1 expands a matrix with stored zeros, which take a first-touch ordinal and are then dropped.
    "peak<k>": "plain" with the weights of the probe row of k entries times PEAK_SCALE: that row changes most from round to round.
    "self":  every probe row also holds its self loop, which multiplies the row with itself: every column of the row is touched twice
             (two products summed in order) and the row has 2 * length - 1 products; one pool row (the "hub") holds a second entry, and
             the probe rows with an even target hold the hub: KS[p] products again, recomputed and asserted by the tests.
    -> (indptr int64, indices int32, data float32, probe row numbers)"""
    rng = np.random.default_rng(SEEDS[variant] if seed is None else seed)
    n = len(KS) + POOL
    probes = np.sort(rng.choice(n, len(KS), replace=False))
    pool = np.setdiff1d(np.arange(n), probes)
    hub, hub_to = (int(pool[7]), int(pool[1900])) if variant == "self" else (-1, -1)
    rows = [None] * n
    for j in pool.tolist():
        rows[j] = [(j, rng.uniform(5, 20) if variant == "self" else rng.uniform(0.5, 2))]
    if variant == "self":
        rows[hub] = [(hub_to, rng.uniform(0.5, 2))] + rows[hub]
    for p, k in zip(probes.tolist(), KS):
        if variant == "self":
            length = (k + 1) // 2 if k % 2 else k // 2
            others = rng.permutation(pool[pool != hub])[:length - 1 - (k % 2 == 0)].tolist()
            cols = [p] + ([hub] if k % 2 == 0 else []) + others
        else:
            cols = rng.permutation(pool)[:k].tolist()
        cols = [cols[o] for o in rng.permutation(len(cols)).tolist()]
        w = rng.uniform(0.5, 2, len(cols))
        if variant == "small":
            w[rng.choice(len(cols), SMALL_PER_ROW, replace=False)] = 1e-3
        if variant == "peak%d" % k:
            w *= PEAK_SCALE
        rows[p] = list(zip(cols, w.tolist()))
    indptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    indices = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    data = np.array([v for r in rows for _, v in r], dtype=np.float32)
    for a in (indptr, indices, data, probes):
        a.setflags(write=False)
    return indptr, indices, data, probes


def products(indptr, indices):
    """what k_mcl_products computes: per row, the summed lengths of the rows its entries name"""
    length = np.diff(indptr)
    row_of = np.repeat(np.arange(len(length)), length)
    return np.bincount(row_of, weights=length[indices], minlength=len(length)).astype(np.int64)


def plan(need, extra, budget):
    """Mcl::plan() of mcl.hip: ranges of rows whose scratch fits `budget` u32 words; a row above LDS_P units takes 2 T + (units, for the
    expansion: `extra`, or T, for the convergence test) words, T = the power of two >= 2 * units.  -> (ranges, words per row)"""
    words = []
    for k in need:
        w = 0
        if k > LDS_P:
            t = 1
            while t < 2 * k:
                t <<= 1
            w = 2 * t + (int(k) if extra else t)
        words.append(w)
    ranges, lo, used = [], 0, 0
    for i, w in enumerate(words):
        if w > budget:
            raise ValueError("one row needs more")
        if used + w > budget:
            ranges.append((lo, i))
            lo, used = i, 0
        used += w
    ranges.append((lo, len(words)))
    return ranges, np.array(words, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def exact(variant, inflation, rounds, check=5, atol=1e-8):
    """the exact-mode oracle on a probe matrix, once per case: (indptr, indices, data, info), never modified"""
    ip, ix, dv, _ = probe_matrix(variant)
    info = {}
    out = scipy_mcl(ip.copy(), ix.copy(), dv.copy(), inflation, rounds=rounds, check=check, atol=atol, power="exact", info=info)
    for a in out:
        a.setflags(write=False)
    return out + (info,)


def same_matrix(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


VARIANTS = ["plain", "small", "self"]
TIER_CASES = [(v, i, r) for v in VARIANTS for i in (1.5, 2.0) for r in (1, 2, 3)]
# convergence cases: (variant, inflation, check interval, index of the check among the run's checks)
PEAKS = [1024, 1025, 1026]   # the last row on k_mcl_diff's LDS tables, the first in global scratch (offset 0), the first at an offset
CONV_CASES = [("plain", 1.5, 1, 0), ("self", 1.5, 1, 0), ("plain", 1.2, 5, 0), ("small", 1.2, 5, 0)] + [("peak%d" % k, 1.5, 1, 0) for k in PEAKS]


def conv_rounds(check, which):
    """two rounds beyond the one in which that check stops the loop"""
    return check * (which + 1) + 3


# ---- the fixtures hold what they promise (CPU) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_probe_rows_sit_on_the_tier_boundaries(variant):
    ip, ix, dv, probes = probe_matrix(variant)
    assert len(ip) - 1 == len(KS) + POOL
    got = products(ip, ix)
    assert got[probes].tolist() == KS                       # 127 / 128 | 129 ... 1024 | 1025 ... 2048 | 2049, 2500: every tier, both sides
    assert got[np.setdiff1d(np.arange(len(got)), probes)].max() <= 3      # (the hub of "self": its own two entries and its neighbour's one)
    for r in range(ip.shape[0] - 1):                        # columns of a row are distinct (the kernel's lanes own one slot each)
        if ip[r + 1] - ip[r] > 1:
            c = ix[ip[r]:ip[r + 1]]
            assert len(np.unique(c)) == len(c)
            assert np.any(np.diff(c) < 0)                   # ... and not in ascending order
    if variant == "self":
        length = np.diff(ip)[probes]
        assert length.tolist() == [(k + 1) // 2 if k % 2 else k // 2 for k in KS]
        assert all(p in ix[ip[p]:ip[p + 1]] for p in probes.tolist())
    # the rounds after the first (the matrix a run of r rounds ends on is what round r expands): every tier and the scratch stay in use
    for inflation in (1.5, 2.0):
        for r in (1, 2):
            a = exact(variant, inflation, r)
            later = products(a[0], a[1])[probes]
            assert (later <= 128).any() and ((later > 128) & (later <= LDS_P)).any() and ((later > LDS_P) & (later <= 2048)).any() and (later > 2048).any()
            if variant == "plain" and inflation == 1.5:
                assert later.tolist() == KS                 # nothing pruned yet: the same boundaries again
            if variant == "self":
                assert {127, 129, 1023, 1025, 2047, 2049} <= set(later.tolist())


def test_small_variant_stores_zeros_after_the_first_round():
    ip, ix, dv, probes = probe_matrix("small")
    assert int((dv == np.float32(1e-3)).sum()) == SMALL_PER_ROW * len(KS)
    for inflation in (1.5, 2.0):
        a = exact("small", inflation, 1)
        assert np.array_equal(a[0], ip)                                     # every entry still stored ...
        zeros = int((a[2] == 0).sum())                                      # ... the small ones as zeros (at inflation 2.0 others too)
        assert zeros == SMALL_PER_ROW * len(KS) if inflation == 1.5 else zeros > SMALL_PER_ROW * len(KS)
        b = exact("small", inflation, 2)
        dropped = np.array(KS) - np.diff(b[0])[probes]                      # round 1 touched them and dropped them
        assert np.all(dropped == SMALL_PER_ROW) if inflation == 1.5 else np.all(dropped >= SMALL_PER_ROW)
    assert int((exact("plain", 1.5, 1)[2] == 0).sum()) == 0


@pytest.mark.parametrize("variant,inflation,check,which", CONV_CASES)
def test_convergence_cases_have_long_old_rows(variant, inflation, check, which):
    info = exact(variant, inflation, conv_rounds(check, which), check)[3]
    c = info["checks"][which]
    assert c["round"] == check * (which + 1)
    assert c["longest_old_row"] > LDS_P, c                  # the global-scratch half of k_mcl_diff
    assert c["max"] > 1e-8                                  # with the default atol the loop goes on
    if check == 1:
        ip, ix, dv, probes = probe_matrix(variant)
        old = np.diff(exact(variant, inflation, 1)[0])[probes]              # x_old of the check in round 1 = the matrix after round 0
        for k in (1023, 1024, 1025):
            assert k in old.tolist() or variant == "self"
        assert old.max() == c["longest_old_row"]


def test_the_maximum_of_one_check_sits_in_a_long_probe_row():
    variant, inflation, check, which = MAX_ROW_CASE
    ip, ix, dv, probes = probe_matrix(variant)
    c = exact(variant, inflation, conv_rounds(check, which), check)[3]["checks"][which]
    assert c["row"] in probes.tolist()
    old_rows = np.diff(exact(variant, inflation, c["round"])[0])            # structure of x_old = the matrix after `round` rounds
    assert old_rows[c["row"]] > LDS_P


@pytest.mark.parametrize("k", PEAKS)
def test_the_maximum_sits_in_the_row_at_the_edge_of_the_lds_table(k):
    """the compared maximum of the "peak<k>" case comes from the probe row with exactly k old entries: the value k_mcl_diff computes for
    THAT row (1024: the fullest LDS table; 1025: global scratch at offset 0; 1026: global scratch behind another row's) decides"""
    variant = "peak%d" % k
    ip, ix, dv, probes = probe_matrix(variant)
    c = exact(variant, 1.5, conv_rounds(1, 0), 1)[3]["checks"][0]
    assert c["row"] == probes[KS.index(k)]
    old_rows = np.diff(exact(variant, 1.5, 1)[0])
    assert old_rows[c["row"]] == k
    words = plan(old_rows, 0, 1 << 28)[1]
    before = int(words[:c["row"]].sum())                     # the row's scratch offset
    assert (words[c["row"]], before) == {1024: (0, 0), 1025: (12288, 0), 1026: (12288, 12288)}[k]
    assert c["max"] > 0.8 and c["max"] < 0.95                # (not the saturated 1 - rtol of a vanished entry)


def test_no_bit_exact_case_is_near_a_rounding_boundary():
    """every run the GPU tests compare bit for bit: no inflated value within 2^-44 (relative) of the midpoint of two float32 values"""
    for variant, inflation, rounds in TIER_CASES:
        assert exact(variant, inflation, rounds)[3]["midpoint_hits"] == 0, (variant, inflation, rounds)
    for variant, inflation, check, which in CONV_CASES:
        info = exact(variant, inflation, conv_rounds(check, which), check)[3]
        assert info["midpoint_hits"] == 0, (variant, inflation, check)
        for atol in conv_atols(variant, inflation, check, which):
            assert exact(variant, inflation, conv_rounds(check, which), check, atol)[3]["midpoint_hits"] == 0
    for name, (ip, ix, dv, inflation, kw) in degenerate_cases().items():
        if name != "negative_weight":
            info = {}
            scipy_mcl(ip.copy(), ix.copy(), dv.copy(), inflation, power="exact", info=info, **oracle_kw(kw))
            assert info["midpoint_hits"] == 0, name


def test_exact_power_is_the_correctly_rounded_one_and_numpy_mode_is_untouched():
    rng = np.random.default_rng(5)
    n = 40
    a = (rng.random((n, n)) < 0.3) * rng.uniform(0.1, 3, (n, n))
    a = np.maximum(a, a.T) + np.diag(rng.uniform(1, 3, n))
    from scipy import sparse
    m = sparse.csr_matrix(a.astype(np.float32))
    ip, ix, dv = m.indptr.astype(np.int64), m.indices.astype(np.int32), m.data.astype(np.float32)
    i1, i2 = {}, {}
    d = scipy_mcl(ip, ix, dv.copy(), 1.5, rounds=1)
    e = scipy_mcl(ip, ix, dv.copy(), 1.5, rounds=1, power="exact", info=i1)
    assert np.array_equal(d[0], e[0]) and np.array_equal(d[1], e[1])
    assert np.allclose(d[2], e[2], rtol=2.5e-7, atol=0)                      # one float32 ulp at the most
    assert i1 == {"rounds": 1, "converged": 0, "checks": [], "midpoint_hits": i1["midpoint_hits"]}
    # one round by hand: normalise, square densely in float64 (sums of at most 40 products: compare loosely), exact power
    x = a.astype(np.float32)
    x = (x / (x.sum(0, dtype=np.float32) + np.float32(1e-8))).astype(np.float32)
    want = (x.astype(np.float64) @ x.astype(np.float64)) ** 1.5
    got = sparse.csr_matrix((e[2], e[1], e[0]), shape=(n, n)).toarray()
    assert np.allclose(got, want, rtol=1e-5, atol=0)
    scipy_mcl(ip, ix, dv.copy(), 1.5, info=i2)
    assert i2["converged"] == 1 and i2["rounds"] == i2["checks"][-1]["round"] + 1 and i2["rounds"] % 5 == 1 and "midpoint_hits" not in i2
    assert all(c["max"].dtype == np.float32 for c in i2["checks"])
    with pytest.raises(ValueError):
        scipy_mcl(ip, ix, dv, 1.5, power="libm")


def conv_atols(variant, inflation, check, which):
    """the maximum the oracle compared at that check, and the next float32 towards zero"""
    m = exact(variant, inflation, conv_rounds(check, which), check)[3]["checks"][which]["max"]
    assert m.dtype == np.float32 and m > 0
    return float(m), float(np.nextafter(m, np.float32(0)))


def degenerate_cases():
    """name -> (indptr, indices, data, inflation, arguments of device_mcl)"""
    rng = np.random.default_rng(11)
    n = 12
    a = np.zeros((n, n), dtype=np.float32)
    for i in range(n):
        for j in range(i, n):
            if i == j or rng.random() < 0.45:
                a[i, j] = a[j, i] = np.float32(rng.uniform(0.5, 3.0))
    from scipy import sparse

    def csr(m):
        m = sparse.csr_matrix(m)
        return m.indptr.astype(np.int64), m.indices.astype(np.int32), m.data.astype(np.float32)
    ip, ix, dv = csr(a)
    holes = a.copy()
    holes[[1, 2, 6, 11], :] = 0                 # empty rows between full ones (their columns stay)
    out = {"one_gene_self_loop": (np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), np.array([2.5], dtype=np.float32), 1.5, {}),
           "one_gene_no_entry": (np.array([0, 0], dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32), 1.5, {}),
           "five_genes_no_entry": (np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32), 1.5, {}),
           "all_weights_zero": (ip, ix, np.zeros_like(dv), 1.5, {}),
           "empty_rows": csr(holes) + (1.5, {}),
           "zero_rounds": (ip, ix, dv, 1.5, {"rounds": 0}),
           "check_0": (ip, ix, dv, 1.5, {"check": 0}),
           "check_minus_3": (ip, ix, dv, 2.0, {"check": -3}),
           "no_gene": (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32), 1.5, {}),
           "no_gene_3_rounds": (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32), 1.5, {"rounds": 3})}
    assert np.diff(out["empty_rows"][0]).tolist().count(0) == 4 and np.diff(out["empty_rows"][0])[0] > 0
    return out


def oracle_kw(kw):
    """so_mcl clamps a check interval below 1 to 1; the oracle (`i % check`) has to be told"""
    kw = dict(kw)
    if kw.get("check", 5) < 1:
        kw["check"] = 1
    return kw


def negative_weight_block():
    ip, ix, dv, _, _ = degenerate_cases()["zero_rounds"]
    dv = dv.copy()
    e = int(np.flatnonzero(ix[ip[4]:ip[5]] != 4)[0] + ip[4])    # an off-diagonal entry of row 4
    dv[e] = -dv[e]
    return ip, ix, dv


def test_degenerate_cases_through_the_oracle():
    """what the oracle itself says about the degenerate inputs, by hand"""
    for name, (ip, ix, dv, inflation, kw) in degenerate_cases().items():
        info = {}
        out = scipy_mcl(ip.copy(), ix.copy(), dv.copy(), inflation, power="exact", info=info, **oracle_kw(kw))
        if name in ("one_gene_self_loop", "one_gene_no_entry", "five_genes_no_entry", "all_weights_zero", "no_gene"):
            assert (info["rounds"], info["converged"]) == (6, 1), name       # nothing moves: the first check, in round 5, succeeds
        if name in ("one_gene_no_entry", "five_genes_no_entry", "all_weights_zero", "no_gene"):
            assert len(out[1]) == 0 and out[0].tolist() == [0] * len(ip), name
        if name == "zero_rounds":
            assert same_matrix(out, (ip, ix, dv)) and info == {"rounds": 0, "converged": 0, "checks": [], "midpoint_hits": 0}
        if name == "no_gene_3_rounds":
            assert (info["rounds"], info["converged"]) == (3, 0)
        if name.startswith("check_"):
            assert info["converged"] == 1 and [c["round"] for c in info["checks"]] == list(range(1, info["rounds"]))
    ip, ix, dv = negative_weight_block()
    assert int((dv < 0).sum()) == 1
    with np.errstate(all="ignore"):
        for rounds in (1, 2, 6):
            info = {}
            out = scipy_mcl(ip.copy(), ix.copy(), dv.copy(), 1.5, rounds=rounds, power="exact", info=info)
            assert np.isnan(out[2]).sum() > 0 and info["converged"] == 0 and info["rounds"] == rounds
            if rounds == 6:
                assert len(info["checks"]) == 1 and np.isnan(info["checks"][0]["max"])


def test_plan_restatement_splits_the_long_rows():
    """the budgets the scratch tests use, worked out as Mcl::plan() does"""
    ip, ix, dv, probes = probe_matrix("plain")
    ranges, words = plan(products(ip, ix), 1, SPLIT_BUDGET)
    assert words[probes].tolist() == [0] * 5 + [9217, 9218, 10239, 10240, 18433, 18884]
    with_long_rows = [r for r in ranges if words[r[0]:r[1]].any()]
    assert len(with_long_rows) >= 3
    assert np.count_nonzero(words[ranges[0][0]:ranges[0][1]]) >= 2                # rows of one range must not share scratch ...
    assert any(np.count_nonzero(words[a:b]) >= 2 for a, b in ranges[1:])           # ... nor in a later range, where the offsets restart
    with pytest.raises(ValueError):
        plan(products(ip, ix), 1, ROW_TOO_BIG_BUDGET)
    # the convergence test of round 1 (check = 1) needs every long row of x_old in ONE range
    old = np.diff(exact("plain", 1.5, 1)[0])
    assert len(plan(products(ip, ix), 1, CONV_TOO_BIG_BUDGET)[0]) >= 2             # the expansion still fits, in ranges
    assert len(plan(old, 0, CONV_TOO_BIG_BUDGET)[0]) >= 2                          # ... the convergence scratch does not
    assert len(plan(old, 0, 1 << 28)[0]) == 1


# ---- the device against the oracle (GPU) ----------------------------------------------------------------------------------------
def device(variant, inflation, rounds, **kw):
    from swiftortho_amd import find_cluster as fc
    ip, ix, dv, _ = probe_matrix(variant)
    info = {}
    return fc.device_mcl(ip, ix, dv, inflation, rounds=rounds, info=info, **kw) + (info,)


def check_tier_case(variant, inflation, rounds):
    got, want = device(variant, inflation, rounds), exact(variant, inflation, rounds)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    bad = np.flatnonzero(got[2] != want[2])
    assert len(bad) == 0, "%d of %d values differ, first at %d: %r != %r" % (len(bad), len(want[2]), bad[0], got[2][bad[0]], want[2][bad[0]])
    assert got[3] == {"rounds": rounds, "converged": 0}


@pytest.mark.gpu
@pytest.mark.parametrize("variant,inflation,rounds", TIER_CASES)
def test_tier_boundaries_bit_for_bit(variant, inflation, rounds):
    """rows of exactly 127 ... 2500 products: the three LDS tables of k_mcl_spgemm and its global scratch, each at its last and first
    row; structure AND values equal to the exact-mode oracle's"""
    check_tier_case(variant, inflation, rounds)


def check_convergence_case(variant, inflation, check, which):
    at, below = conv_atols(variant, inflation, check, which)
    stop = check * (which + 1) + 1                        # rounds begun when the check of loop index check * (which + 1) succeeds
    want = exact(variant, inflation, conv_rounds(check, which), check, at)
    assert (want[3]["rounds"], want[3]["converged"]) == (stop, 1)
    got = device(variant, inflation, conv_rounds(check, which), check=check, atol=at)
    assert (got[3]["rounds"], got[3]["converged"]) == (stop, 1)
    assert same_matrix(got, want)
    want = exact(variant, inflation, conv_rounds(check, which), check, below)
    got = device(variant, inflation, conv_rounds(check, which), check=check, atol=below)
    assert (got[3]["rounds"], got[3]["converged"]) != (stop, 1) and got[3]["rounds"] > stop
    assert got[3] == {"rounds": want[3]["rounds"], "converged": want[3]["converged"]}
    assert same_matrix(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,inflation,check,which", CONV_CASES)
def test_convergence_decision_exactly(variant, inflation, check, which):
    """the maximum k_mcl_diff hands to the host is the oracle's float32 maximum, to the bit: with atol = that maximum the loop stops at
    that check, with the next float32 below it the loop goes on.  The x_old rows of these checks are 1023 / 1024 / 1025 ... 2500 entries
    long.  The result is ONE maximum, so which row holds it is what a case checks: the 2500-entry row in "plain" at check interval 1
    (global scratch, [T keys][T vals][T seen]), a pool row in "self", and in "peak1024" / "peak1025" / "peak1026" the row of exactly
    that many old entries: the fullest LDS table, the first row in global scratch, and a scratch row at an offset (the CPU tests assert
    where the oracle finds the maximum)."""
    check_convergence_case(variant, inflation, check, which)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "self"])
def test_scratch_ranges(variant, monkeypatch):
    """SOHIT_MCL_SCRATCH = a budget that splits the long rows over several ranges of rows (offsets restart per range, the tier lists and
    both passes run per range): same result, bit for bit"""
    free = device(variant, 1.5, 3)
    monkeypatch.setenv("SOHIT_MCL_SCRATCH", str(SPLIT_BUDGET))
    split = device(variant, 1.5, 3)
    assert same_matrix(split, free)
    assert same_matrix(split, exact(variant, 1.5, 3))


@pytest.mark.gpu
def test_scratch_budget_refusals(monkeypatch):
    """below one row's need, and below the convergence test's, so_mcl refuses with the message of that case; the process lives and the
    next call is served"""
    monkeypatch.setenv("SOHIT_MCL_SCRATCH", str(ROW_TOO_BIG_BUDGET))
    with pytest.raises(RuntimeError, match="one matrix row needs more scratch"):
        device("plain", 1.5, 3)
    monkeypatch.setenv("SOHIT_MCL_SCRATCH", str(CONV_TOO_BIG_BUDGET))
    assert same_matrix(device("plain", 1.5, 1, check=1), exact("plain", 1.5, 1, 1))     # one round: no convergence test yet
    with pytest.raises(RuntimeError, match="convergence scratch exceeds"):
        device("plain", 1.5, 2, check=1)
    monkeypatch.delenv("SOHIT_MCL_SCRATCH")
    assert same_matrix(device("plain", 1.5, 2, check=1), exact("plain", 1.5, 2, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("poison", ["0xFF", "0x5A"])
def test_stale_device_memory_mcl(poison, monkeypatch):
    """every fresh device allocation of so_mcl pre-filled (so_mcl reads SOHIT_POISON per call): 0xFF makes a table that is not cleared
    look empty (MCL_EMPTY), 0x5A makes it look full"""
    monkeypatch.setenv("SOHIT_POISON", poison)
    for variant in VARIANTS:
        check_tier_case(variant, 1.5, 3)
    check_convergence_case("plain", 1.5, 1, 0)
    check_convergence_case("plain", 1.2, 5, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("poison", ["0xFF", "0x5A"])
def test_stale_device_memory_apc(poison, monkeypatch):
    """the same for so_apc: the "hubs" graph of tests/test_find_cluster_apc.py, 3 rounds, against its oracle value for value"""
    from apc_numpy_oracle import numpy_apc
    from swiftortho_amd import find_cluster as fc
    from apc_graphs import _entries
    _, row, col, score, n = _entries("hubs")
    want = numpy_apc(row, col, score, n, 0.5, rounds=3)
    monkeypatch.setenv("SOHIT_POISON", poison)
    lab, r, a = fc.device_apc(row, col, score, n, 0.5, rounds=3)
    assert np.array_equal(lab, want[0]) and np.array_equal(r, want[1]) and np.array_equal(a, want[2])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(degenerate_cases()))
def test_degenerate_inputs(name):
    from swiftortho_amd import find_cluster as fc
    ip, ix, dv, inflation, kw = degenerate_cases()[name]
    winfo, ginfo = {}, {}
    want = scipy_mcl(ip.copy(), ix.copy(), dv.copy(), inflation, power="exact", info=winfo, **oracle_kw(kw))
    got = fc.device_mcl(ip, ix, dv, inflation, info=ginfo, **kw)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float32
    assert same_matrix(got, want)
    assert ginfo == {"rounds": winfo["rounds"], "converged": winfo["converged"]}


@pytest.mark.gpu
@pytest.mark.parametrize("rounds", [1, 2, 6])
def test_negative_weight(rounds):
    """one negative weight: a column sum below zero takes normalize()'s other addend (flags[2] of k_mcl_colsum), the power of a negative
    value is NaN, and the NaN goes through k_mcl_diff to the host, where `NaN <= atol` is false as in the reference"""
    from swiftortho_amd import find_cluster as fc
    ip, ix, dv = negative_weight_block()
    winfo, ginfo = {}, {}
    with np.errstate(all="ignore"):
        want = scipy_mcl(ip.copy(), ix.copy(), dv.copy(), 1.5, rounds=rounds, power="exact", info=winfo)
    got = fc.device_mcl(ip, ix, dv, 1.5, rounds=rounds, info=ginfo)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.allclose(got[2], want[2], rtol=1e-6, atol=1e-12, equal_nan=True)
    assert np.isnan(got[2]).sum() == np.isnan(want[2]).sum() > 0
    assert ginfo == {"rounds": rounds, "converged": 0} and winfo["converged"] == 0
