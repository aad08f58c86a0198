"""The pan-genome device call (csrc/pan.hip so_pan_genome: k_pan_curve, k_pan_type) at every edge of its kernels, against the numpy
definitions (swiftortho_amd/pan.py count_matrix, row_types, rarefaction) array for array: dtype, shape, every entry, the totals and the
stats.  pan.device_pan_genome is called directly, so that the orders and the step thresholds can be anything (tests/pan_curve_inputs.py;
tests/test_pan_curve_inputs.py shows on the CPU that the right answer of every input differs from the plausible wrong ones).  Device
memory is poisoned in every test; every case runs in both tiers of k_pan_curve where the LDS tier can hold it:
  * orders per workgroup: every remainder of size modulo 4 (a wave without an order), one and several workgroups, no order at all;
  * designed orders: identity, reversed, the same order in all four waves, in two workgroups, the last taxon first; 2 and 3 taxa;
  * the row mask of the last tile, which decides as soon as C <= 0, with 1 .. 129 rows; S and C at their 32-bit clamps and at -1;
  * 818, 819 and 820 taxa: the largest LDS launch (65 472 bytes) and the switch to the global tier, from both sides;
  * 1, 255, 256, 257, 512 and 513 tiles: one, two and three tiles per range, with a full, a nearly full and a one-row last tile;
  * k_pan_type: the file rows ending before, at and behind a tile's edge, under thresholds that make everything Specific, nothing
    Specific, nothing Share;
  * one shape after another in one process: large, one row, the most LDS, one order;
  * the grid's height: the refusal above it and the largest size served.

Observed on an MI355X, numpy reference included: test_grid_height 0.8 s (the device serves 262 144 orders, 4 x its grid height of 65 536;
with a second tier at that size it took 2.6 s, and 5.1 s once inside a run of the whole suite, which is why only one tier runs there),
a test_tile_ranges case 0.03 .. 0.09 s, every other test at most 0.05 s; this module and tests/test_gpu_pan.py together 5.6 s.  No path
disagreed with numpy.  A library built without the row mask in the core count (`& mask` deleted) fails test_mask_and_extreme_thresholds at
1, 63, 65, 127 and 129 rows in both tiers and the golden u0 in both tiers, and passes every test the suite had before them.

Run on the GPU box:  python -m pytest tests/test_gpu_pan_curve.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import pan_curve_inputs as ci

pytestmark = pytest.mark.gpu

TIERS = ("lds", "global")
TIER_CODE = {"lds": 1, "global": 2}


@pytest.fixture(scope="module")
def pan():
    from swiftortho_amd import pan
    return pan


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("SOHIT_POISON", "165")
    monkeypatch.delenv("SOHIT_PAN_TIER", raising=False)


class Want:
    def __init__(self, counts, types, totals, curves):
        self.counts, self.types, self.totals, self.curves = counts, types, totals, curves


_WANT = {}


def numpy_answer(case):
    """the numpy definitions on a case: computed once, shared, left unchanged"""
    if case.name not in _WANT:
        from swiftortho_amd import pan
        counts = pan.count_matrix(case.row, case.taxon, case.n_rows, case.n_taxa)
        types, totals = pan.row_types(counts, case.n_file_rows, case.spec_max, case.core_min)
        _WANT[case.name] = Want(counts, types, totals, pan.rarefaction(counts, case.perm, case.S, case.C))
    return _WANT[case.name]


def expected_tier(case, tier):
    """the tier a call reports: none without a curve; the LDS tier unless it is switched off or cannot hold the taxa"""
    if case.size == 0 or case.n_taxa < 2:
        return 0
    return 1 if tier in (None, "lds") and case.fits_lds else 2


def serve(pan, monkeypatch, case, tier, want_counts=True):
    """one device call under `tier` (None: no switch), held to numpy -> the result"""
    if tier is None:
        monkeypatch.delenv("SOHIT_PAN_TIER", raising=False)
    else:
        monkeypatch.setenv("SOHIT_PAN_TIER", tier)
    got, want = pan.device_pan_genome(*case.args(), want_counts=want_counts), numpy_answer(case)
    assert got.types.dtype == np.uint8 and got.types.shape == (case.n_rows,) and got.types.tolist() == want.types.tolist(), case.name
    assert got.totals == want.totals and sum(got.totals) == case.n_file_rows, case.name
    for k, a, b in zip(("core", "spec", "panz"), (got.core, got.spec, got.panz), want.curves):
        assert a.dtype == np.int64 and a.shape == b.shape == (case.size, max(case.n_taxa - 1, 0)) and a.tolist() == b.tolist(), (case.name, k)
    if want_counts:
        assert got.counts.dtype == np.int32 and got.counts.shape == want.counts.shape and got.counts.tolist() == want.counts.tolist(), case.name
    else:
        assert got.counts is None
    assert got.stats == {"tier": expected_tier(case, tier), "waits": 1}, case.name
    return got


@pytest.mark.parametrize("tier", TIERS)
def test_orders_per_workgroup(pan, monkeypatch, tier):
    """a wave without an order, at every remainder of size modulo 4; and the first s orders' curves do not depend on how many follow"""
    got = {size: serve(pan, monkeypatch, ci.size_case(size), tier) for size in ci.SIZES}
    full = got[21]
    for size in ci.SIZES:
        for k in ("core", "spec", "panz"):
            assert getattr(got[size], k).tolist() == getattr(full, k)[:size].tolist(), (size, k)
    none = serve(pan, monkeypatch, ci.size_case(0), tier)         # no order: no curve, types and counts all the same
    assert none.core.shape == (0, ci.SIZE_TAXA - 1) and none.types.tolist() == full.types.tolist() and none.totals == full.totals
    assert none.counts.tolist() == full.counts.tolist()
    serve(pan, monkeypatch, ci.size_case(5), tier, want_counts=False)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("case", ci.order_cases(), ids=lambda c: c.name)
def test_designed_orders(pan, monkeypatch, case, tier):
    got = serve(pan, monkeypatch, case, tier)
    perm = case.perm.tolist()
    for p in range(case.size):                                    # equal orders, in one workgroup or in two: equal rows
        for q in range(p):
            if perm[p] == perm[q]:
                assert got.core[p].tolist() == got.core[q].tolist() and got.spec[p].tolist() == got.spec[q].tolist() and got.panz[p].tolist() == got.panz[q].tolist()


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("n_rows", ci.MASK_ROWS)
def test_mask_and_extreme_thresholds(pan, monkeypatch, n_rows, tier):
    """C <= 0: every row is core and no lane behind the last row is; C, S at the clamps; S = -1"""
    for name, (_, _, what) in sorted(ci.EXTREMES.items()):
        case = ci.mask_case(n_rows, name)
        got = serve(pan, monkeypatch, case, tier)
        if what == "core_all":
            assert (got.core == n_rows).all(), name
        elif what == "core_none":
            assert not got.core.any(), name
        elif what == "spec_none":
            assert not got.spec.any(), name
        else:
            x = got.counts > 0
            assert got.spec.tolist() == [[int(x[:, t].sum()) for t in order[1:]] for order in case.perm.tolist()], name


@pytest.mark.parametrize("tier", (None,) + TIERS)
@pytest.mark.parametrize("n_taxa", ci.LDS_TAXA)
def test_lds_bound(pan, monkeypatch, n_taxa, tier):
    """818 and 819 taxa take the LDS tier (819: 65 472 bytes of LDS, the most the kernel asks for), 820 the global one; forced to the
    global tier, all three"""
    got = serve(pan, monkeypatch, ci.lds_case(n_taxa), tier)
    assert got.stats["tier"] == (2 if tier == "global" or n_taxa > ci.LDS_MAX_TAXA else 1)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("W", ci.TILE_W)
def test_tile_ranges(pan, monkeypatch, W, tier):
    for n_rows in ci.tile_rows(W):
        serve(pan, monkeypatch, ci.tile_case(n_rows), tier)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("n_file_rows", ci.TYPE_FILE_ROWS)
def test_types(pan, monkeypatch, n_file_rows, tier):
    for th in ci.TYPE_THRESHOLDS:
        got = serve(pan, monkeypatch, ci.type_case(n_file_rows, th), tier)
        assert not got.types[n_file_rows:].any()
        if th == (5, 6):
            assert got.totals == (0, 0, n_file_rows) and not got.types.any()


@pytest.mark.parametrize("poison_byte", ["165", "90"])
def test_shape_after_shape(pan, monkeypatch, poison_byte):
    """a large call, then a one-row one, then the most LDS, then one order: none sees what the one before left"""
    monkeypatch.setenv("SOHIT_POISON", poison_byte)
    cases = ci.sequence_cases()
    assert [(c.n_rows, c.n_taxa, c.size) for c in cases] == [(32832, 5, 5), (1, 2, 5), (130, 819, 5), (130, 6, 1)]
    for tier in (None, "global"):
        for case in cases:
            serve(pan, monkeypatch, case, tier)


def test_grid_height(pan, monkeypatch):
    """a workgroup per 4 orders along the grid's height: a size above what the device's grid takes is refused before a launch, with the
    largest size served in the message; that size is served and equals numpy (most of the test's time: a quarter of a million orders
    are compared entry by entry), and 4 x 4096 + 1 orders in both tiers"""
    limit = ci.served_size_limit(pan.device_pan_genome)
    for size in (limit + 1, limit + ci.WAVES):
        with pytest.raises(RuntimeError) as e:
            pan.device_pan_genome(*ci.grid_case(size).args())
        assert "%d orders are more than one call serves" % size in str(e.value) and "largest size served is %d)" % limit in str(e.value)
    serve(pan, monkeypatch, ci.grid_case(limit), None)
    for tier in TIERS:                                               # a last group of one order, 4096 groups up
        serve(pan, monkeypatch, ci.grid_case(ci.GRID_ORDERS), tier)
