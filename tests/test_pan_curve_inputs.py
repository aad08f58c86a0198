"""CPU-only: the designed inputs of tests/test_gpu_pan_curve.py (tests/pan_curve_inputs.py) hold what they claim, so that no device test
can pass on an input whose right answer coincides with a plausible wrong one; and the two statements of the definition -- the numpy
functions of swiftortho_amd/pan.py and the plain loops of pan_curve_inputs -- agree on every one of them, and with what the REAL
scripts/pan_genome.py wrote for the goldens u0 and l_huge."""
import os
import re

import numpy as np
import pytest

import pan_curve_inputs as ci
import pan_inputs as pi
from conftest import ROOT
from test_pan import library_result


@pytest.fixture(scope="module")
def pan():
    from swiftortho_amd import pan
    return pan


def numpy_answer(pan, case):
    counts = pan.count_matrix(case.row, case.taxon, case.n_rows, case.n_taxa)
    types, totals = pan.row_types(counts, case.n_file_rows, case.spec_max, case.core_min)
    return counts, types, totals, pan.rarefaction(counts, case.perm, case.S, case.C)


def curve_rows(curves):
    """-> per order the tuple of its three curves"""
    core, spec, panz = (np.asarray(c).tolist() for c in curves)
    return [(tuple(core[p]), tuple(spec[p]), tuple(panz[p])) for p in range(len(core))]


def test_constants_mirror_the_sources():
    tune = open(os.path.join(ROOT, "swiftortho_amd", "csrc", "tune.h")).read()
    for k in ("PAN_LDS_BYTES", "PAN_TILE_RANGES"):
        assert int(re.search(r"#define %s (\d+)u?\b" % k, tune).group(1)) == getattr(ci, k), k
    src = open(os.path.join(ROOT, "swiftortho_amd", "csrc", "pan.hip")).read()
    expr = re.search(r"size_t pan_lds_bytes\(u64 T\) \{ return \(size_t\)\((.*?)\); \}", src).group(1)
    py = re.sub(r"\b(\d+)u\b", r"\1", expr).replace("(T > 0 ? T - 1 : 0)", "(T - 1 if T > 0 else 0)")
    assert "?" not in py and "u" not in py, py
    for T in (0, 1, 2, 3, 64, 818, 819, 820, 4096):
        assert eval(py, {"T": T}) == ci.lds_bytes(T), T
    assert "lds <= PAN_LDS_BYTES" in src and "(W + PAN_TILE_RANGES - 1u) / PAN_TILE_RANGES" in src and "(u32)((size + 3) / 4)" in src
    # the bound in taxa follows from the two: the LDS tier's largest launch asks for 65 472 bytes, a taxon more no longer fits
    assert ci.lds_bytes(ci.LDS_MAX_TAXA) <= ci.PAN_LDS_BYTES < ci.lds_bytes(ci.LDS_MAX_TAXA + 1)
    assert (ci.LDS_MAX_TAXA, ci.lds_bytes(ci.LDS_MAX_TAXA)) == (819, 65472) and ci.LDS_TAXA == (818, 819, 820)
    assert [c.fits_lds for c in map(ci.lds_case, ci.LDS_TAXA)] == [True, True, False]
    assert ci.shuffled_orders(0, 3).shape == (3, 0) and ci.shuffled_orders(4, 0).shape == (0, 4)


def test_orders_restate_the_script_and_are_prefixes(pan):
    for T in (2, 3, 5, 6, 9, 819):
        for size in (0, 1, 5, 20, 21):
            assert ci.shuffled_orders(T, size).tolist() == pan.permutations(T, size).tolist()
    assert ci.shuffled_orders(6, 21)[:20].tolist() == pan.permutations(6).tolist()


@pytest.mark.parametrize("case", ci.all_cases(), ids=lambda c: c.name)
def test_loops_equal_numpy(pan, case):
    counts, types, totals, curves = numpy_answer(pan, case)
    lc = ci.loop_counts(case.row, case.taxon, case.n_rows, case.n_taxa)
    assert counts.tolist() == lc and counts.shape == (case.n_rows, case.n_taxa)
    lt, ltot = ci.loop_types(lc, case.n_file_rows, case.spec_max, case.core_min)
    assert types.tolist() == lt and list(totals) == ltot
    for got, want in zip(curves, ci.loop_curves(lc, case.perm, case.S, case.C)):
        assert got.shape == (case.size, case.n_taxa - 1) and got.tolist() == want


@pytest.mark.parametrize("name", ["u0", "l_huge"])
def test_loops_equal_the_real_script(pan, name):
    """the loops on the two goldens: the script's own _xy.txt and `# Number` line, with orders and thresholds restated here"""
    taxa, table, res = library_result(pan, name)
    meta, T = pi.golden(name), len(taxa)
    ts, tc = pi.flag_values(pi.case_texts(name)[3])
    counts = ci.loop_counts(table.row, table.taxon, table.n_rows, T)
    S, C, spec_max, core_min = {"u0": ([0] * T, [0] * T, 1, 0), "l_huge": ([ci.I32_MAX] * T, [0] + list(range(2, T + 1)), ci.I32_MAX, T)}[name]
    # (u0: Ts = max(.05 j, 1) = 1, so S = 0; Tc = 0.  l_huge: Ts = 1e12; Tc = .95 j, whose ceiling is j up to j = 20)
    assert (ts, tc) == {"u0": (.05, 0.), "l_huge": (1e12, .95)}[name]
    core, spec, panz = ci.loop_curves(counts, ci.shuffled_orders(T, 20), S, C)
    xy = "".join("%d\t%d\t%d\t%d\n" % (i + 2, core[p][i], spec[p][i], panz[p][i]) for i in range(T - 1) for p in range(20))
    assert xy == meta["xy"]
    types, (n_core, n_share, n_spec) = ci.loop_types(counts, table.n_file_rows, spec_max, core_min)
    assert "\t".join(map(str, ["# Number", n_core, n_share, n_spec + table.n_rows - table.n_file_rows, T])) == meta["number"]
    assert [l.split("\t")[1] for l in meta["table"].split("\n")[1:-1]] == [pan.TYPE_NAMES[t] for t in types]
    assert [list(map(int, l.split("\t")[2:])) for l in meta["table"].split("\n")[1:-1]] == counts


def test_prefix_property(pan):
    """permutations(T, s) is a prefix of permutations(T, 20): the curves of the first s orders do not depend on how many follow"""
    full = numpy_answer(pan, ci.size_case(21))[3]
    for size in (0,) + ci.SIZES:
        case = ci.size_case(size)
        assert case.perm.tolist() == ci.size_case(21).perm[:size].tolist()
        for got, want in zip(numpy_answer(pan, case)[3], full):
            assert got.tolist() == want[:size].tolist()


def test_tables_hold_what_they_claim(pan):
    seen = set()
    for case in ci.all_cases():
        key = (case.n_rows, case.n_taxa)
        if key in seen:
            continue
        seen.add(key)
        counts = pan.count_matrix(case.row, case.taxon, case.n_rows, case.n_taxa)
        x = counts > 0
        assert x[0].all() and counts.max() <= 3 and len(case.row) == counts.sum()
        if case.n_rows < 63:
            continue
        cols = set(x[:, t].tobytes() for t in range(case.n_taxa))
        assert len(cols) == case.n_taxa, key                                  # no two taxa alike
        zero = int((x.sum(1) == 0).sum())
        assert zero >= sum(1 for r in range(case.n_rows - 1) if r % 7 == 3) and x[-1, 0] and x[-1, -1], key
        if case.n_taxa >= 5:                                                  # (with fewer taxa a row is often empty by chance, too)
            assert abs(zero / case.n_rows - 1 / 7) < .05, key
        assert (x.all(1)).sum() >= 1 and (counts == 2).sum() > 0 and (counts >= 2).sum() > .1 * x.sum(), key
        assert not np.array_equal(np.asarray(case.row), np.sort(case.row))    # the pairs come in any order
    assert len(seen) >= 25


def test_different_orders_give_different_curves(pan):
    """in every case two orders give the same curve exactly when they are the same order -- so a wave that walked another wave's order, or
    a flush into another order's counters, shows; and order 0 stands apart from every other"""
    for case in ci.all_cases():
        if case.n_taxa < 2 or case.n_rows < 63 or case.name.split("_")[-1] in ("C0", "C-5", "C-max", "C+max", "S-1", "S+max"):
            continue
        rows, perm = curve_rows(numpy_answer(pan, case)[3]), case.perm.tolist()
        for p in range(case.size):
            for q in range(p):
                assert (rows[p] == rows[q]) == (perm[p] == perm[q]), (case.name, p, q)
            assert any(rows[p][2]) and any(rows[p][0]) and any(rows[p][1]), case.name


def test_dead_waves_are_covered(pan):
    """every remainder of size modulo 4, in the first workgroup and in a later one; all orders of a size differ, so do their curves"""
    assert set(s % 4 for s in ci.SIZES) == {0, 1, 2, 3} and set(s % 4 for s in ci.SIZES if s > 4) == {0, 1, 3} and 21 in ci.SIZES
    assert ci.MASK_SIZE % 4 and ci.LDS_SIZE % 4 and ci.TILE_SIZE % 4
    case = ci.size_case(21)
    rows = curve_rows(numpy_answer(pan, case)[3])
    assert len(set(map(tuple, case.perm.tolist()))) == 21 and len(set(rows)) == 21
    # what a dead wave would add if it ran on the zeros it holds for an order (genome 0 at every step) is not nothing: it would show
    ghost = curve_rows(pan.rarefaction(pan.count_matrix(case.row, case.taxon, case.n_rows, case.n_taxa), np.zeros((1, case.n_taxa), dtype=np.int32), case.S, case.C))[0]
    assert any(ghost[0]) and any(ghost[2])
    names = [c.name for c in ci.order_cases()]
    assert names[:6] == ["identity", "reversed", "identity_reversed", "four_alike", "fifth_is_first", "last_taxon_first"]
    by = {c.name: c for c in ci.order_cases()}
    assert by["four_alike"].size == 4 and len(set(map(tuple, by["four_alike"].perm.tolist()))) == 1
    p5 = by["fifth_is_first"].perm.tolist()
    assert len(p5) == 5 and p5[4] == p5[0] and len(set(map(tuple, p5))) == 4
    assert by["last_taxon_first"].perm[0, 0] == ci.ORDER_TAXA - 1 and by["identity"].perm.tolist() == [list(range(9))]
    assert curve_rows(numpy_answer(pan, by["identity"])[3]) != curve_rows(numpy_answer(pan, by["reversed"])[3])
    assert [(c.n_taxa, c.size) for c in ci.order_cases()[6:]] == [(2, 1), (2, 5), (3, 1), (3, 5)]
    # the grid's height: two taxa have two orders, their curves differ, and the pattern of the orders has a period no group of 4 shares
    case = ci.grid_case(ci.GRID_ORDERS)
    rows = curve_rows(numpy_answer(pan, case)[3])
    assert case.size == 4 * 4096 + 1 and case.perm[:7].tolist() == [[1, 0], [0, 1], [0, 1], [1, 0], [0, 1], [0, 1], [1, 0]]
    assert len(set(rows)) == 2 and rows[0] != rows[1] and all(rows[p] == rows[p % 3 and 1] for p in range(case.size))
    assert ci.loop_curves(ci.loop_counts(case.row, case.taxon, case.n_rows, 2), case.perm[:9], case.S, case.C)[1] == [list(r[1]) for r in rows[:9]]


@pytest.mark.parametrize("n_rows", ci.MASK_ROWS)
def test_mask_and_extremes_decide(pan, n_rows):
    """C <= 0: every row is core, and whole tiles would count more wherever the last tile is partial; the other extremes give what their
    names say, and never what the moving thresholds give"""
    plain = ci.Case("plain", n_rows, ci.MASK_TAXA, ci.shuffled_orders(ci.MASK_TAXA, ci.MASK_SIZE))
    counts, _, _, (core0, spec0, panz0) = numpy_answer(pan, plain)
    x = counts > 0
    whole_tiles = 64 * ((n_rows + 63) // 64)
    assert (whole_tiles != n_rows) == (n_rows not in (64, 128))
    for name, (S, C, what) in sorted(ci.EXTREMES.items()):
        case = ci.mask_case(n_rows, name)
        assert (case.S[1:] == S).all() if S is not None else case.S.tolist() == plain.S.tolist()
        assert (case.C[1:] == C).all() if C is not None else case.C.tolist() == plain.C.tolist()
        core, spec, panz = numpy_answer(pan, case)[3]
        assert panz.tolist() == panz0.tolist()
        if what == "core_all":
            assert (core == n_rows).all() and spec.tolist() == spec0.tolist()
            if n_rows > 1:
                assert (panz < n_rows).all() or n_rows < 4          # (ys > 0 is not ys >= 0: the all-zero rows part them)
        elif what == "core_none":
            assert not core.any() and spec.tolist() == spec0.tolist()
        elif what == "spec_none":
            assert not spec.any() and core.tolist() == core0.tolist()
        else:
            assert spec.tolist() == [[int(x[:, t].sum()) for t in order[1:]] for order in case.perm.tolist()] and core.tolist() == core0.tolist()
        if n_rows >= 63:                                            # the extreme is not what the moving thresholds give
            assert (core.tolist(), spec.tolist()) != (core0.tolist(), spec0.tolist()), name


def test_tile_ranges_are_covered(pan):
    """tiles per range: 1 up to W = 256, 2 from 257, 3 at 513; the last range and the last tile each hold rows that count"""
    assert [ci.tile_grid(64 * W)[1:] for W in ci.TILE_W] == [(1, 1), (1, 255), (1, 256), (2, 129), (2, 256), (3, 171)]
    assert max(max(ci.tile_rows(W)) for W in ci.TILE_W) == 32832
    for W in ci.TILE_W:
        for n_rows in ci.tile_rows(W):
            case = ci.tile_case(n_rows)
            Wc, tiles, ranges = ci.tile_grid(n_rows)
            assert Wc == W and case.n_file_rows == max(n_rows - 3, 0) and (len(case.row) < 3 * n_rows or W == 1)
            counts, _, _, curves = numpy_answer(pan, case)
            rows = curve_rows(curves)
            for cut in (64 * (W - 1), 64 * tiles * (ranges - 1)):      # without the last tile; without the last range
                assert cut < n_rows
                less = curve_rows(pan.rarefaction(counts[:cut], case.perm, case.S, case.C))
                assert all(a != b for a, b in zip(rows, less)), (n_rows, cut)


def test_types_are_covered(pan):
    """every threshold pair gives another typing of the same table, and the rows behind the file rows would be typed otherwise"""
    assert ci.TYPE_FILE_ROWS == (0, 63, 64, 65, 129) and ci.TYPE_ROWS == 129
    seen = set()
    for th in ci.TYPE_THRESHOLDS:
        full = numpy_answer(pan, ci.type_case(ci.TYPE_ROWS, th))
        seen.add(tuple(full[1].tolist()))
        for f in ci.TYPE_FILE_ROWS:
            _, types, totals, _ = numpy_answer(pan, ci.type_case(f, th))
            assert sum(totals) == f and types[:f].tolist() == full[1][:f].tolist() and not types[f:].any()
            if f < ci.TYPE_ROWS and th != (5, 6):
                assert full[1][f:].any()
    assert len(seen) == len(ci.TYPE_THRESHOLDS)
    everything_specific = numpy_answer(pan, ci.type_case(129, (5, 6)))
    assert everything_specific[2] == (0, 0, 129)
    assert numpy_answer(pan, ci.type_case(129, (0, 0)))[2][1] == 0 and numpy_answer(pan, ci.type_case(129, (-1, 3)))[2][2] == 0
