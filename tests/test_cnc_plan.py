"""`find_cluster -a mcl -G A` on the CPU: the inputs of tests/cnc_plan_inputs.py hold what they promise (asserted from numpy alone);
row_plan() equals a literal restatement of the lines of cnc() it was cut from, on every input; single deviations of the plan are each
told apart by some input; cnc_columns() / groups_from_tables() with a numpy restatement of the device batch call plugged in equal
cnc() on the text find_orth would write, list for list; the flag, the binding and the refusals that come before a device is looked
for."""
import functools

import numpy as np
import pytest

import cnc_inputs as ci
import cnc_plan_inputs as pi
from mcl_scipy_oracle import scipy_mcl
from test_mcl_rows import numpy_block

FIELDS = ("gene_code", "X", "Y", "comp1", "grp", "order", "cut", "tied")
DEVIATIONS = ("unsigned_group_order", "unstable_ties", "order_by_gene_number", "cut_at_tie")


def old_front(cx, cy, Z, n_codes, deviation=None):
    """cnc() between _edge_columns() and its batch loop as it stood before row_plan() was cut out of it, statement for statement ->
    the fields of RowPlan.  `deviation`: one of DEVIATIONS, a single wrong turn"""
    from swiftortho_amd import find_cluster as fc
    assert deviation is None or deviation in DEVIATIONS
    nrow = len(cx)
    if nrow == 0:
        return tuple(np.zeros(0, dtype=np.int64) for _ in FIELDS)
    seq = np.empty(2 * nrow, dtype=np.int64)
    seq[0::2], seq[1::2] = cx, cy
    vals, first = np.unique(seq, return_index=True)
    order = np.argsort(first, kind='stable')
    number_of_code = np.zeros(n_codes, dtype=np.int64)
    number_of_code[vals[order]] = np.arange(len(vals))
    X, Y = number_of_code[cx], number_of_code[cy]
    gene_code = vals[order]
    n = len(vals)
    res = fc.group_numbers(X, Y, Z, n)
    grp = res[1]
    gx, gy = grp[X], grp[Y]
    keep = np.flatnonzero((gx != 0) & (gy != 0) & (gx == gy))
    kg, kx, ky = gx[keep], cx[keep], cy[keep]
    if deviation == "order_by_gene_number":
        kx, ky = X[keep], Y[keep]
    order = np.lexsort((ky, kx, kg.astype(np.uint32) if deviation == "unsigned_group_order" else kg))
    sg, sx, sy = kg[order], kx[order], ky[order]
    dup = np.flatnonzero((sg[1:] == sg[:-1]) & (sx[1:] == sx[:-1]) & (sy[1:] == sy[:-1]))
    if deviation == "unstable_ties" and len(dup):
        run_start = dup[np.concatenate([[True], np.diff(dup) > 1])]
        for s0 in run_start.tolist():
            e0 = s0 + 1
            while e0 < len(order) and sg[e0] == sg[s0] and sx[e0] == sx[s0] and sy[e0] == sy[s0]:
                e0 += 1
            order[s0:e0] = order[s0:e0][::-1].copy()
    rows_sorted = keep[order]
    kcls = kg[order]
    change = np.concatenate([[0], np.flatnonzero(kcls[1:] != kcls[:-1]) + 1, [len(kcls)]])
    cut, tied = change[1:-1], dup + 1
    if deviation == "cut_at_tie":
        cut = np.union1d(cut, tied)
    return gene_code, X, Y, res[0], grp, rows_sorted, cut, tied


@functools.lru_cache(maxsize=None)
def plan(name):
    from swiftortho_amd import find_cluster as fc
    P = fc.row_plan(*pi.inputs()[name])
    for f in FIELDS:
        getattr(P, f).setflags(write=False)
    return P


def sorted_triples(name):
    cx, cy, _, _ = pi.inputs()[name]
    P = plan(name)
    return P.grp[P.X[P.order]], cx[P.order], cy[P.order]


def test_the_inputs_hold_what_they_promise():
    B = pi.inputs()
    assert sorted(k for k in B if not k.endswith("_reversed")) == sorted(k[:-9] for k in B if k.endswith("_reversed"))
    for name, (cx, cy, z, n_codes) in B.items():
        assert len(cx) == len(cy) == len(z) and np.all(cx <= cy) and not np.isnan(z).any(), name
        if len(cx):
            assert cx.min() >= 0 and cy.max() < n_codes, name
        if name.endswith("_reversed"):
            assert np.array_equal(cx[::-1], B[name[:-9]][0]) and np.array_equal(cy[::-1], B[name[:-9]][1]) and np.array_equal(z[::-1], B[name[:-9]][2])
        P = plan(name)
        g, sx, sy = sorted_triples(name)
        # whatever has a row keeps a row of the pool, and the pool comes first
        assert (len(P.order) > 0) == (len(cx) > 0), name
        if len(cx):
            assert g[0] == -1 and np.all(np.diff(g) >= 0) and not np.any(g == 0), name
            assert np.array_equal(np.sort(P.gene_code), np.unique(np.concatenate([cx, cy]))), name
    assert len(B["no_rows"][0]) == 0 and B["no_rows"][3] == 5 and len(B["one_row"][0]) == 1 and len(B["two_rows"][0]) == 2 and len(B["two_rows_shared"][0]) == 2
    assert pi.LANES == 256 and pi.SCAN_TILE == 256 * 4 * 8 and pi.SCAN_ONE_LAUNCH == 4 * pi.SCAN_TILE
    # first appearance against the codes: every group of four genes lies below all groups before it
    gc = plan("codes_against_appearance").gene_code
    assert len(gc) == 162 and np.all(gc[:160].reshape(40, 4).max(axis=1)[1:] < gc[:160].reshape(40, 4).min(axis=1)[:-1]) and gc[160:].max() < gc[:160].min()
    # unused codes below, between and above
    cx, cy, z, n_codes = B["unused_codes"]
    used = np.unique(np.concatenate([cx, cy]))
    assert used[0] == 7 and np.all(np.diff(used) == 3) and n_codes == used[-1] + 1 + 11 and len(plan("unused_codes").order) == 40
    # as few kept rows as rows allow; everything kept; group 0 dropped
    assert len(plan("one_kept").order) == 1 and len(B["one_kept"][0]) == 4
    P = plan("one_component")
    assert len(P.order) == len(B["one_component"][0]) == 300 and np.all(P.grp == -1) and len(P.cut) == 0 and P.comp1.max() == 0
    for name in B:                                            # ... and nowhere else is every row kept
        assert name.startswith(("one_component", "one_row", "no_rows")) or plan(name).comp1.max() == 0 or len(plan(name).order) < len(B[name][0]), name
    P = plan("group0_dropped")
    assert (P.grp == 0).sum() == 4 and 0 < len(P.order) < len(B["group0_dropped"][0]) and set(sorted_triples("group0_dropped")[0].tolist()) == {-1, 1}
    for k in pi.KEPT:
        P = plan("kept%d" % k)
        assert len(P.order) == k and len(B["kept%d" % k][0]) == k + 3 and len(P.cut) == (k - 1) // 3, k
        assert not np.array_equal(P.gene_code, np.sort(P.gene_code)) and len(P.tied) == 0
    for n in pi.ROWS:
        assert len(B["rows%d" % n][0]) == n and 2 * pi.ROWS[1] == pi.SCAN_ONE_LAUNCH
    # self pairs among the rows and among the kept rows
    cx, cy, _, _ = B["self_pairs"]
    assert int((cx == cy).sum()) == 4 and int((cx[plan("self_pairs").order] == cy[plan("self_pairs").order]).sum()) >= 2
    cx, cy, z, n_codes = B["family"]
    assert 18000 <= len(cx) <= 22000 and len(plan("family").gene_code) == 4000 and n_codes == 5000 and len(plan("family").tied) >= 5 and len(plan("family").cut) >= 50
    assert len(plan("family").order) > 15000


@pytest.mark.parametrize("times,tied", [(2, [256]), (3, [256, 257]), (64, list(range(225, 288)))])
def test_the_repeated_pair(times, tied):
    """the repeats straddle positions 255 | 256 of the order; among them the rows stand in file order, which is against their weights' text"""
    name = "repeat%d_straddles_256" % times
    cx, cy, z, _ = pi.inputs()[name]
    P = plan(name)
    assert P.tied.tolist() == tied and tied[0] - 1 <= 255 < 256 <= tied[-1]
    run = P.order[tied[0] - 1:tied[-1] + 1]
    assert len(run) == times and np.all(np.diff(run) > 1)                       # file order, other rows between them
    assert np.all(np.diff(z[run]) < 0)                                          # heaviest first
    text = [repr(float(v)).encode() for v in z[run]]
    assert sorted(text) == text[::-1]                                           # the weights' text orders them the other way round
    R = plan(name + "_reversed")
    assert len(R.tied) == times - 1 and np.all(np.diff(pi.inputs()[name + "_reversed"][2][R.order[R.tied[0] - 1:R.tied[-1] + 1]]) > 0)


@pytest.mark.parametrize("name", sorted(pi.inputs()))
def test_row_plan_equals_the_lines_it_was_cut_from(name):
    want = old_front(*pi.inputs()[name])
    P = plan(name)
    for f, w in zip(FIELDS, want):
        got = getattr(P, f)
        assert got.dtype == np.int64 and np.array_equal(got, w), (name, f)


@pytest.mark.parametrize("deviation,name", [("unsigned_group_order", "group0_dropped"), ("unsigned_group_order", "kept256"), ("unstable_ties", "repeat2_straddles_256"),
                                            ("unstable_ties", "repeat64_straddles_256"), ("unstable_ties", "family"), ("order_by_gene_number", "kept257"),
                                            ("order_by_gene_number", "unused_codes"), ("cut_at_tie", "repeat3_straddles_256"), ("cut_at_tie", "family")])
def test_single_deviations_are_told_apart(deviation, name):
    """each wrong turn changes `order` or `cut` on the input named beside it (and the restatement without one changes nothing)"""
    P = plan(name)
    got = old_front(*pi.inputs()[name], deviation=deviation)
    differs = [f for f, w in zip(FIELDS, got) if not np.array_equal(getattr(P, f), w)]
    assert differs and set(differs) <= {"order", "cut", "tied"}, (deviation, name, differs)
    assert ("cut" in differs) == (deviation in ("cut_at_tie", "unsigned_group_order"))      # (the pool at the far end moves every cut)


def test_every_deviation_has_an_input():
    assert set(DEVIATIONS) == {"unsigned_group_order", "unstable_ties", "order_by_gene_number", "cut_at_tie"}
    assert len(ci.DEVIATIONS) >= 1          # (the component stage's own table lives in cnc_inputs)


# ---- columns and tables instead of text ---------------------------------------------------------------------------------------------
def tables_from_rows(rows, both=()):
    """rows (a, b, value) over ids (bytes) -> (names, RelationTables): the rows dealt out over the IP, OT and CO sections in turn, every
    fifth one turned round (b, a); `both`: (a, b, value in OT, value in CO) occur in the OT and in the CO section"""
    from swiftortho_amd import find_orth as fo
    ids = sorted({g for a, b, _ in rows for g in (a, b)} | {g for a, b, _, _ in both for g in (a, b)})
    names = np.array(ids, dtype=np.bytes_)
    code = {g: k for k, g in enumerate(ids)}
    sec = {"ip": [], "ot": [], "co": []}
    for k, (a, b, v) in enumerate(rows):
        a, b = (code[a], code[b]) if k % 5 else (code[b], code[a])
        sec[("ip", "ot", "co")[k % 3]].append((a, b, v))
    for a, b, v_ot, v_co in both:
        lo, hi = sorted((code[a], code[b]))
        sec["ot"].append((lo, hi, v_ot))
        sec["co"].append((lo, hi, v_co))
    cols = []
    for k in ("ip", "ot", "co"):
        cols += [np.array([r[0] for r in sec[k]], dtype=np.int64), np.array([r[1] for r in sec[k]], dtype=np.int64), np.array([r[2] for r in sec[k]], dtype=np.float64)]
    return names, fo.RelationTables(*cols)


def id_rows(rows):
    ident = lambda g: ("t%d|p%03d_%02d" % (g[0] % 4, g[0], g[1])).encode()
    return [(ident(a), ident(b), w * (1 + 1 / 3.0)) for a, b, w in rows]    # (values whose repr runs to 17 digits)


def table_cases():
    fam = id_rows(ci.family_graph(41, 120, 9, 0.5, 0.4))
    (a, b), (c, d), (e, f) = fam[301][:2], fam[601][:2], fam[901][:2]
    small = id_rows(ci.family_graph(5, 6, 5, 0.7, 1.0))
    return {"family": (fam, ()),
            "both_sections_differ": (fam, ((a, b, 12.5, 3.0625), (c, d, 0.30000000000000004, 0.3), (e, f, 9.0, 10.0))),
            "both_sections_equal": (fam, ((a, b, 7.25, 7.25), (c, d, fam[601][2], fam[601][2]), (e, f, 0.1, 0.1))),
            "small": (small, ((small[0][0], small[0][1], 2.0, 10.0),)),
            "large": (id_rows(ci.family_graph(31, 200, 18)), ())}


@pytest.mark.parametrize("case,chk", [(c, k) for c in sorted(table_cases()) for k in (10 ** 7, 50) if (c, k) != ("large", 50)])   # (the large table runs once)
def test_tables_equal_the_text_they_would_be_written_as(case, chk):
    from swiftortho_amd import find_cluster as fc, find_orth as fo
    names, tables = tables_from_rows(*table_cases()[case])
    text = b"".join(l + b"\n" for l in fo.lines_from_tables(names, tables))
    want = fc.cnc(text, 1.5, chk=chk, mcl=scipy_mcl)
    assert len(want) > 3 and any(len(g) > 2 for g in want)
    calls = []

    def block(*args):
        calls.append(len(args[0]))
        return numpy_block(*args)
    assert fc.groups_from_tables(names, tables, 1.5, chk=chk, mcl=scipy_mcl) == want
    assert fc.groups_from_tables(names, tables, 1.5, chk=chk, mcl=scipy_mcl, block=block) == want and len(calls) >= 1
    if case.startswith("both_sections"):
        a = np.concatenate([tables.ip_a, tables.ot_a, tables.co_a])
        b = np.concatenate([tables.ip_b, tables.ot_b, tables.co_b])
        use = a <= b
        P = fc.row_plan(a[use], b[use], np.concatenate([tables.ip_v, tables.ot_v, tables.co_v])[use], len(names))
        assert len(P.tied) >= 3          # (with its own row each pair stands three times)


def test_cnc_columns_is_cnc_behind_the_tokeniser():
    from swiftortho_amd import find_cluster as fc
    rows = ci.family_graph(41, 120, 9, 0.5, 0.4)
    lines = ["g%03d|%02d\tg%03d|%02d\t%r\n" % (a[0], a[1], b[0], b[1], w) for a, b, w in rows]
    want = fc.cnc(lines, 1.5, chk=50, mcl=scipy_mcl)
    names, cx, cy, Z, ztext = fc._edge_columns(lines)
    seen = []

    def plan_spy(*args):
        seen.append(len(args[0]))
        return fc.row_plan(*args)
    assert fc.cnc_columns(names, cx, cy, Z, ztext, 1.5, 50, scipy_mcl) == want
    assert fc.cnc_columns(names, cx, cy, Z, ztext, 1.5, 50, scipy_mcl, block=numpy_block, plan=plan_spy) == want and seen == [len(cx)]
    assert fc.cnc_columns(names, cx[:0], cy[:0], Z[:0], ztext) == []


def test_flag_table_and_manual_carry_the_all_value(capsys):
    from swiftortho_amd import find_cluster as fc
    assert fc.DEFAULTS["-G"] == "F"
    assert fc.parse(["find_cluster.py", "-i", "x", "-G", "A"])["-G"] == "A" and fc.parse(["find_cluster.py", "-i", "x", "-Ga"])["-G"] == "a"
    fc.manual_print()
    out = capsys.readouterr().out
    assert "  -G: " in out and "A|T|M|F" in out


def test_main_hands_the_all_value_to_cnc(monkeypatch, tmp_path):
    """-G A / -Ga select device_stage='all'; the other values what they selected before"""
    from swiftortho_amd import find_cluster as fc
    seen = []
    monkeypatch.setattr(fc, "cnc", lambda f, ifl, device_stage=False: seen.append(device_stage) or [])
    monkeypatch.setattr(fc, "device_mcl", lambda *a, **k: None)
    inp = tmp_path / "in.orth"
    inp.write_text("a|1\ta|2\t1.0\n")
    for flags in (["-G", "A"], ["-Ga"], ["-G", "M"], ["-G", "T"], ["-G", "F"], []):
        assert fc.main(["find_cluster.py", "-i", str(inp), "-a", "mcl"] + flags) == 0
    assert seen == ["all", "all", "matrix", True, False, False]


def test_a_nan_weight_keeps_the_numpy_plan(monkeypatch):
    """cnc(device_stage='all') never hands a NaN weight to the device plan"""
    from swiftortho_amd import find_cluster as fc
    monkeypatch.setattr(fc, "device_row_plan", lambda *a, **k: pytest.fail("the device plan was asked"))
    lines = ["a|0\ta|1\t5.0\n", "b|0\tb|1\t5.0\n", "a|0\tb|0\t1.0\n", "c|0\tc|1\tnan\n", "z|0\tz|1\t5.0\n"]
    with np.errstate(all="ignore"):
        want = fc.cnc(lines, 1.5, mcl=scipy_mcl)
        assert fc.cnc(lines, 1.5, mcl=scipy_mcl, device_stage="all", block=numpy_block) == want


def test_exports_name_the_new_symbols():
    from swiftortho_amd import _lib
    assert {"so_cnc_plan", "so_cnc_plan_free"} <= set(_lib.EXPORTS)
    import ctypes as C
    assert C.sizeof(_lib.SoCncPlanResult) == 8 * 8 + 4 * 4 + 8 * C.sizeof(C.c_void_p)


@pytest.fixture(scope="module")
def built():
    from swiftortho_amd import build
    build.build(verbose=False)


def refused(args, flags=0):
    """(return code, message, the result structure) of so_cnc_plan through the C ABI"""
    import ctypes as C
    from swiftortho_amd import _lib
    L = _lib.load()
    cx, cy, z, n_codes = args
    x, y, w = np.ascontiguousarray(cx, dtype=np.int32), np.ascontiguousarray(cy, dtype=np.int32), np.ascontiguousarray(z, dtype=np.float64)
    res = _lib.SoCncPlanResult()
    res.n_genes = 77                                      # (the call clears the structure before anything else)
    rc = L.so_cnc_plan(0, int(n_codes), len(x), x.ctypes.data, y.ctypes.data, w.ctypes.data, flags, C.byref(res))
    return rc, L.so_cnc_last_error().decode(), res


def nothing_allocated(res):
    return not any(bool(getattr(res, f)) for f in ("gene_code", "x", "y", "comp1", "grp", "order", "cut", "tied")) and res.n_genes == 0 and res.n_keep == 0 and res.waits == 0


@pytest.mark.parametrize("name", sorted(pi.refusals()))
def test_refusals_come_before_the_device(name, built):
    """non-zero, the message, no result allocated -- on a machine without a device too, so nothing was launched"""
    import ctypes as C
    from swiftortho_amd import _lib
    args, message = pi.refusals()[name]
    rc, msg, res = refused(args)
    assert rc != 0 and message in msg, msg
    assert nothing_allocated(res)
    L = _lib.load()
    x, w = np.zeros(1, dtype=np.int32), np.zeros(1)
    assert L.so_cnc_plan(0, 1, -1, x.ctypes.data, x.ctypes.data, w.ctypes.data, 0, C.byref(res)) != 0 and "bad arguments" in L.so_cnc_last_error().decode()
    assert L.so_cnc_plan(0, 1, 1 << 31, x.ctypes.data, x.ctypes.data, w.ctypes.data, 0, C.byref(res)) != 0 and "2^31" in L.so_cnc_last_error().decode()
    assert L.so_cnc_plan(0, 1, 0, None, None, None, 0, None) != 0


def test_device_plan_fails_loudly_without_a_gpu(built):
    """no CPU path: device_row_plan reports the missing device, for an input without a row too"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from swiftortho_amd import find_cluster as fc
    for name in ("one_row", "no_rows"):
        with pytest.raises(RuntimeError) as e:
            fc.device_row_plan(*pi.inputs()[name])
        assert "HIP" in str(e.value)
