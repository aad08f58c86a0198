"""The host side of `find_cluster -a apc -G A` without a GPU: find_cluster.apc_entry_columns() -- the numpy definition the device stage
(libsohit so_apc_rows, swiftortho_amd/csrc/apc.hip) is pinned to -- is the column half of apc_entries(); the inputs of
tests/apc_rows_inputs.py hold what their names promise; apc_columns() / apc_from_tables() / apc(device_stage=True) with the literal
oracle as the loop and a numpy restatement of the device call plugged in reproduce the reference's stdout; the command line and
pipeline.groups_from_search() hand the new values on.  tests/test_gpu_apc_rows.py runs the same inputs on the device."""
import inspect
import os

import numpy as np
import pytest

import apc_rows_inputs as RI
from apc_edge_inputs import LM, W
from apc_numpy_oracle import apc_rounds, numpy_apc
from conftest import GOLD
from test_find_cluster_apc import CASES, _case, _text


@pytest.fixture(scope="module")
def built():
    from swiftortho_amd import build
    build.build(verbose=False)


_ORACLE_RUNS = {}


def oracle_loop(row, col, score, n, damp, rounds=100):
    """numpy_apc, each entry list run once (the paths under test hand the same list to the loop again and again); read-only"""
    key = (np.asarray(row).tobytes(), np.asarray(col).tobytes(), np.asarray(score, dtype=np.float32).tobytes(), int(n), float(damp), int(rounds))
    if key not in _ORACLE_RUNS:
        _ORACLE_RUNS[key] = numpy_apc(row, col, score, n, damp, rounds)
        for x in _ORACLE_RUNS[key]:
            x.setflags(write=False)
    return _ORACLE_RUNS[key]


def numpy_rows(cx, cy, z, n_codes, taxon_of_code, damp, rounds=100):
    """device_apc_rows restated: the definition, then the literal oracle"""
    from swiftortho_amd import find_cluster as fc
    gene_code, row, col, score, n, _ = fc.apc_entry_columns(cx, cy, z, n_codes, taxon_of_code)
    return gene_code, oracle_loop(row, col, score, n, damp, rounds)[0]


def golden_inputs():
    return sorted({_case(n, v)[0] for n, v in CASES})


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inp", golden_inputs(), ids=os.path.basename)
def test_apc_entries_is_tokeniser_then_columns(inp, built, monkeypatch):
    """apc_entries(text) == tokeniser, taxon codes, apc_entry_columns -- field for field, the scores as uint32 -- wherever the tokeniser
    takes the input; and equals the literal loop's list everywhere"""
    from swiftortho_amd import find_cluster as fc
    data = open(inp, "rb").read()
    monkeypatch.setenv("SOHIT_TSV_NATIVE", "0")
    literal = fc.apc_entries(data)
    monkeypatch.setenv("SOHIT_TSV_NATIVE", "1")
    monkeypatch.setenv("SOHIT_TSV_MIN", "0")
    got = fc.apc_entries(data)
    assert got[0] == literal[0] and got[4] == literal[4]
    for a, b in zip(got[1:4], literal[1:4]):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    kind = fc._apc_input(data)
    if kind[0] != "columns":
        assert os.path.basename(inp) in ("apc_odd_rows.orth", "apc_hub_edges.orth"), inp     # (rows only the literal loop can judge)
        return
    ids, cx, cy, z = kind[1:]
    tax, n_taxa = fc._taxon_codes(ids)
    assert tax.dtype == np.int32 and n_taxa == len(set(g.split("|")[0] for g in ids)) == int(tax.max()) + 1
    assert all((tax[i] == tax[j]) == (ids[i].split("|")[0] == ids[j].split("|")[0]) for i in range(0, len(ids), 7) for j in range(0, len(ids), 5))
    gene_code, row, col, score, n, n_used = fc.apc_entry_columns(cx, cy, z, len(ids), tax)
    assert [ids[c] for c in gene_code.tolist()] == got[0] and n == got[4]
    assert row.dtype == np.int32 and col.dtype == np.int32 and score.dtype == np.float32
    assert np.array_equal(row, got[1]) and np.array_equal(col, got[2]) and np.array_equal(score.view(np.uint32), got[3].view(np.uint32))
    assert n_used == len(set(g.split("|")[0] for g in got[0]))


def test_some_golden_goes_through_the_tokeniser(built, monkeypatch):
    from swiftortho_amd import find_cluster as fc
    monkeypatch.setenv("SOHIT_TSV_MIN", "0")
    kinds = {os.path.basename(i): fc._apc_input(open(i, "rb").read())[0] for i in golden_inputs()}
    assert sum(k == "columns" for k in kinds.values()) >= 4, kinds
    assert kinds["apc_odd_rows.orth"] == "rows"


@pytest.mark.parametrize("name", RI.NAMES)
def test_definition_by_hand(name):
    """apc_entry_columns against a literal restatement: a dictionary numbers the genes, a loop writes the entries"""
    cx, cy, z, n_codes, tax = RI.rows(name)
    gene_code, row, col, score, n, n_used = RI.definition(name)
    number, ent = {}, []
    for a, b, w in zip(cx.tolist(), cy.tolist(), z.tolist()):
        assert a <= b
        number.setdefault(a, len(number)), number.setdefault(b, len(number))
        with np.errstate(over="ignore"):
            w32 = np.float64(w).astype(np.float32)
        ent += [(number[a], number[b], w32), (number[b], number[a], w32)]
    used = len({int(tax[c]) for c in number})
    ent += [(g, g, np.float32(-20.0 * used)) for g in range(len(number))]
    assert gene_code.dtype == np.int64 and gene_code.tolist() == list(number) and n == len(number) and n_used == used
    assert row.dtype == np.int32 and col.dtype == np.int32 and score.dtype == np.float32
    assert row.tolist() == [e[0] for e in ent] and col.tolist() == [e[1] for e in ent]
    assert np.array_equal(score.view(np.uint32), np.array([e[2] for e in ent], dtype=np.float32).view(np.uint32))


# ---- the inputs hold what they promise -------------------------------------------------------------------------------------------------
def test_every_promised_input_is_there():
    assert {"one_row", "two_rows", "no_row", "codes_ascending", "codes_descending", "codes_shuffled", "unused_codes", "taxon_of_unused_codes_only", "one_taxon",
            "every_gene_its_taxon", "self_pairs"} <= set(RI.BASE_NAMES)
    assert (LM, W) == (32, 64) and RI.HUB_LENGTHS == (32, 33, 64, 65)
    for L in RI.HUB_LENGTHS:
        assert {"hub_first_L%d" % L, "hub_later_L%d" % L, "hub_self_L%d" % L} <= set(RI.BASE_NAMES)
    assert {"genes_%d" % d for d in (255, 256, 257)} | {"rows_%d" % n for n in (4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768, 32769)} <= set(RI.BASE_NAMES)
    assert {"repeated_2", "repeated_3", "repeated_64"} | {"weights_" + k for k in ("zeros", "denormal", "overflow", "nan", "pinf", "ninf", "tie_to_even", "round_up")} <= set(RI.BASE_NAMES)
    assert len(RI.ORDERED) == 4 and len(RI.NAMES) == 2 * len(RI.BASE_NAMES)
    for name in RI.BASE_NAMES:
        a, b = RI.rows(name), RI.rows(name + "_rev")
        assert np.array_equal(a[0][::-1], b[0]) and np.array_equal(a[1][::-1], b[1]) and np.array_equal(a[2][::-1].view(np.uint64), b[2].view(np.uint64))
    assert set(RI.HUNDRED) <= set(RI.BASE_NAMES) and all(RI.is_small(n) for n in RI.HUNDRED)


def test_sizes_and_codes():
    d = RI.definition
    assert d("one_row")[4] == 2 and len(d("one_row")[1]) == 4 and d("two_rows")[4] == 3 and len(d("two_rows")[1]) == 7
    assert d("no_row")[4] == 0 and len(d("no_row")[1]) == 0 and d("no_row")[5] == 0
    assert d("codes_ascending")[0].tolist() == list(range(12))
    desc = d("codes_descending")[0].tolist()
    assert desc[:2] == [10, 11] and desc[2:] == list(range(9, -1, -1))
    sh = d("codes_shuffled")[0]
    assert sorted(sh.tolist()) == list(range(40)) and np.any(np.diff(sh) < 0) and np.any(np.diff(sh) > 0)
    used = sorted(d("unused_codes")[0].tolist())
    assert used == list(RI.UNUSED_USED) and used[0] > 0 and used[-1] < RI.rows("unused_codes")[3] - 1 and any(b - a > 1 for a, b in zip(used, used[1:]))
    cx, cy, z, n_codes, tax = RI.rows("taxon_of_unused_codes_only")
    assert len(set(tax.tolist())) == 3 and d("taxon_of_unused_codes_only")[5] == 2 and not np.any(tax[d("taxon_of_unused_codes_only")[0]] == 2)
    assert d("taxon_of_unused_codes_only")[3][-1] == np.float32(-40.0)
    assert d("one_taxon")[5] == 1 and d("one_taxon")[3][-1] == np.float32(-20.0)
    e = d("every_gene_its_taxon")
    assert e[5] == e[4] == 7 and RI.rows("every_gene_its_taxon")[3] == 9
    for g in RI.GENE_COUNTS:
        x = d("genes_%d" % g)
        assert x[4] == g and RI.rows("genes_%d" % g)[3] == g + 5 and not np.array_equal(x[0], np.sort(x[0]))
    for n in RI.ROW_COUNTS:
        x = RI.rows("rows_%d" % n)
        assert len(x[0]) == n and np.any(x[0] == x[1])
        lens = np.bincount(d("rows_%d" % n)[1])
        assert ((lens <= LM).any() or n > 30000) and ((lens > LM).any() or n < 8000)


def test_row_lengths_at_the_lane_wave_split():
    """the hub's row -- and its column -- hold exactly L entries, the preference entry and the doubled self pair counted"""
    for L in RI.HUB_LENGTHS:
        for kind, hub_gene in (("first", 0), ("later", 1), ("self", 1)):
            for rev in ("", "_rev"):
                name = "hub_%s_L%d%s" % (kind, L, rev)
                gene_code, row, col, score, n, _ = RI.definition(name)
                rl, cl = np.bincount(row, minlength=n), np.bincount(col, minlength=n)
                assert np.array_equal(rl, cl)                                     # every entry is mirrored or diagonal
                h = int(np.argmax(rl))
                assert rl[h] == L and np.sum(rl == L) == 1 and rl.max() == L, (name, rl[h])
                if not rev:
                    assert h == hub_gene, name
                diag = int(np.sum((row == h) & (col == h)))
                assert diag == (3 if kind == "self" else 1), name
                if kind == "self":                                               # two off-list diagonal entries in front of the preference entry
                    at = np.flatnonzero((row == h) & (col == h))
                    assert at[1] == at[0] + 1 and at[0] % 2 == 0 and at[2] == len(row) - n + h
                assert np.sum((rl > 1) & (rl <= LM)) >= 1                         # short rows next to it


def test_pairs():
    gene_code, row, col, score, n, _ = RI.definition("self_pairs")
    assert int(np.sum(row[:len(row) - n] == col[:len(row) - n])) == 8 and np.bincount(row)[gene_code.tolist().index(2)] == 6
    for k in RI.REPEATS:
        cx, cy, z, _, _ = RI.rows("repeated_%d" % k)
        at = np.flatnonzero((cx == 0) & (cy == 1))
        assert len(at) == k and at[0] <= 255 and at[-1] >= 256 and np.array_equal(at, np.arange(at[0], at[0] + k))
        assert len(set(z[at].tolist())) == min(k, 5)
        _, row, col, _, n, _ = RI.definition("repeated_%d" % k)
        pairs = row.astype(np.int64) * n + col
        assert np.sum(pairs == pairs[2 * at[0]]) == k


def test_weights():
    sc = lambda kind: RI.definition("weights_" + kind)[3]
    bits = lambda kind: set(sc(kind).view(np.uint32).tolist())
    assert {0x00000000, 0x80000000} <= bits("zeros")
    den = sc("denormal")
    assert np.sum((den != 0) & (np.abs(den) < np.finfo(np.float32).tiny)) == 4      # kept, not flushed
    assert {0x7F800000, 0xFF800000} <= bits("overflow") and np.all(np.isfinite(RI.rows("weights_overflow")[2]))
    assert np.isnan(sc("nan")).sum() == 2 and 0x7F800000 in bits("pinf") and 0xFF800000 in bits("ninf")
    assert 0x3F800000 in bits("tie_to_even") and 0x3F800001 not in bits("tie_to_even")           # 1 + 2^-24 ties to even
    assert 0x3F800001 in bits("round_up")                                                         # a 2^-50 more rounds up
    assert RI.rows("weights_tie_to_even")[2][1] != 1.0


@pytest.mark.parametrize("name", RI.ORDERED)
def test_the_order_of_a_column_shows_in_a_bit(name):
    """from the oracle alone: after one round at damping 0.5 the A of the hub's diagonal entry carries the order of the column's entries
    -- moving the entries of that column to another order inside the list changes its last bit"""
    gene_code, row, col, score, n, _ = RI.definition(name)
    cx, cy, z, n_codes, _ = RI.rows(name)
    h = gene_code.tolist().index(n_codes - 1)
    assert np.bincount(col)[h] == (LM if "lane" in name else W + 7)
    diag = len(row) - n + h
    assert row[diag] == col[diag] == h
    a1 = next(iter(apc_rounds(row, col, score, n, 0.5, 1)))[2]
    want = 0x3E800001 if "tiny_first" in name else 0x3E800000
    assert int(a1.view(np.uint32)[diag]) == want
    at = np.flatnonzero((col == h) & (row != h))                                      # the column's entries, in entry order
    perm = np.arange(len(row))
    perm[at] = at[::-1]                                                               # ... handed their scores in reverse order
    a2 = next(iter(apc_rounds(row, col, score[perm], n, 0.5, 1)))[2]
    assert int(a2.view(np.uint32)[diag]) == (want ^ 1)
    rev = RI.definition(name + "_rev")
    a3 = next(iter(apc_rounds(rev[1], rev[2], rev[3], rev[4], 0.5, 1)))[2]
    hr = rev[0].tolist().index(n_codes - 1)
    assert int(a3.view(np.uint32)[len(rev[1]) - rev[4] + hr]) == (want ^ 1)           # and so do the reversed rows


# ---- columns and tables to groups -------------------------------------------------------------------------------------------------------
def _columns_of_text(inp):
    """(ids by code, cx, cy, z) of a relation file whose every x <= y row the literal loop keeps; None where it drops one (its genes
    then exist without a row, which columns cannot say)"""
    from swiftortho_amd import find_cluster as fc
    lines = open(inp).readlines()
    names, X, Y, Z = fc._apc_rows_python(lines)
    kept = sum(1 for x, y, _ in fc._rows(lines))
    if kept != len(X):
        return None
    ids = sorted(names, key=lambda g: g.encode("utf-8"))
    code = {g: c for c, g in enumerate(ids)}
    to_code = np.array([code[g] for g in names], dtype=np.int64)
    return ids, to_code[X], to_code[Y], Z


COLUMN_CASES = [(n, v) for n, v in CASES if _columns_of_text(_case(n, v)[0]) is not None]


def test_most_goldens_are_columns():
    assert len(CASES) == 10 and len(COLUMN_CASES) >= 7
    assert {n for n, _ in CASES} - {n for n, _ in COLUMN_CASES} <= {"odd_rows", "hub_edges"}


@pytest.mark.parametrize("name,variant", COLUMN_CASES)
def test_columns_and_tables_match_reference(name, variant):
    """apc_columns and apc_from_tables, through the entry list and `loop`, and through `rows`, print the reference's bytes"""
    from swiftortho_amd import find_cluster as fc, find_orth as fo
    inp, _, damp, want = _case(name, variant)
    ids, cx, cy, z = _columns_of_text(inp)
    calls = []

    def rows(*args):
        calls.append(len(args[0]))
        return numpy_rows(*args)
    no_rows = lambda *a: pytest.fail("the device stage was asked")
    no_loop = lambda *a: pytest.fail("the loop was asked on a host entry list")
    assert _text(fc.apc_columns(ids, cx, cy, z, damp, loop=oracle_loop, rows=no_rows)) == want
    assert _text(fc.apc_columns(ids, cx, cy, z, damp, device_stage=True, loop=no_loop, rows=rows)) == want and calls == [len(cx)]
    k1, k2 = len(cx) // 3, 2 * len(cx) // 3
    cols = []                                              # (a table may hold a pair's other direction too: rows with a > b are not used)
    for s in (slice(0, k1), slice(k1, k2), slice(k2, None)):
        a, b, v = cx[s], cy[s], z[s]
        m = a[:5] < b[:5]
        cols += [np.concatenate([a, b[:5][m]]), np.concatenate([b, a[:5][m]]), np.concatenate([v, v[:5][m] + 1.0])]
    tables = fo.RelationTables(*cols)
    names = np.array([g.encode("utf-8") for g in ids])
    assert _text(fc.apc_from_tables(names, tables, damp, loop=oracle_loop, rows=no_rows)) == want
    assert _text(fc.apc_from_tables(names, tables, damp, device_stage=True, loop=no_loop, rows=rows)) == want and len(calls) == 2


@pytest.mark.parametrize("name,variant", CASES)
def test_apc_with_the_device_stage_matches_reference(name, variant, built, monkeypatch):
    """apc(device_stage=True) on the ten goldens with the tokeniser forced: the bytes of the reference; input only the literal loop
    can judge keeps the host entry list"""
    from swiftortho_amd import find_cluster as fc
    monkeypatch.setenv("SOHIT_TSV_MIN", "0")
    inp, _, damp, want = _case(name, variant)
    calls = []

    def rows(*args):
        calls.append(1)
        return numpy_rows(*args)
    assert _text(fc.apc(open(inp), damp, loop=oracle_loop, device_stage=True, rows=rows)) == want
    assert calls == ([1] if fc._apc_input(open(inp))[0] == "columns" else [])
    if name == "odd_rows":
        assert calls == []


def test_tiny_input_keeps_the_host_path(built):
    """fewer than SOHIT_TSV_MIN lines: the literal loop reads them, whatever device_stage says"""
    from swiftortho_amd import find_cluster as fc
    inp, _, damp, want = _case("taxa5", "default")
    assert _text(fc.apc(open(inp), damp, loop=oracle_loop, device_stage=True, rows=lambda *a: pytest.fail("the device stage was asked"))) == want
    assert fc.apc_columns([], np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0), device_stage=True, rows=lambda *a: pytest.fail("asked")) == []


# ---- the command line and the pipeline ----------------------------------------------------------------------------------------------------
def test_flags():
    from swiftortho_amd import find_cluster as fc
    assert fc.DEFAULTS["-G"] == "F" and fc.DEFAULTS["-a"] == "apc"
    assert fc.parse(["find_cluster.py", "-i", "x", "-a", "apc", "-G", "A"])["-G"] == "A"
    assert fc.parse(["find_cluster.py", "-i", "x", "-a", "apc", "-Ga"])["-G"] == "a"
    assert fc.parse(["find_cluster.py", "-i", "x", "-a", "apc"])["-G"] == "F"


@pytest.mark.parametrize("flags,device", [(["-G", "A"], True), (["-Ga"], True), (["-G", "T"], False), (["-G", "M"], False), (["-G", "F"], False), ([], False)])
def test_main_selects_the_device_stage(flags, device, built, monkeypatch, capsys):
    """`-a apc -G A` goes through device_apc_rows; -G T, -G M, -G F and no -G through the entry list and device_apc"""
    from swiftortho_amd import find_cluster as fc
    monkeypatch.setenv("SOHIT_TSV_MIN", "0")
    inp, _, damp, want = _case("taxa5", "default")
    asked = []

    def rows(cx, cy, z, n_codes, tax, d, **kw):
        asked.append("rows")
        return numpy_rows(cx, cy, z, n_codes, tax, d)

    def loop(row, col, score, n, d, **kw):
        if len(row) > 1:                                  # (the warm-up thread's 1 x 1 problem is not the command's call)
            asked.append("loop")
        return oracle_loop(row, col, score, n, d, kw.get("rounds", 100))
    monkeypatch.setattr(fc, "device_apc_rows", rows)
    monkeypatch.setattr(fc, "device_apc", loop)
    assert fc.main(["find_cluster.py", "-i", inp, "-a", "apc"] + flags) == 0
    assert capsys.readouterr().out == want
    assert asked == (["rows"] if device else ["loop"])


def test_groups_from_search_has_the_new_keywords(tmp_path):
    from swiftortho_amd import pipeline
    sig = inspect.signature(pipeline.groups_from_search)
    assert sig.parameters["algorithm"].default == "mcl" and sig.parameters["damp"].default == 0.5
    assert sig.parameters["device_stage"].default == "all" and sig.parameters["inflation"].default == 1.5
    missing = str(tmp_path / "not_there.fsa")
    with pytest.raises(ValueError, match="sap"):
        pipeline.groups_from_search(missing, algorithm="sap")          # (refused before the file is opened)
    with pytest.raises(OSError):
        pipeline.groups_from_search(missing, algorithm="apc")


def test_exports_and_signatures():
    import ctypes as C
    from swiftortho_amd import _lib, find_cluster as fc
    assert {"so_apc_rows", "so_apc_rows_free"} <= set(_lib.EXPORTS)
    assert C.sizeof(_lib.SoApcRowsResult) == 5 * 8 + 2 * 4 + 7 * C.sizeof(C.c_void_p)
    p = inspect.signature(fc.device_apc_rows).parameters
    assert list(p)[:6] == ["cx", "cy", "z", "n_codes", "taxon_of_code", "damp"] and p["rounds"].default == 100 and p["want_entries"].default is False
    p = inspect.signature(fc.apc_columns).parameters
    assert list(p) == ["names", "cx", "cy", "Z", "damp", "device_stage", "loop", "rows"] and p["device_stage"].default is False
    p = inspect.signature(fc.apc).parameters
    assert list(p)[:3] == ["lines", "damp", "loop"] and p["device_stage"].default is False
    assert inspect.signature(fc.apc_from_tables).parameters["device_stage"].default is False


# ---- refusals: before a device is touched -------------------------------------------------------------------------------------------------
def call_rows(cx, cy, z, n_codes, tax, n_taxa=None, n_rows=None, rounds=1, flags=0):
    """(return code, message, the result structure) of so_apc_rows through the C ABI"""
    import ctypes as C
    from swiftortho_amd import _lib
    L = _lib.load()
    x, y = np.ascontiguousarray(cx, dtype=np.int32), np.ascontiguousarray(cy, dtype=np.int32)
    w, t = np.ascontiguousarray(z, dtype=np.float64), np.ascontiguousarray(tax, dtype=np.int32)
    res = _lib.SoApcRowsResult()
    res.n_genes = 77                                      # (the call clears the structure before anything else)
    rc = L.so_apc_rows(0, int(n_codes), len(x) if n_rows is None else n_rows, x.ctypes.data, y.ctypes.data, w.ctypes.data, t.ctypes.data,
                       (int(t.max()) + 1 if len(t) else 0) if n_taxa is None else n_taxa, 0.5, rounds, flags, C.byref(res))
    return rc, L.so_apc_last_error().decode(), res


def nothing_allocated(res):
    return not any(bool(getattr(res, f)) for f in ("gene_code", "labels", "row", "col", "score", "r", "a")) and res.n_genes == 0 and res.n_entries == 0 and res.waits == 0


def refusals():
    """name -> (arguments of call_rows, a word of the message)"""
    ok = ([0, 1], [1, 2], [1.0, 2.0], 3, [0, 1, 0])
    return {"negative_rows": (ok, dict(n_rows=-1), "bad arguments"), "negative_codes": (ok[:3] + (-1, ok[4]), {}, "bad arguments"),
            "negative_taxa": (ok, dict(n_taxa=-1), "bad arguments"), "negative_rounds": (ok, dict(rounds=-1), "bad arguments"),
            "rows_2_31": (ok, dict(n_rows=1 << 31), "2^31"), "codes_2_31": (ok[:3] + (1 << 31, ok[4]), {}, "2^31"), "taxa_2_31": (ok, dict(n_taxa=1 << 31), "2^31"),
            "code_above": (([0, 1], [1, 3], [1.0, 2.0], 3, [0, 1, 0]), {}, "code outside"), "code_below": (([-1, 1], [1, 2], [1.0, 2.0], 3, [0, 1, 0]), {}, "code outside"),
            "taxon_above": (ok[:4] + ([0, 2, 0],), dict(n_taxa=2), "taxon outside"), "taxon_below": (ok[:4] + ([0, -1, 0],), dict(n_taxa=2), "taxon outside"),
            "cx_above_cy": (([0, 2], [1, 1], [1.0, 2.0], 3, [0, 1, 0]), {}, "cx > cy"),
            "too_many_entries": (([0], [0], [1.0], 1, [0]), dict(n_rows=(0x7FFFFFF0 >> 1) + 1), "too large")}


@pytest.mark.parametrize("name", sorted(refusals()))
def test_refusals_come_before_the_device(name, built):
    """non-zero, the message, no result allocated -- on a machine without a device too, so nothing was launched"""
    args, kw, word = refusals()[name]
    rc, msg, res = call_rows(*args, **kw)
    assert rc != 0 and word in msg and msg.startswith("so_apc_rows: "), msg
    assert nothing_allocated(res)


def test_device_apc_rows_fails_loudly_without_a_gpu(built):
    """no CPU path: device_apc_rows reports the missing device -- for an input without a row too"""
    import torch
    from swiftortho_amd import find_cluster as fc
    for name in ("one_row", "no_row") if not torch.cuda.is_available() else ():
        with pytest.raises(RuntimeError, match="HIP"):
            fc.device_apc_rows(*RI.rows(name), 0.5)
    with pytest.raises(ValueError):
        fc.device_apc_rows([0], [1, 2], [1.0], 3, [0, 0, 0], 0.5)
    with pytest.raises(RuntimeError, match="32 bits"):
        fc.device_apc_rows([0], [1 << 31], [1.0], 3, [0, 0, 0], 0.5)
