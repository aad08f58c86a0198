"""`find_cluster -a apc -G A` on the GPU (libsohit so_apc_rows, swiftortho_amd/csrc/apc.hip): on every input of tests/apc_rows_inputs.py the
entry list the device derives equals find_cluster.apc_entry_columns() field for field (scores as uint32), and labels, R and A after 1, 2,
3, 10 (and 100) rounds equal so_apc on the host-built entries BIT FOR BIT (same_bits: a NaN equals a NaN) -- and the literal oracle on
the small inputs; under stale device memory; a short input right behind a long one; the refusals; `-G A` down to the golden bytes; the
tables route and the one-process path from a FASTA file to the groups.  tests/test_apc_rows.py shows without a GPU that the inputs hold
what they promise."""
import os
import subprocess
import sys

import numpy as np
import pytest

import apc_rows_inputs as RI
from apc_edge_inputs import LM, W, same_bits
from conftest import GOLD, ROOT
from test_apc_rows import call_rows, nothing_allocated, refusals
from test_find_cluster_apc import CASES, _case, _text
from test_gpu_orth_relations import SEARCH_KW

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "bin", "find_cluster.py")
DAMPS = (0.5, 0.9)


def differing(got, want):
    x, y = got.view(np.uint32), want.view(np.uint32)
    return int(((x != y) & ~(np.isnan(got) & np.isnan(want))).sum())


def run_rows(name, damp, rounds, want_entries=True, info=None):
    from swiftortho_amd import find_cluster as fc
    return fc.device_apc_rows(*RI.rows(name), damp, rounds=rounds, want_entries=want_entries, info=info)


def check_loop(what, got, want):
    """got: device_apc_rows with entries; want: (labels, r, a)"""
    print(what, "labels differing", int((got[1] != want[0]).sum()), "R differing", differing(got[5], want[1]), "A differing", differing(got[6], want[2]), "of",
          len(want[1]), "NaN", int(np.isnan(want[1]).sum() + np.isnan(want[2]).sum()))
    assert got[1].dtype == np.int64 and got[5].dtype == np.float32 and got[6].dtype == np.float32
    assert np.array_equal(got[1], want[0]), what
    assert same_bits(got[5], want[1]), what
    assert same_bits(got[6], want[2]), what


def check_entries(name, got, info):
    gene_code, row, col, score, n, n_used = RI.definition(name)
    assert got[0].dtype == np.int64 and np.array_equal(got[0], gene_code), name
    assert got[2].dtype == np.int32 and np.array_equal(got[2], row), name
    assert got[3].dtype == np.int32 and np.array_equal(got[3], col), name
    assert got[4].dtype == np.float32 and np.array_equal(got[4].view(np.uint32), score.view(np.uint32)), name
    assert info["n_genes"] == n and info["n_entries"] == len(row) and info["n_taxa_used"] == n_used, (name, info)
    # one wait each for the number of genes, the list lengths and the end -- none per round
    assert info["waits"] == (3 if len(RI.rows(name)[0]) else 0), (name, info)


@pytest.mark.parametrize("name", RI.NAMES)
def test_entries_equal_the_definition(name):
    info = {}
    got = run_rows(name, 0.5, 1, info=info)
    check_entries(name, got, info)
    assert info["rounds"] == 1


@pytest.mark.parametrize("damp", DAMPS)
@pytest.mark.parametrize("name", RI.NAMES)
def test_rounds_equal_the_host_built_entries(name, damp):
    """labels, R and A after 1, 2, 3, 10 (100 on a few inputs) rounds: so_apc on the definition's entries, bit for bit; on the small
    inputs the literal oracle too"""
    from swiftortho_amd import find_cluster as fc
    _, row, col, score, n, _ = RI.definition(name)
    for t in RI.rounds_of(name):
        info = {}
        got = run_rows(name, damp, t, info=info)
        check_entries(name, got, info)
        check_loop("%s damp %s rounds %d against so_apc" % (name, damp, t), got, fc.device_apc(row, col, score, n, damp, rounds=t))
        if RI.is_small(name) and len(row):
            check_loop("%s damp %s rounds %d against the oracle" % (name, damp, t), got, RI.oracle_snapshots(name, damp)[t])


@pytest.mark.parametrize("name", RI.NAMES)
def test_labels_without_the_entries(name):
    """the command's call: gene codes and labels only"""
    from swiftortho_amd import find_cluster as fc
    gene_code, row, col, score, n, _ = RI.definition(name)
    got = run_rows(name, 0.5, 3, want_entries=False)
    assert len(got) == 2 and got[0].dtype == np.int64 and got[1].dtype == np.int64
    assert np.array_equal(got[0], gene_code) and np.array_equal(got[1], fc.device_apc(row, col, score, n, 0.5, rounds=3)[0])


@pytest.mark.parametrize("name", RI.ORDERED)
def test_ordered_column_bits(name):
    """the A of the hub's diagonal entry after one round holds the float32 of the column's float64 sum IN ENTRY ORDER"""
    got = run_rows(name, 0.5, 1)
    gene_code, row, col, score, n, _ = RI.definition(name)
    h = gene_code.tolist().index(RI.rows(name)[3] - 1)
    bits = int(got[6].view(np.uint32)[len(row) - n + h])
    print(name, "A of the diagonal %#x" % bits)
    assert bits == (0x3E800001 if "tiny_first" in name else 0x3E800000)


def test_taxa_of_genes_first_seen_in_the_second_column():
    """129 rows (2 x 129 = 258 positions: one workgroup and two positions of the next) in which every gene but the one at position 0
    -- cx of row 0, which no input can move -- first appears in the cy column, and taxa 1 and 2 are carried by those genes alone: the
    taxa in use come from the shared numbering's flags at the ODD positions, read by so_apc_rows' own kernel"""
    from swiftortho_amd import find_cluster as fc
    nrow = 129
    cy = np.random.RandomState(7).permutation(np.arange(1, nrow + 1)).astype(np.int32)   # code order is not gene order
    cx = np.zeros(nrow, dtype=np.int32)
    z = np.linspace(0.25, 3.0, nrow)
    tax = np.array([0] + [1 + c % 2 for c in range(1, nrow + 1)] + [3], dtype=np.int32)   # code nrow + 1 is unused: taxon 3 does not count
    gene_code, row, col, score, n, n_used = fc.apc_entry_columns(cx, cy, z, len(tax), tax)
    seq = np.stack([cx, cy], axis=1).ravel()
    first = np.array([np.flatnonzero(seq == c)[0] for c in gene_code])
    assert n == nrow + 1 and n_used == 3 and (first[1:] % 2 == 1).all() and first[0] == 0 and first.max() == 2 * nrow - 1 > 256
    assert set(tax[gene_code[first % 2 == 1]]) == {1, 2} and tax[gene_code[0]] == 0
    info = {}
    got = fc.device_apc_rows(cx, cy, z, len(tax), tax, 0.5, rounds=1, want_entries=True, info=info)
    assert np.array_equal(got[0], gene_code) and np.array_equal(got[2], row) and np.array_equal(got[3], col)
    assert np.array_equal(got[4].view(np.uint32), score.view(np.uint32))
    assert info["n_genes"] == n and info["n_entries"] == len(row) and info["n_taxa_used"] == n_used and info["waits"] == 3, info


def test_no_row():
    from swiftortho_amd import find_cluster as fc
    for want_entries in (False, True):
        info = {}
        got = fc.device_apc_rows(*RI.rows("no_row"), 0.5, want_entries=want_entries, info=info)
        assert len(got) == (7 if want_entries else 2) and all(len(x) == 0 for x in got)
        assert info == dict(n_genes=0, n_entries=0, n_taxa_used=0, rounds=100, waits=0)
    assert fc.device_apc_rows([], [], [], 0, [], 0.5)[1].dtype == np.int64


def test_zero_rounds():
    info = {}
    got = run_rows("codes_shuffled", 0.5, 0, info=info)
    assert np.array_equal(got[1], np.arange(len(got[0]))) and not got[5].any() and not got[6].any()
    check_entries("codes_shuffled", got, info)
    assert info["rounds"] == 0 and info["n_genes"] == 40


@pytest.mark.parametrize("name", sorted(refusals()))
def test_refusals_leave_a_message_and_the_next_call_works(name):
    args, kw, word = refusals()[name]
    rc, msg, res = call_rows(*args, **kw)
    assert rc != 0 and word in msg and msg.startswith("so_apc_rows: "), msg
    assert nothing_allocated(res)
    info = {}
    check_entries("two_rows", run_rows("two_rows", 0.5, 2, info=info), info)


def test_device_index_out_of_range():
    from swiftortho_amd import find_cluster as fc
    with pytest.raises(RuntimeError, match="device index out of range"):
        fc.device_apc_rows(*RI.rows("one_row"), 0.5, device=4096)


STALE = ("hub_self_L%d" % (W + 1), "repeated_64_rev", "weights_nan", "rows_8193")


@pytest.mark.parametrize("poison", ["0xFF", "0x5A"])
@pytest.mark.parametrize("name", STALE)
def test_stale_device_memory(name, poison, monkeypatch):
    """every fresh device allocation pre-filled (so_apc_rows reads SOHIT_POISON per call): nothing rests on what an allocation held"""
    from swiftortho_amd import find_cluster as fc
    assert name in RI.NAMES
    _, row, col, score, n, _ = RI.definition(name)
    want = {t: fc.device_apc(row, col, score, n, 0.5, rounds=t) for t in (1, 3, 10)}
    monkeypatch.setenv("SOHIT_POISON", poison)
    for t in (1, 3, 10):
        info = {}
        got = run_rows(name, 0.5, t, info=info)
        check_entries(name, got, info)
        check_loop("%s poison %s rounds %d" % (name, poison, t), got, want[t])
        assert np.array_equal(run_rows(name, 0.5, t, want_entries=False)[1], want[t][0])


def test_calls_do_not_depend_on_the_call_before():
    """a long input, then a short one, then back, in one process: each result equals so_apc's, whatever ran before"""
    from swiftortho_amd import find_cluster as fc
    long_, short = "rows_32769", "hub_later_L%d" % LM
    lens = lambda name: np.bincount(RI.definition(name)[1])
    assert (lens(long_) > LM).all() and (lens(short) <= LM).all()
    want = {}
    for name in (long_, short, "hub_first_L%d" % (W + 1)):
        _, row, col, score, n, _ = RI.definition(name)
        want[name] = fc.device_apc(row, col, score, n, 0.5, rounds=3)
    for name in (long_, short, long_, short, short, "hub_first_L%d" % (W + 1), short, long_):
        info = {}
        got = run_rows(name, 0.5, 3, info=info)
        check_entries(name, got, info)
        check_loop(name + " in sequence", got, want[name])


# ---- down to the bytes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", CASES)
def test_groups_match_reference_with_the_device_stage(name, variant, monkeypatch):
    """apc(device_stage=True) with the tokeniser forced (the goldens are small): the reference's bytes, through so_apc_rows wherever the
    tokeniser takes the input"""
    from swiftortho_amd import find_cluster as fc
    monkeypatch.setenv("SOHIT_TSV_MIN", "0")
    inp, _, damp, want = _case(name, variant)
    calls, real = [], fc.device_apc_rows
    got = _text(fc.apc(open(inp), damp, device_stage=True, rows=lambda *a, **k: calls.append(1) or real(*a, **k)))
    assert got == want
    assert calls == ([1] if fc._apc_input(open(inp))[0] == "columns" else [])


def test_the_device_stage_really_ran(monkeypatch):
    from swiftortho_amd import find_cluster as fc
    monkeypatch.setenv("SOHIT_TSV_MIN", "0")
    inp, _, damp, want = _case("taxa8_big", "default")
    monkeypatch.setattr(fc, "device_apc", lambda *a, **k: pytest.fail("the loop was asked on a host entry list"))
    assert _text(fc.apc(open(inp), damp, fc._device_loop, True, fc._device_rows)) == want


@pytest.mark.parametrize("name,variant", CASES)
def test_find_cluster_cli_apc_with_the_device_stage(name, variant, tmp_path):
    """`-a apc -G A` prints the golden bytes, with the goldens' few lines (the literal loop reads them) and with the tokeniser forced"""
    inp, flags, _, want = _case(name, variant)
    env = dict(os.environ, SOHIT_TSV_MIN="0") if variant == "default" else None
    r = subprocess.run([sys.executable, CLI, "-i", inp, "-G", "A"] + flags, capture_output=True, text=True, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == want
    assert os.listdir(str(tmp_path)) == []


def _tables_of_text(path):
    """the RelationTables a relation file was written from: (names as find_orth numbers them, tables)"""
    from swiftortho_amd import find_orth as fo
    rows = [l.rstrip(b"\n").split(b"\t") for l in open(path, "rb")]
    names = np.unique(np.array([r[1] for r in rows] + [r[2] for r in rows]))
    code = {g: c for c, g in enumerate(names.tolist())}
    cols = []
    for kind in (b"IP", b"OT", b"CO"):
        sec = [r for r in rows if r[0] == kind]
        cols += [np.array([code[r[1]] for r in sec], dtype=np.int64), np.array([code[r[2]] for r in sec], dtype=np.int64),
                 np.array([float(r[3]) for r in sec], dtype=np.float64)]
    return names, fo.RelationTables(*cols)


def test_tables_on_the_device_equal_the_text(monkeypatch):
    from swiftortho_amd import find_cluster as fc, find_orth as fo
    path = os.path.join(GOLD, "orth_taxa5.default.orth")
    names, tables = _tables_of_text(path)
    text = b"".join(l + b"\n" for l in fo.lines_from_tables(names, tables))
    want = fc.apc(text, 0.5)
    assert len(want) > 3 and any(len(g) > 2 for g in want)
    calls, real = [], fc.device_apc_rows
    assert fc.apc_from_tables(names, tables, 0.5, device_stage=True, rows=lambda *a, **k: calls.append(1) or real(*a, **k)) == want and calls == [1]
    assert fc.apc_from_tables(names, tables, 0.5) == want
    monkeypatch.setenv("SOHIT_TSV_MIN", "0")
    assert fc.apc(text, 0.5, device_stage=True) == want


def test_groups_from_search_apc(tmp_path):
    """one process from the FASTA file to the groups of `-a apc` == apc() on the lines orthology_from_search() returns (find_hit, then
    find_orth, then find_cluster -a apc, in-process on the same file); the existing keys of the timing dict stay"""
    from swiftortho_amd import find_cluster as fc, pipeline, synthprot
    p = str(tmp_path / "x.fsa")
    open(p, "wb").write(synthprot.synthprot(600, 200, 61))
    lines, _ = pipeline.orthology_from_search(p, **SEARCH_KW)
    assert len(lines) > 100
    want = fc.apc(b"".join(l + b"\n" for l in lines), 0.9)
    groups, t = pipeline.groups_from_search(p, algorithm="apc", damp=0.9, **SEARCH_KW)
    assert groups == want
    assert {"load", "search", "orth_relations", "cluster", "rows", "relations", "groups"} <= set(t) and "write_sc" not in t and "write_orth" not in t
    assert t["groups"] == len(want) and t["relations"] == len(lines)
    assert sum(1 for g in want if len(g) > 1) > 1
    assert pipeline.groups_from_search(p, algorithm="apc", device_stage=False, **SEARCH_KW)[0] == fc.apc(b"".join(l + b"\n" for l in lines), 0.5)
    assert sorted(os.listdir(str(tmp_path))) == ["x.fsa"]
