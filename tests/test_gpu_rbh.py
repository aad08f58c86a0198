"""Reciprocal best hits and the core-gene table on the GPU (csrc/rbh.hip, include/sohit.h so_rbh_*) against the REAL reference scripts'
goldens (tests/golden/rbh_*.json) and against the numpy definitions (swiftortho_amd/rbh.py) on seeded random tables: ids, order and
counts are exact.  Both tiers of the winner stage (SOHIT_RBH_TIER) with device memory poisoned, so_hit records uploaded with torch and
the records a real search leaves in HBM, both scripts with -G T, and pipeline.core_genes_from_search against the script chain.

Run on the GPU box:  python -m pytest tests/test_gpu_rbh.py -m gpu -q
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import orth_inputs as oi
import rbh_inputs as ri
from conftest import ROOT
from test_rbh import _call, _cols, _groups, run_rbh2phy

pytestmark = pytest.mark.gpu

TIERS = ("auto", "wave", "long", "sort")


@pytest.fixture(scope="module")
def rbh():
    from swiftortho_amd import rbh
    return rbh


def same_table(got, want):
    return (got.slots == want.slots and got.reference == want.reference and got.genes.tolist() == want.genes.tolist()
            and got.fwd.shape == want.fwd.shape and got.fwd.tolist() == want.fwd.tolist() and got.rec.tolist() == want.rec.tolist())


@functools.lru_cache(maxsize=None)
def random_case(seed):
    """(columns, fasta, numpy pairs, {-r value: numpy table}) of a seeded random table: computed once, shared, left unchanged"""
    from swiftortho_amd import find_orth, rbh
    sc, fasta = ri.random_columns(seed)
    cols = find_orth.columns_from_text(sc)
    refs = ("", rbh.fasta_taxa(fasta)[1].decode())
    return cols, fasta, rbh.reciprocal_best_hits(cols), {r: rbh.core_table(cols, fasta, r) for r in refs}


def check_against_numpy(rbh, cols, fasta, want_pairs, want_tables):
    a, b = rbh.device_reciprocal_best_hits(cols)
    assert a.tolist() == want_pairs[0].tolist() and b.tolist() == want_pairs[1].tolist()
    stats = None
    for ref, want in want_tables.items():
        got = rbh.device_core_table(cols, fasta, ref)
        assert same_table(got, want), ref
        assert got.pairs[0].tolist() == a.tolist() and got.pairs[1].tolist() == b.tolist()     # the pairs of the same call
        stats = got.stats
    return stats


@pytest.mark.parametrize("name", ri.golden_names())
def test_goldens_through_the_device(rbh, name):
    sc, fasta, meta = ri.golden(name)
    cols = _cols(name)
    a, b = rbh.device_reciprocal_best_hits(cols)
    assert rbh.rbh_lines(cols.names, a, b) == meta["pairs"].encode()
    for ref in meta["raises"]:
        with pytest.raises(ValueError) as e:
            rbh.device_core_table(cols, fasta, ref)
        assert "not among the taxa of the FASTA" in str(e.value)
    for ref, want in meta["groups"].items():
        table = rbh.device_core_table(cols, fasta, ref)
        assert _groups(rbh, cols, table) == want, ref
        assert same_table(table, rbh.core_table(cols, fasta, ref)), ref
        assert rbh.rbh_lines(cols.names, *table.pairs) == meta["pairs"].encode()


@pytest.mark.parametrize("name", [n for n in ri.golden_names() if n != "edge_nan"])
@pytest.mark.parametrize("tier", TIERS)
def test_forced_tiers_on_the_goldens(rbh, monkeypatch, tier, name):
    """every run through the named tier (the switch is read per call), device memory poisoned: the same pairs and tables.  `wave` adds
    nothing to `auto` (the wave tier already takes every run it can hold); `long` and `sort` are two spellings of the sorted tier"""
    monkeypatch.setenv("SOHIT_RBH_TIER", tier)
    monkeypatch.setenv("SOHIT_POISON", "165")
    sc, fasta, meta = ri.golden(name)
    cols = _cols(name)
    refs = [r for r in meta["groups"]]
    a, b = rbh.device_reciprocal_best_hits(cols)
    assert rbh.rbh_lines(cols.names, a, b) == meta["pairs"].encode()
    for ref in refs:
        table = rbh.device_core_table(cols, fasta, ref)
        assert _groups(rbh, cols, table) == meta["groups"][ref], ref
        q = np.asarray(cols.q)
        lens = np.diff(np.flatnonzero(np.concatenate([[True], q[1:] != q[:-1], [True]]))) if len(q) else np.zeros(0, dtype=np.int64)
        long_runs = lens if tier in ("long", "sort") else lens[lens > ri.WAVE_ROWS]
        if len(q):
            assert table.stats["n_runs"] == len(lens) and table.stats["n_runs_long"] == len(long_runs) and table.stats["n_rows_long"] == int(long_runs.sum())


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("tier", ("auto", "long"))
def test_random_tables(rbh, monkeypatch, tier, seed):
    monkeypatch.setenv("SOHIT_RBH_TIER", tier)
    monkeypatch.setenv("SOHIT_POISON", "90")
    cols, fasta, pairs, tables = random_case(seed)
    assert len(pairs[0]) > 20 and all(len(t.genes) > 3 for t in tables.values())
    stats = check_against_numpy(rbh, cols, fasta, pairs, tables)
    assert 0 < stats["n_runs_long"] <= stats["n_runs"] and stats["n_winners"] > 0 and stats["waits"] > 0


@pytest.mark.parametrize("shape", ri.RUN_SHAPES)
@pytest.mark.parametrize("n", ri.RUN_SIZES)
def test_run_shapes(rbh, monkeypatch, n, shape):
    """run heads, scans and run starts at their edges (a workgroup of 256 rows, a scan tile of 8192 values, the single-launch scan's
    32768): every row a run, one run of all rows (the sorted tier), heads exactly on 255 .. 257, 8191 .. 8193, 32767 and 32768 --
    pairs, tables and the run count against the numpy definitions, device memory poisoned"""
    monkeypatch.setenv("SOHIT_POISON", "165")
    cols, fasta, starts, pairs, tables = ri.run_shape_case(n, shape)
    stats = check_against_numpy(rbh, cols, fasta, pairs, tables)
    assert stats["n_runs"] == len(starts)
    if shape == "one" and n > ri.WAVE_ROWS:
        assert stats["n_runs_long"] == 1 and stats["n_rows_long"] == n


def _upload(rec):
    import torch
    return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()


@pytest.mark.parametrize("tier", ("auto", "long"))
def test_records_path(rbh, monkeypatch, tier):
    """so_hit records on the device (uploaded with torch): id lists in another order than the names, ids that occur twice in the query
    list (two ordinals, one code: their neighbouring runs merge)"""
    from swiftortho_amd import find_orth
    monkeypatch.setenv("SOHIT_RBH_TIER", tier)
    cols0, fasta, _, _ = random_case(0)
    rec, qids, sids = oi.records_from_columns(cols0)
    cols = find_orth.columns_from_records(rec, qids, sids)
    want = rbh.reciprocal_best_hits(cols)
    assert len(want[0]) > 20
    names, a, b = rbh.device_reciprocal_best_hits_from_records(_upload(rec), qids, sids)
    assert names.tolist() == cols.names.tolist() and a.tolist() == want[0].tolist() and b.tolist() == want[1].tolist()
    for ref in ("", rbh.fasta_taxa(fasta)[2].decode()):
        names, table = rbh.device_core_table_from_records(_upload(rec), qids, sids, fasta, ref)
        assert same_table(table, rbh.core_table(cols, fasta, ref)) and len(table.genes) > 3
        assert table.pairs[0].tolist() == want[0].tolist()


def test_records_path_edges(rbh):
    import torch
    cols0, fasta, _, _ = random_case(0)
    rec, qids, sids = oi.records_from_columns(cols0)
    names, a, b = rbh.device_reciprocal_best_hits_from_records(torch.zeros(0, dtype=torch.uint8, device="cuda"), qids, sids)
    assert len(a) == 0 and len(b) == 0
    with pytest.raises(TypeError):
        rbh.device_reciprocal_best_hits_from_records(torch.zeros(80, dtype=torch.uint8), qids, sids)
    with pytest.raises(ValueError):
        rbh.device_reciprocal_best_hits_from_records(torch.zeros(81, dtype=torch.uint8, device="cuda"), qids, sids)
    for field in ("qidx", "sidx"):
        for v in (-1, len(qids) + 5):
            r2 = rec.copy()
            r2[field][len(r2) // 2] = v
            with pytest.raises(RuntimeError) as e:
                rbh.device_reciprocal_best_hits_from_records(_upload(r2), qids, sids)
            assert field in str(e.value) and "outside" in str(e.value)


def test_refusals(rbh):
    import torch
    from swiftortho_amd import _lib
    L = _lib.load()
    assert _call(L, _lib) == (0, "")
    rc, msg = _call(L, _lib, q=(0,), s=(2,))
    assert rc != 0 and "name code" in msg
    rc, msg = _call(L, _lib, q=(-1,), s=(1,))
    assert rc != 0 and "name code" in msg
    rc, msg = _call(L, _lib, n=1 << 31)
    assert rc != 0 and "2^31 rows" in msg
    assert _call(L, _lib) == (0, "")             # a refusal leaves nothing behind
    # a device that is not there
    q, s, sco, tax = np.zeros(1, dtype=np.int32), np.ones(1, dtype=np.int32), np.ones(1), np.array([0, 1], dtype=np.int32)
    out = _lib.SoRbhResult()
    assert L.so_rbh_cols(torch.cuda.device_count(), 1, q.ctypes.data, s.ctypes.data, sco.ctypes.data, 2, tax.ctypes.data, 2, -1, 0, C.byref(out)) != 0
    assert "device" in L.so_rbh_last_error().decode()
    # n = 0 is served: empty arrays that the free function releases
    assert L.so_rbh_cols(0, 0, None, None, None, 0, None, 0, -1, 0, C.byref(out)) == 0 and out.n_rbh == 0 and out.n_core == 0 and out.waits == 0
    L.so_rbh_free(C.byref(out))
    # a NULL record pointer with rows to read
    assert L.so_rbh_records(0, None, 1, q.ctypes.data, 1, s.ctypes.data, 1, 2, tax.ctypes.data, 2, -1, 0, C.byref(out)) != 0
    assert "NULL" in L.so_rbh_last_error().decode()


def test_nan_is_refused_by_the_call_and_served_by_the_literal_loop(rbh, monkeypatch):
    from swiftortho_amd import _lib
    L = _lib.load()
    sc, fasta, meta = ri.golden("edge_nan")
    cols = _cols("edge_nan")
    tax, taxa = rbh.name_taxa(cols.names)
    head, keep = rbh._cols_head(cols, 0)
    with pytest.raises(RuntimeError) as e:
        rbh._rbh_call("cols", head, len(cols.names), tax, len(taxa), -1)
    assert "NaN" in str(e.value)
    calls = []
    literal = rbh._literal_winners
    monkeypatch.setattr(rbh, "_literal_winners", lambda *a: calls.append(a[2]) or literal(*a))
    a, b = rbh.device_reciprocal_best_hits(cols)
    assert rbh.rbh_lines(cols.names, a, b) == meta["pairs"].encode() and calls == [False]
    table = rbh.device_core_table(cols, fasta, "b")
    assert _groups(rbh, cols, table) == meta["groups"]["b"] and rbh.rbh_lines(cols.names, *table.pairs) == meta["pairs"].encode()


@pytest.mark.parametrize("name", ["taxa5", "taxa12", "edge_runs", "edge_ties", "edge_pairs"])
def test_script_get_rbh_G_T(tmp_path, name):
    sc, _, meta = ri.golden(name)
    p = str(tmp_path / "in.sc")
    open(p, "wb").write(sc)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "get_rbh.py"), p, "-G", "T"], capture_output=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == meta["pairs"].encode()


@pytest.mark.parametrize("name,ref", [("taxa5", ""), ("taxa12", "tx06"), ("edge_core", ""), ("edge_taxa", ""), ("edge_absent_taxon", "")])
def test_script_rbh2phy_G_T(tmp_path, name, ref):
    meta = ri.golden(name)[2]
    r, groups, files = run_rbh2phy(tmp_path, name, ref, extra=("-G", "T"))
    if ref in meta["raises"]:
        assert r.returncode != 0 and b"not among the taxa of the FASTA" in r.stderr
        return
    assert r.returncode == 0, r.stderr[-2000:]
    assert groups == files == meta["groups"][ref]


SEARCH_KW = dict(ssd="111111", nr="AST,CFILMVY,DN,EQ,G,H,KR,P,W", ht=12000017, chk=50000, step=1, v=500, expect=1e-5, flt="T")


def test_real_search_records_and_pipeline(rbh, tmp_path):
    """search_device() -> so_rbh_records on the records where they lie == the numpy definition on the same records downloaded; and
    pipeline.core_genes_from_search == scripts/get_rbh.py + scripts/rbh2phy.py on the .sc file it wrote"""
    from swiftortho_amd import find_orth, fsearch, pipeline, synthprot
    fa = synthprot.synthprot(600, 200, 61)   # (two taxa; 999 rows by the CPU oracle's search)
    ids = find_orth.fasta_ids(fa)
    s = fsearch.Searcher(**SEARCH_KW)
    try:
        s.load_ref_bytes(fa)
        s.load_queries_bytes(fa)
        dev = s.search_device()
        from swiftortho_amd import _lib
        rec = np.frombuffer(dev.tensor().cpu().numpy().tobytes(), dtype=np.dtype(_lib.SoHit))
        assert len(rec) == len(dev) > len(ids)
        cols = find_orth.columns_from_records(rec, ids, ids)
        want = rbh.reciprocal_best_hits(cols)
        assert len(want[0]) > 20
        names, table = rbh.device_core_table_from_records(dev, ids, ids, fa)
        assert names.tolist() == cols.names.tolist() and same_table(table, rbh.core_table(cols, fa)) and len(table.genes) > 20
        assert table.pairs[0].tolist() == want[0].tolist() and table.pairs[1].tolist() == want[1].tolist()
        names, a, b = rbh.device_reciprocal_best_hits_from_records(dev.tensor(), ids, ids)       # a copy of the records in a torch tensor
        assert a.tolist() == want[0].tolist() and b.tolist() == want[1].tolist()
    finally:
        s.close()
    p, sc, o = str(tmp_path / "x.fsa"), str(tmp_path / "x.sc"), str(tmp_path / "g.tsv")
    open(p, "wb").write(fa)
    pairs, groups, t = pipeline.core_genes_from_search(p, sc_path=sc, **SEARCH_KW)
    assert t["rows"] == len(rec) and t["pairs"] == len(pairs) == len(want[0]) and "rbh" in t and "write_sc" in t
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "get_rbh.py"), sc], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"".join(x + b"\t" + y + b"\n" for x, y in pairs)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "rbh2phy.py"), "-i", sc, "-f", p, "-o", o], capture_output=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(o, "rb").read() == b"".join(b"\t".join(g) + b"\n" for g in groups) and len(groups) > 20
    # collapse=True: duplicates searched once, the records multiplied back on the device -- held to the script on the file of THAT route
    sc2 = str(tmp_path / "y.sc")
    pairs2, groups2, t2 = pipeline.core_genes_from_search(p, collapse=True, sc_path=sc2, **SEARCH_KW)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "get_rbh.py"), sc2], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"".join(x + b"\t" + y + b"\n" for x, y in pairs2) and len(pairs2) > 20
    assert {"collapse", "expand", "rows_collapsed"} <= set(t2) and len(groups2) > 20
