"""The relations stage of find_orth on the GPU (csrc/orth.hip, include/sohit.h so_orth_relations_*) against the numpy stage it restates
(find_orth.relation_tables): every table equal, float64 values bit for bit.  Inputs: the 16 goldens of the reference script, the generator
of tests/orth_inputs.py, the clique family and the edge inputs of tests/orth_rel_inputs.py (whose guarantees tests/test_orth_relations.py
asserts), so_hit records uploaded with torch and the records a real search leaves in HBM.

Run on the GPU box:  python -m pytest tests/test_gpu_orth_relations.py -m gpu -q
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import orth_inputs as oi
import orth_rel_inputs as ri
from conftest import GOLD, ROOT, orth_golden_cases
from test_orth_candidates import _golden, generated

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fo():
    from swiftortho_amd import find_orth
    return find_orth


@functools.lru_cache(maxsize=None)
def numpy_generated(seed, flags):
    return ri.numpy_tables(generated(seed), *oi.FLAG_SETS[flags])


@functools.lru_cache(maxsize=None)
def numpy_clique(k, flags):
    cols = ri.clique(k)
    return cols, ri.numpy_tables(cols, *ri.FLAGS[flags])


@pytest.mark.parametrize("name,variant", orth_golden_cases())
def test_goldens_through_the_device(fo, name, variant):
    cols, flags, want = _golden(name, variant)
    got = fo.device_relation_tables(cols, *flags)
    assert ri.same_tables(got, ri.numpy_tables(cols, *flags)) == ""
    assert fo.lines_from_tables(cols.names, got) == want


@pytest.mark.parametrize("name,variant", orth_golden_cases())
def test_cli_flag_G_R(name, variant):
    """bin/find_orth.py -G R prints the reference script's bytes"""
    from test_find_orth import _load
    meta, sc = _load(name)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "find_orth.py"), "-i", sc, "-G", "R"] + meta["variants"][variant], capture_output=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == open(os.path.join(GOLD, "orth_%s.%s.orth" % (name, variant)), "rb").read()


@pytest.mark.parametrize("seed,flags", [(0, f) for f in sorted(oi.FLAG_SETS)] + [(1, "no")])
def test_generated_inputs(fo, seed, flags):
    got = fo.device_relation_tables(generated(seed), *oi.FLAG_SETS[flags])
    assert ri.same_tables(got, numpy_generated(seed, flags)) == ""
    assert len(got.ip_a) > 50 and len(got.ot_a) > 2000 and len(got.co_a) > 100      # (every section is there: 53 / 2629 / 107 rows at the least)


@pytest.mark.parametrize("poison", ("255", "90"))
@pytest.mark.parametrize("flags", sorted(ri.FLAGS))
@pytest.mark.parametrize("k", ri.CLIQUE_KS + ri.BOUND_KS)
def test_clique_inputs(fo, monkeypatch, k, flags, poison):
    """surviving and dropped repeats, k occurrences of a pair in a block, k * k products per ortholog pair, groups of 63 / 64 / 65 rows and of
    thousands, taxon codes that do not ascend with the names, a zero normaliser -- with device memory poisoned (0xFF, 0x5A), so that nothing
    rests on what an allocation held before"""
    monkeypatch.setenv("SOHIT_POISON", poison)
    cols, want = numpy_clique(k, flags)
    got = fo.device_relation_tables(cols, *ri.FLAGS[flags])
    assert ri.same_tables(got, want) == ""
    assert len(got.co_a) == 3 * k * (k - 1) + 2


@functools.lru_cache(maxsize=None)
def kept_edges_case(flags):
    from swiftortho_amd import find_orth
    cols = oi.kept_edges()
    return cols, find_orth.candidates(cols, *oi.FLAG_SETS[flags]), ri.numpy_tables(cols, *oi.FLAG_SETS[flags])


@pytest.mark.parametrize("flags", ("no", "bsr"))
def test_kept_row_edges(fo, monkeypatch, flags):
    """more than 32768 kept rows with a dropped row directly before and after kept rows 256, 8192 and 32768 (tests/orth_inputs.py
    kept_edges; tests/test_orth_relations.py asserts that it holds them): the compaction offsets and the run heads of the kept rows on a
    workgroup's, a scan tile's and the single-launch scan's edge -- candidates and relation tables against the numpy stage, poisoned"""
    monkeypatch.setenv("SOHIT_POISON", "165")
    cols, want_cand, want = kept_edges_case(flags)
    assert oi.same_candidates(fo.device_candidates(cols, *oi.FLAG_SETS[flags]), want_cand) == ""
    assert ri.same_tables(fo.device_relation_tables(cols, *oi.FLAG_SETS[flags]), want) == ""


def _edge_cases():
    both = dict(oi.edge_inputs())
    both.update(ri.edge_inputs())
    return both


@pytest.mark.parametrize("case", sorted(_edge_cases()))
def test_edge_inputs_through_the_device(fo, case):
    cols = _edge_cases()[case]
    for flags in oi.FLAG_SETS.values():
        cand = fo.candidates(cols, *flags)
        if np.isnan(cand.ip_s).any() or np.isnan(cand.ot_s).any() or np.isnan(cand.co_best).any():
            continue                                                                # (0 / 0 under bsr: outside what the stage defines)
        got = fo.device_relation_tables(cols, *flags)
        assert ri.same_tables(got, ri.numpy_tables(cols, *flags)) == "", flags
        assert fo.lines_from_tables(cols.names, got) == fo.relations(cols, *flags)


def _upload(rec):
    import torch
    return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()


@pytest.mark.parametrize("flags", sorted(oi.FLAG_SETS))
def test_records_path(fo, flags):
    """so_hit records on the device (uploaded with torch) give what the columns they stand for give"""
    rec, qids, sids = oi.records_from_columns(generated(0))
    cols = fo.columns_from_records(rec, qids, sids)
    want = fo.device_relation_tables(cols, *oi.FLAG_SETS[flags])
    names, got = fo.device_relation_tables_from_records(_upload(rec), qids, sids, *oi.FLAG_SETS[flags])
    assert ri.same_tables(got, want) == "" and ri.same_tables(got, ri.numpy_tables(cols, *oi.FLAG_SETS[flags])) == ""
    assert np.array_equal(names, cols.names)
    lines = fo.relations_from_device(_upload(rec), qids, sids, *oi.FLAG_SETS[flags], stage="relations")
    assert lines == fo.relations_from_records(rec, qids, sids, *oi.FLAG_SETS[flags]) and len(lines) > 1000


def test_records_path_no_records(fo):
    import torch
    rec, qids, sids = oi.records_from_columns(generated(0))
    none = torch.zeros(0, dtype=torch.uint8, device="cuda")
    names, got = fo.device_relation_tables_from_records(none, qids, sids)
    assert ri.same_tables(got, fo.RelationTables.empty()) == ""
    assert fo.relations_from_device(none, qids, sids, stage="relations") == []
    with pytest.raises(ValueError):
        fo.relations_from_device(none, qids, sids, stage="text")


SEARCH_KW = dict(ssd="111111", nr="AST,CFILMVY,DN,EQ,G,H,KR,P,W", ht=12000017, chk=50000, step=1, v=500, expect=1e-5, flt="T")


def test_real_search_relations_on_the_device(tmp_path):
    """orthology_from_search(device_stage='relations') == device_stage=False, line for line, on the proteome test_gpu_orth.py searches"""
    from swiftortho_amd import pipeline, synthprot
    fa = synthprot.synthprot(600, 200, 61)
    p = str(tmp_path / "x.fsa")
    open(p, "wb").write(fa)
    l0, t0 = pipeline.orthology_from_search(p, **SEARCH_KW)
    l1, t1 = pipeline.orthology_from_search(p, device_stage="relations", **SEARCH_KW)
    assert l1 == l0 and len(l0) > 50 and all(any(l.startswith(k) for l in l0) for k in (b"IP", b"OT", b"CO"))
    assert t1["rows"] == t0["rows"] and "orth_relations" in t1 and "orth_candidates" not in t1 and "orth_relations" not in t0


def _cols_call(cols, n_names=None, tax=None, n_taxa=None, n=None, device=0):
    """so_orth_relations_cols with arguments the Python wrapper would never pass -> (return code, message)"""
    from swiftortho_amd import _lib, find_orth
    L = _lib.load()
    t, taxa = find_orth._taxa(cols.names, "|")
    tax = np.ascontiguousarray(t if tax is None else tax, dtype=np.int32)
    q, s = np.ascontiguousarray(cols.q, dtype=np.int32), np.ascontiguousarray(cols.s, dtype=np.int32)
    f = [np.ascontiguousarray(getattr(cols, k), dtype=np.float64) for k in ("idy", "aln", "qst", "qed", "score", "qlen")]
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    out = _lib.SoOrthRel()
    rc = L.so_orth_relations_cols(device, len(q) if n is None else n, ptr(q), ptr(s), *[ptr(a) for a in f], len(cols.names) if n_names is None else n_names, ptr(tax),
                                  len(taxa) if n_taxa is None else n_taxa, .5, 0., 0, C.byref(out))
    msg = L.so_orth_last_error().decode()
    if rc == 0:
        L.so_orth_rel_free(C.byref(out))
    return rc, msg


def test_refusals(fo):
    """what the candidates calls refuse, the relations calls refuse, through so_orth_last_error"""
    import torch
    from swiftortho_amd import _lib
    cols = oi.edge_inputs()["last_pair"]
    assert _cols_call(cols) == (0, "")
    for kw, word in ((dict(n=1 << 31), "2^31 rows"), (dict(n_names=3037000500), "2^63"), (dict(n_names=5), "name code"),
                     (dict(tax=np.array([0, 0, 0, 1, 1, 7])), "taxon"), (dict(device=torch.cuda.device_count()), "device")):
        rc, msg = _cols_call(cols, **kw)
        assert rc != 0 and word in msg and msg.startswith("so_orth_relations_cols"), kw
    assert _cols_call(cols) == (0, "")             # a refusal leaves nothing behind
    rec, qids, sids = oi.records_from_columns(oi.many_taxa(64), n_dup=2)
    for field in ("qidx", "sidx"):
        for v in (-1, len(qids) + 5):
            r2 = rec.copy()
            r2[field][len(r2) // 2] = v
            with pytest.raises(RuntimeError) as e:
                fo.device_relation_tables_from_records(_upload(r2), qids, sids)
            assert field in str(e.value) and "outside" in str(e.value)
    L = _lib.load()
    out = _lib.SoOrthRel()
    z = np.zeros(4, dtype=np.int32)
    assert L.so_orth_relations_records(0, None, 3, C.c_void_p(z.ctypes.data), 4, C.c_void_p(z.ctypes.data), 4, 1, C.c_void_p(z.ctypes.data), 1, .5, 0., 0, C.byref(out)) != 0
    assert "NULL" in L.so_orth_last_error().decode()
    assert L.so_orth_relations_cols(0, 0, None, None, None, None, None, None, None, None, 0, None, 0, .5, 0., 0, None) != 0


def test_candidates_unchanged(fo):
    """the candidates call gives the same tables before and after a relations call"""
    cols = generated(0)
    before = fo.device_candidates(cols, *oi.FLAG_SETS["no"])
    fo.device_relation_tables(cols, *oi.FLAG_SETS["no"])
    after = fo.device_candidates(cols, *oi.FLAG_SETS["no"])
    assert oi.same_candidates(before, after) == "" and oi.same_candidates(after, fo.candidates(cols, *oi.FLAG_SETS["no"])) == ""
