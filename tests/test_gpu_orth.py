"""The candidate stage of find_orth on the GPU (csrc/orth.hip, include/sohit.h so_orth_*) against the numpy stage it restates
(find_orth.candidates): every table equal, float64 values bit for bit.  Inputs: the 16 goldens of the reference script, the generator
of tests/orth_inputs.py (whose guarantees tests/test_orth_candidates.py asserts: every tier bound of csrc/tune.h from both sides,
repeated subjects, second runs, key groups of 1 .. 4 members, the last-pair rule both ways), hand-made edge inputs, so_hit records
uploaded with torch and the records a real search leaves in HBM.

Run on the GPU box:  python -m pytest tests/test_gpu_orth.py -m gpu -q
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import orth_inputs as oi
from conftest import GOLD, ROOT, orth_golden_cases
from test_orth_candidates import _golden, generated

pytestmark = pytest.mark.gpu

TIERS = ("auto", "wave", "lds", "scratch")


@pytest.fixture(scope="module")
def fo():
    from swiftortho_amd import find_orth
    return find_orth


@functools.lru_cache(maxsize=None)
def numpy_stage(seed, flags):
    from swiftortho_amd import find_orth
    return find_orth.candidates(generated(seed), *oi.FLAG_SETS[flags])


@pytest.mark.parametrize("name,variant", orth_golden_cases())
def test_goldens_through_the_device(fo, name, variant):
    cols, flags, want = _golden(name, variant)
    got = fo.device_candidates(cols, *flags)
    assert oi.same_candidates(got, fo.candidates(cols, *flags)) == ""
    assert fo.relations(cols, *flags, candidates=fo.device_candidates) == want


@pytest.mark.parametrize("name", sorted(set(n for n, _ in orth_golden_cases())))
def test_cli_flag_G(name):
    """bin/find_orth.py -G T prints the reference script's bytes"""
    variant = [v for n, v in orth_golden_cases() if n == name][-1]
    from test_find_orth import _load
    meta, sc = _load(name)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "find_orth.py"), "-i", sc, "-G", "T"] + meta["variants"][variant], capture_output=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == open(os.path.join(GOLD, "orth_%s.%s.orth" % (name, variant)), "rb").read()


@pytest.mark.parametrize("flags", sorted(oi.FLAG_SETS))
@pytest.mark.parametrize("tier", TIERS)
def test_forced_tiers(fo, monkeypatch, tier, flags):
    """every run through the named tier wherever that tier can take it (the switch is read per call): the same tables whatever the tier, with
    device memory poisoned so that nothing rests on what an allocation held before.  The `wave` rows add nothing to the `auto` rows: the
    wave tier already takes every run it can hold, so forcing it changes no run's tier; they only show that the spelling is accepted."""
    monkeypatch.setenv("SOHIT_ORTH_TIER", tier)
    monkeypatch.setenv("SOHIT_POISON", "165")
    for seed in (0, 2):   # (the last-pair rule: met by both lists of seed 0, by neither of seed 2)
        got = fo.device_candidates(generated(seed), *oi.FLAG_SETS[flags])
        assert oi.same_candidates(got, numpy_stage(seed, flags)) == "", (seed, tier, flags)


def test_second_seed_default_tiers(fo):
    got = fo.device_candidates(generated(1), *oi.FLAG_SETS["no"])
    assert oi.same_candidates(got, numpy_stage(1, "no")) == ""


@pytest.mark.parametrize("n_taxa", [oi.ORTH_LDS_TAXA - 1, oi.ORTH_LDS_TAXA, oi.ORTH_LDS_TAXA + 1])
@pytest.mark.parametrize("tier", ("auto", "lds", "scratch"))
def test_taxa_bound_of_the_lds_tier(fo, monkeypatch, tier, n_taxa):
    """one taxon more than the per-taxon LDS table holds sends the long runs to global scratch"""
    monkeypatch.setenv("SOHIT_ORTH_TIER", tier)
    cols = oi.many_taxa(n_taxa)
    assert oi.same_candidates(fo.device_candidates(cols, .5, 0., "no"), fo.candidates(cols, .5, 0., "no")) == ""


@pytest.mark.parametrize("case", sorted(oi.edge_inputs()))
@pytest.mark.parametrize("tier", ("auto", "scratch"))
def test_edge_inputs_through_the_device(fo, monkeypatch, tier, case):
    monkeypatch.setenv("SOHIT_ORTH_TIER", tier)
    cols = oi.edge_inputs()[case]
    for flags in oi.FLAG_SETS.values():
        got = fo.device_candidates(cols, *flags)
        assert oi.same_candidates(got, fo.candidates(cols, *flags)) == "", flags
        assert fo.relations(cols, *flags, candidates=fo.device_candidates) == fo.relations(cols, *flags)


def _upload(rec):
    import torch
    return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()


@pytest.mark.parametrize("flags", sorted(oi.FLAG_SETS))
def test_records_path(fo, flags):
    """so_hit records on the device (uploaded with torch): identities with more than two decimals, id lists in another order than the names,
    ids that occur twice in the query list (two ordinals, one code: their neighbouring runs merge)"""
    rec, qids, sids = oi.records_from_columns(generated(0))
    cols = fo.columns_from_records(rec, qids, sids)
    assert len(set(qids)) < len(qids) and len(np.unique(cols.idy)) >= 5
    want = fo.candidates(cols, *oi.FLAG_SETS[flags])
    assert want.n_runs < len(np.flatnonzero(np.diff(rec["qidx"]))) + 1          # runs of two ordinals did merge
    got = fo.device_candidates_from_records(_upload(rec), qids, sids, *oi.FLAG_SETS[flags])
    assert oi.same_candidates(got, want) == ""
    assert fo.relations_from_device(_upload(rec), qids, sids, *oi.FLAG_SETS[flags]) == fo.relations_from_records(rec, qids, sids, *oi.FLAG_SETS[flags])


def test_records_path_no_records(fo):
    import torch
    rec, qids, sids = oi.records_from_columns(generated(0))
    got = fo.device_candidates_from_records(torch.zeros(0, dtype=torch.uint8, device="cuda"), qids, sids)
    assert oi.same_candidates(got, fo.Candidates.empty()) == ""
    assert fo.relations_from_device(torch.zeros(0, dtype=torch.uint8, device="cuda"), qids, sids) == []
    with pytest.raises(TypeError):
        fo.device_candidates_from_records(torch.zeros(80, dtype=torch.uint8), qids, sids)
    with pytest.raises(ValueError):
        fo.device_candidates_from_records(torch.zeros(81, dtype=torch.uint8, device="cuda"), qids, sids)


SEARCH_KW = dict(ssd="111111", nr="AST,CFILMVY,DN,EQ,G,H,KR,P,W", ht=12000017, chk=50000, step=1, v=500, expect=1e-5, flt="T")


def test_real_search_records_stay_on_the_device(fo, tmp_path):
    """search_device() -> relations_from_device() == search() -> relations_from_records(), line for line; the searcher's next search finds
    its rows unchanged (the stage only reads the records)"""
    from swiftortho_amd import fsearch, pipeline, synthprot
    fa = synthprot.synthprot(600, 200, 61)   # (999 rows and 176 relations of all three kinds by the CPU oracle's search)
    ids = fo.fasta_ids(fa)
    s = fsearch.Searcher(**SEARCH_KW)
    try:
        s.load_ref_bytes(fa)
        s.load_queries_bytes(fa)
        hits = s.search()
        rec = hits.array()
        rows = b"".join(hits.rows())
        hits.close()
        assert len(rec) > len(ids)
        for flags in oi.FLAG_SETS.values():
            want = fo.relations_from_records(rec, ids, ids, *flags)
            assert len(want) > 50 and all(any(l.startswith(k) for l in want) for k in (b"IP", b"OT", b"CO"))
            dev = s.search_device()
            assert len(dev) == len(rec) and dev.device_pointer() != 0
            assert fo.relations_from_device(dev, ids, ids, *flags) == want
            assert oi.same_candidates(fo.device_candidates_from_records(dev, ids, ids, *flags), fo.candidates(fo.columns_from_records(rec, ids, ids), *flags)) == ""
            assert fo.relations_from_device(dev.tensor(), ids, ids, *flags) == want   # a copy of the records in a torch tensor
        hits = s.search()
        assert b"".join(hits.rows()) == rows
        hits.close()
    finally:
        s.close()
    p, sc0, sc1 = str(tmp_path / "x.fsa"), str(tmp_path / "a.sc"), str(tmp_path / "b.sc")
    open(p, "wb").write(fa)
    l0, t0 = pipeline.orthology_from_search(p, sc_path=sc0, **SEARCH_KW)
    l1, t1 = pipeline.orthology_from_search(p, sc_path=sc1, device_stage=True, **SEARCH_KW)
    l2, t2 = pipeline.orthology_from_search(p, device_stage=True, norm="bsr", **SEARCH_KW)
    assert l1 == l0 == fo.relations_from_records(rec, ids, ids) and t1["rows"] == t0["rows"] == len(rec)
    assert open(sc0, "rb").read() == open(sc1, "rb").read() == rows
    assert "orth_candidates" in t1 and "orth_candidates" not in t0 and "write_sc" not in t2
    assert l2 == fo.relations_from_records(rec, ids, ids, norm="bsr")


def _cols_call(cols, n_names=None, tax=None, n_taxa=None, n=None, device=0):
    """so_orth_candidates_cols with arguments the Python wrapper would never pass -> (return code, message)"""
    from swiftortho_amd import _lib, find_orth
    L = _lib.load()
    t, taxa = find_orth._taxa(cols.names, "|")
    tax = np.ascontiguousarray(t if tax is None else tax, dtype=np.int32)
    q, s = np.ascontiguousarray(cols.q, dtype=np.int32), np.ascontiguousarray(cols.s, dtype=np.int32)
    f = [np.ascontiguousarray(getattr(cols, k), dtype=np.float64) for k in ("idy", "aln", "qst", "qed", "score", "qlen")]
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    out = _lib.SoOrthCand()
    rc = L.so_orth_candidates_cols(device, len(q) if n is None else n, ptr(q), ptr(s), *[ptr(a) for a in f], len(cols.names) if n_names is None else n_names, ptr(tax),
                                   len(taxa) if n_taxa is None else n_taxa, .5, 0., 0, C.byref(out))
    msg = L.so_orth_last_error().decode()
    if rc == 0:
        L.so_orth_free(C.byref(out))
    return rc, msg


def test_refusals(fo):
    import torch
    from swiftortho_amd import _lib
    cols = oi.edge_inputs()["last_pair"]
    assert _cols_call(cols) == (0, "")
    rc, msg = _cols_call(cols, n=1 << 31)
    assert rc != 0 and "2^31 rows" in msg
    rc, msg = _cols_call(cols, n_names=3037000500)
    assert rc != 0 and "2^63" in msg
    rc, msg = _cols_call(cols, n_names=5)          # the codes run to 5
    assert rc != 0 and "name code" in msg
    bad = oi.columns([b"a|1", b"b|1"], [(b"a|1", b"b|1", 90., 100., 1., 100., 50., 100.)])
    bad.q = np.array([-1], dtype=np.int64)
    rc, msg = _cols_call(bad)
    assert rc != 0 and "name code" in msg
    rc, msg = _cols_call(cols, tax=np.array([0, 0, 0, 1, 1, 7]))
    assert rc != 0 and "taxon" in msg
    rc, msg = _cols_call(cols, device=torch.cuda.device_count())
    assert rc != 0 and "device" in msg
    assert _cols_call(cols) == (0, "")             # a refusal leaves nothing behind
    # records: an ordinal outside its map
    rec, qids, sids = oi.records_from_columns(oi.many_taxa(64), n_dup=2)
    for field, word in (("qidx", "qidx"), ("sidx", "sidx")):
        for v in (-1, len(qids) + 5):
            r2 = rec.copy()
            r2[field][len(r2) // 2] = v
            with pytest.raises(RuntimeError) as e:
                fo.device_candidates_from_records(_upload(r2), qids, sids)
            assert word in str(e.value) and "outside" in str(e.value)
    got = fo.device_candidates_from_records(_upload(rec), qids, sids)
    assert oi.same_candidates(got, fo.candidates(fo.columns_from_records(rec, qids, sids))) == ""
    # a NULL record pointer with rows to read
    L = _lib.load()
    out = _lib.SoOrthCand()
    z = np.zeros(4, dtype=np.int32)
    assert L.so_orth_candidates_records(0, None, 3, C.c_void_p(z.ctypes.data), 4, C.c_void_p(z.ctypes.data), 4, 1, C.c_void_p(z.ctypes.data), 1, .5, 0., 0, C.byref(out)) != 0
    assert "NULL" in L.so_orth_last_error().decode()
