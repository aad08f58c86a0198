"""The guarantees of tests/ungapq_inputs.py (the sets of tests/test_gpu_ungapq_edges.py), checked without a GPU: the model's per-query hit
counts are the oracle's own (its seed_hits for that query alone), every edge count is there at the protein built for it, and the
straddling seeds straddle."""
import numpy as np
import pytest

import ungapq_inputs as ui


def oracle_hits(oracle, path, q):
    r = oracle.blastp(path, path, "", ssd=ui.SEED, nr=oracle.AA9, ht=ui.HT, chk=50000, step=1, v=500, expect=1e-5, flt="T", thr=100000, st=q, ed=q + 1)
    return r.stats["seed_hits"]


def test_edge_set(oracle, tmp_path):
    fasta, model, roles = ui.edge_set(oracle)
    path = str(tmp_path / "e.fsa")
    open(path, "wb").write(fasta)
    got = model.hit_counts()
    assert 590 <= len(roles) <= 640 and fasta == ui.edge_set(oracle)[0]
    first = roles.index("edge:%d" % ui.EDGE_COUNTS[0])
    for i, c in enumerate(ui.EDGE_COUNTS):
        assert roles[first + i] == "edge:%d" % c and got[first + i] == c
    for q in (first + 1, first + 6, len(roles) - 1):
        assert got[q] == oracle_hits(oracle, path, q)
    for role in ("mosaic", "runs", "copies"):
        q = roles.index(role)
        assert got[q] == oracle_hits(oracle, path, q)
    assert all(got[q] > 1024 for q, r in enumerate(roles) if r == "copies")
    wh = model.window_hits()
    # the mosaic proteins' pieces: windows of two entries (the piece's source and the protein itself) with one-entry windows around them
    q = roles.index("mosaic")
    assert np.count_nonzero(wh[q] == 2) >= 15
    for e in (64, 128, 512, 1024):   # (256: straddle_set)
        assert any(roles[q] == "copies" for q in ui.straddlers(wh, e))


def test_straddle_set(oracle, tmp_path):
    fasta, model, where = ui.straddle_set(oracle)
    path = str(tmp_path / "s.fsa")
    open(path, "wb").write(fasta)
    wh, got = model.window_hits(), model.hit_counts()
    assert sorted(where) == [128, 256, 512] and len(model.ref) >= 256
    for e, q in where.items():
        assert q in ui.straddlers(wh, e)
        assert got[q] == oracle_hits(oracle, path, q) and got[q] > e + 3
        assert len(model.ref[q]) + 10 <= 512
