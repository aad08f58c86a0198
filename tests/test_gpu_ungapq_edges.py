"""k_ungapq (the wave-per-query singleton finder of a sparse seed pass) at the edges of its walk: per-query hit counts around the 64-ordinal
steps and the 256-ordinal tiles, the register cache of the first SOHIT_UQ_CACHE ordinals moved to every boundary, a seed whose index
entries lie on both sides of a tile edge and of the cache limit, and two chunks.  Every case goes through oracle_vs_gpu (rows, candidates
of every query, seed_hits) with SOHIT_UG_COUNT=1 (the number of BLOSUM lookups too) and asserts that k_ungapq took singletons.

The sets come from tests/ungapq_inputs.py; that the counts they are built for are the library's own is read back from it (query_work
through swiftortho_amd.dist.sharded_query_work, one rank, one chunk)."""
import numpy as np
import pytest

import ungapq_inputs as ui
from test_gpu_parity import fs, oracle_vs_gpu  # noqa: F401  (fs is a fixture)

pytestmark = pytest.mark.gpu


def kw_of(oracle, chk=50000):
    # thr: the frequency cap (about one hit per query residue and chunk by default) out of reach, so that a query of 250 residues can have 1200
    return dict(ssd=ui.SEED, nr=oracle.AA9, ht=ui.HT, chk=chk, step=1, v=500, expect=1e-5, flt="T", thr=100000)


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    """a process group of this process alone (gloo over a file store), for sharded_query_work"""
    import torch.distributed as dist
    made = not dist.is_initialized()
    if made:
        store = dist.FileStore(str(tmp_path_factory.mktemp("pg") / "store"), 1)
        dist.init_process_group("gloo", store=store, rank=0, world_size=1)
    yield
    if made:
        dist.destroy_process_group()


def library_counts(fs, fasta, kw):
    """seed hits of every query as the library counts them (one chunk: per query and chunk, k_ungapq's n)"""
    from swiftortho_amd import dist as sdist
    s = fs.Searcher(**kw)
    s.load_ref_bytes(fasta)
    s.load_queries_bytes(fasta)
    lens = s.query_lengths()
    w = sdist.sharded_query_work(s, lens, 0, len(lens))
    s.close()
    return w


@pytest.fixture(scope="module")
def edge(oracle):
    return ui.edge_set(oracle)


@pytest.fixture(scope="module")
def straddle(oracle):
    return ui.straddle_set(oracle)


def test_edge_set_counts_are_the_librarys(fs, oracle, edge, one_rank):
    """A generator drift must not lose an edge silently: every count the set is built for occurs among the library's per-query counts, at
    the query built for it; so do a count above 1024 and, for the mosaic queries, the model's."""
    fasta, model, roles = edge
    got = library_counts(fs, fasta, kw_of(oracle))
    want = model.hit_counts()
    assert len(got) == len(roles)
    for q, r in enumerate(roles):
        if r.startswith("edge:"):
            assert got[q] == int(r[5:]), (q, r, got[q])
        elif r != "background":
            assert got[q] == want[q], (q, r, got[q], want[q])
    for c in ui.EDGE_COUNTS:
        assert c in got
    assert got.max() > 1024 and all(got[q] > 1024 for q, r in enumerate(roles) if r == "copies")


@pytest.mark.parametrize("cache", [0, 64, 128, 256, 1024])
def test_cache_boundary(fs, oracle, tmp_path, monkeypatch, edge, cache):
    """The edge set with the register cache ending at `cache` ordinals (0: every index entry read twice, as before the cache; 1024: the
    compiled size, the copies' 1200 hits regenerated beyond it)."""
    monkeypatch.setenv("SOHIT_UG_COUNT", "1")
    monkeypatch.setenv("SOHIT_BUCKET", "0")   # (a set this small would be binned by buckets: every pass on the sorted path)
    monkeypatch.setenv("SOHIT_UQ_CACHE", str(cache))
    c, st = oracle_vs_gpu(fs, oracle, edge[0], kw_of(oracle), tmp_path)
    assert c["hits_bucketed"] == 0 and c["groups_single"] > 0
    # the mosaic queries' pieces alone make 400 singletons, the 1-hit query one more
    assert c["groups_single"] >= 400


@pytest.mark.parametrize("cache", [256, 128])
def test_seed_run_across_tile_and_cache_edge(fs, oracle, tmp_path, monkeypatch, straddle, one_rank, cache):
    """Seeds of seven and eight index entries that begin three ordinals in front of ordinals 128, 256 and 512: at SOHIT_UQ_CACHE=256 the one
    across the first tile edge is also the one across the cache limit (its first entries from the registers, the others regenerated with
    the owner carried in), the one at 512 crosses a tile edge beyond the cache; at 128 the cache ends inside a tile and the walk picks
    the tile up in the middle."""
    fasta, model, where = straddle
    wh = model.window_hits()
    for e, q in where.items():
        assert q in ui.straddlers(wh, e), (e, q)
    got = library_counts(fs, fasta, kw_of(oracle))
    want = model.hit_counts()
    for e, q in where.items():
        assert got[q] == want[q] and got[q] > e + 3, (e, q, got[q], want[q])
    monkeypatch.setenv("SOHIT_UG_COUNT", "1")
    monkeypatch.setenv("SOHIT_BUCKET", "0")   # (a set this small would be binned by buckets: every pass on the sorted path)
    monkeypatch.setenv("SOHIT_UQ_CACHE", str(cache))
    c, st = oracle_vs_gpu(fs, oracle, fasta, kw_of(oracle), tmp_path)
    assert c["hits_bucketed"] == 0 and c["groups_single"] > 0


def test_two_chunks(fs, oracle, tmp_path, monkeypatch, edge):
    """The edge set in two chunks: the queries that meet only themselves have their hits in one chunk and none in the other."""
    monkeypatch.setenv("SOHIT_UG_COUNT", "1")
    monkeypatch.setenv("SOHIT_BUCKET", "0")   # (a set this small would be binned by buckets: every pass on the sorted path)
    c, st = oracle_vs_gpu(fs, oracle, edge[0], kw_of(oracle, chk=400), tmp_path)
    assert c["n_chunks"] == 2
    assert c["hits_bucketed"] == 0 and c["groups_single"] >= 400
