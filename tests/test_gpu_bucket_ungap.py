"""The bucketed seed pass (k_bkt_group, then k_ungap1 for the singleton groups and the non-QSEG instance of k_ungap2 for the chains: what
the default seed 111111 always takes) on PLANTED diagonals: the query-slot instances and the fall-back above U1_QCAP, the ends of the
query and of the subject array, the X-drop at every element of a step in both directions, the first position of a right pass's maximum,
covered and left-bounded seeds at every count of masked bytes, every word offset of the 64-word scan, the ring, the pass buffer, the list
pieces, the bands and k_bkt_group's segment sizes and cap.  Every set goes through oracle_vs_gpu (rows, candidates of every query,
seed_hits) with SOHIT_UG_COUNT=1 (ungap_steps: the number of BLOSUM lookups, that is the EXTENT of every pass -- what separates a drop of 30
from one of 31) and SOHIT_BUCKET_MIN=0, and the counters say that the flow under test ran: every hit bucketed, and k_ungap1's singletons
and k_ungap2's chains EXACTLY the model's diagonals of one and of two and more kept hits.

The sets and the model come from tests/bucket_ungap_inputs.py (checked against the oracle in tests/test_bucket_ungap_inputs.py); its head
says what cannot be built, and why the slot set is searched with and without the counting instances."""
import pytest

import bucket_ungap_inputs as bi
from test_gpu_parity import fs, gpu_rows, oracle_vs_gpu  # noqa: F401  (fs is a fixture)

pytestmark = pytest.mark.gpu


def kw_of(oracle, flt="F", chk=50000):
    return dict(ssd=bi.SEED, nr=oracle.AA9, ht=bi.HT, chk=chk, step=1, v=500, expect=1e-5, flt=flt, thr=100000)


def setenv(monkeypatch, count=True, **more):
    monkeypatch.setenv("SOHIT_UG_COUNT", "1" if count else "0")
    monkeypatch.setenv("SOHIT_BUCKET_MIN", "0")
    for k, v in more.items():
        monkeypatch.setenv(k, str(v))


def flow_ran(c, m, qs=None):
    """every hit through the buckets; the singleton test of k_ungap1 is exact, so are the counts"""
    assert c["hits_bucketed"] == c["seed_hits"] == m.n_hits(qs)
    assert (c["groups_single"], c["groups_chain"]) == (m.n_single(qs), m.n_chain(qs))
    assert c["groups"] == m.n_single(qs) + m.n_chain(qs)


@pytest.fixture(scope="module")
def slot(oracle):
    return bi.slot_set(oracle)


@pytest.fixture(scope="module")
def scan(oracle):
    return bi.scan_set(oracle)


@pytest.fixture(scope="module")
def chain(oracle):
    return bi.chain_set(oracle)


def test_xdrop_at_every_element(fs, oracle, tmp_path, monkeypatch):
    """a drop of exactly 30 (the pass goes on) and of exactly 31 (it has ended) at every reachable element offset up to 47, both directions"""
    fasta, m, cases = bi.xdrop_set(oracle)
    setenv(monkeypatch)
    c, st = oracle_vs_gpu(fs, oracle, fasta, kw_of(oracle), tmp_path)
    flow_ran(c, m)


@pytest.mark.parametrize("name", ["even", "odd"])
@pytest.mark.parametrize("count", [True, False], ids=["counting_instance", "slot_instances"])
def test_query_slots_and_ends(fs, oracle, tmp_path, monkeypatch, slot, name, count):
    """even: passes whose longest queries are of 7, 512, 1024 and 2048 residues; odd: 513 and 1025.  With the counters (the U1_QCAP slot) the
    flow and the extents; without them the slot instances of 512, 1024 and U1_QCAP residues the passes choose by their longest query: rows
    and candidates.  Singletons that run from the query's last window down to position 1 against the reference's last sequence and from
    position 1 up to the last residue against its first one, the W-rich one at 19 000 points, queries of one and two windows, a subject of 12
    residues, a hit behind a subject's last residue; the batch's last query is of 2048 residues."""
    ref, qry, m, w = slot
    setenv(monkeypatch, count)
    lo, hi = w["ranges"][name]
    c, st = oracle_vs_gpu(fs, oracle, ref, kw_of(oracle), tmp_path, sub=(lo, hi), qry=qry)
    if count:
        flow_ran(c, m, range(lo, hi))
    else:
        assert c["hits_bucketed"] == c["seed_hits"] == m.n_hits(range(lo, hi)) and c["groups"] == m.n_single(range(lo, hi)) + m.n_chain(range(lo, hi))


def test_query_above_the_slot_falls_back(fs, oracle, tmp_path, monkeypatch, slot):
    """2049 residues: pmaxq > U1_QCAP, everything goes to k_ungap"""
    ref, qry, m, w = slot
    setenv(monkeypatch)
    lo, hi = w["ranges"]["over"]
    c, st = oracle_vs_gpu(fs, oracle, ref, kw_of(oracle), tmp_path, sub=(lo, hi), qry=qry)
    assert c["groups_single"] == 0 and c["groups_chain"] == 0
    assert c["hits_bucketed"] == c["seed_hits"] == m.n_hits(range(lo, hi)) and c["groups"] == m.n_single(range(lo, hi)) + m.n_chain(range(lo, hi))


def test_slots_in_two_chunks(fs, oracle, tmp_path, monkeypatch, slot):
    """chk = c0: the subject whose head is query qc opens the second chunk, its offset-0 entry is dropped there; the reference's first and
    last sequence end up in different chunks"""
    ref, qry, m, w = slot
    setenv(monkeypatch)
    lo, hi = w["ranges"]["even"]
    c, st = oracle_vs_gpu(fs, oracle, ref, kw_of(oracle, chk=w["c0"]), tmp_path, sub=(lo, hi), qry=qry)
    assert c["n_chunks"] == 2
    flow_ran(c, bi.BucketModel(oracle, m.refs, m.qrys, chk=w["c0"]), range(lo, hi))


def signature(c, m, env):
    """what the counters say of the flow a switch leaves"""
    if env.get("SOHIT_BUCKET") == "0":
        assert c["hits_bucketed"] == 0
        return
    assert c["hits_bucketed"] == c["seed_hits"]
    if "SOHIT_UG1" in env or "SOHIT_UG_W32" in env:
        assert c["groups_single"] == 0 and c["groups_chain"] == 0
    elif "SOHIT_UG1_CHAIN" in env:
        assert (c["groups_single"], c["groups_chain"]) == (m.n_single(), 0)
    else:
        assert (c["groups_single"], c["groups_chain"]) == (m.n_single(), m.n_chain())


VARIANTS = [{}, {"SOHIT_UG1": "0"}, {"SOHIT_UG1_CHAIN": "0"}, {"SOHIT_UG_W32": "0"}, {"SOHIT_BUCKET": "0"}]


def same_under_every_variant(fs, oracle, monkeypatch, ref, qry, m, sub=(-1, -1)):
    out = []
    for env in VARIANTS:
        setenv(monkeypatch, **env)
        s, hits, rows = gpu_rows(fs, ref, qry, kw_of(oracle), *sub)
        out.append((hits.array().tobytes(), rows, s.counters()))
        hits.close()
        s.close()
        for k in env:
            monkeypatch.delenv(k)
        signature(out[-1][2], m, env)
    rec0, rows0, c0 = out[0]
    assert c0["ungap_steps"] > 0
    for rec, rows, c in out[1:]:
        assert rec == rec0 and rows == rows0
        assert (c["ungap_steps"], c["seed_hits"]) == (c0["ungap_steps"], c0["seed_hits"])
        assert c["groups"] == c0["groups"]


def test_scan_edges(fs, oracle, tmp_path, monkeypatch, scan):
    """64 queries that shift every group of one bucket over every word offset of the 64-word scan, bucket totals of 64 n and 64 n + 1"""
    ref, qry, m = scan
    setenv(monkeypatch)
    # (a range of its own: without one a search ends at the query whose number is the reference's size)
    c, st = oracle_vs_gpu(fs, oracle, ref, kw_of(oracle), tmp_path, sub=(0, len(m.qrys)), qry=qry)
    flow_ran(c, m)


def test_scan_edges_under_every_variant(fs, oracle, monkeypatch, scan):
    ref, qry, m = scan
    same_under_every_variant(fs, oracle, monkeypatch, ref, qry, m, sub=(0, len(m.qrys)))


def test_chains(fs, oracle, tmp_path, monkeypatch, chain):
    """the first segment's maximum at every offset 0 .. 47, ties, the next seed at lo - 1, lo, lo + 1 and behind 0 .. 16 and 20 residues,
    groups of 2, 3, 64, 65 and 245 hits, neighbouring diagonals, two groups on one subject, queries of 512, 1024 and 2048 residues"""
    fasta, m, w = chain
    setenv(monkeypatch)
    c, st = oracle_vs_gpu(fs, oracle, fasta, kw_of(oracle), tmp_path)
    flow_ran(c, m)


def test_chains_under_every_variant(fs, oracle, monkeypatch, chain):
    fasta, m, w = chain
    same_under_every_variant(fs, oracle, monkeypatch, fasta, fasta, m)


def test_chains_on_poisoned_allocations(fs, oracle, tmp_path, monkeypatch, chain):
    fasta, m, w = chain
    setenv(monkeypatch, SOHIT_POISON="165")
    c, st = oracle_vs_gpu(fs, oracle, fasta, kw_of(oracle), tmp_path)
    flow_ran(c, m)


def test_many_lanes_ring_and_segments(fs, oracle, tmp_path, monkeypatch):
    """70 singletons that pass in the same step (the pass buffer of 32 in more than one round), 130 singletons in front of a bucket's first
    longer group (the ring of 128 refilled while lanes work), per-subject segments of 1, 2, 16, 17, 64 and 65 hits, more than BG_BINS
    sequences (several ranges per chunk)"""
    ref, qry, m, w = bi.lanes_set(oracle)
    setenv(monkeypatch)
    c, st = oracle_vs_gpu(fs, oracle, ref, kw_of(oracle), tmp_path, qry=qry)
    flow_ran(c, m)
    assert c["candidates"] >= 70 + 131   # (the burst's 70 subjects, the ring's 131: every planted singleton reaches MIN_UNGAP)


def test_list_pieces(fs, oracle, tmp_path, monkeypatch):
    """one bucket with more chain heads than a wave's piece of the chain list holds, one with more passing singletons than its piece of
    the pass list"""
    ref, qry, m = bi.list_set(oracle)
    setenv(monkeypatch)
    c, st = oracle_vs_gpu(fs, oracle, ref, kw_of(oracle), tmp_path, qry=qry)
    flow_ran(c, m)


@pytest.mark.parametrize("target", [bi.BG_CAP - 1, bi.BG_CAP, bi.BG_CAP + 1])
def test_bucket_at_the_grouping_cap(fs, oracle, tmp_path, monkeypatch, target):
    """queries whose one bucket (SOHIT_BUCKET_AVG=100000: one range per chunk) holds BG_CAP - 1, BG_CAP and BG_CAP + 1 hits"""
    fasta, m, qs = bi.cap_set(oracle, target)
    setenv(monkeypatch, SOHIT_BUCKET_AVG=100000)
    c, st = oracle_vs_gpu(fs, oracle, fasta, kw_of(oracle, flt="T"), tmp_path)
    flow_ran(c, m)


def test_subject_of_several_bands(fs, oracle, tmp_path, monkeypatch):
    """a subject of 13 diagonal bands among 260 of one band: the BANDS instances (btab) of k_ungap1 and k_ungap2 -- bi.band_set says why the
    pass takes the banded layout; singletons and groups of 35 hits in every band"""
    ref, qry, m = bi.band_set(oracle)
    setenv(monkeypatch)
    c, st = oracle_vs_gpu(fs, oracle, ref, kw_of(oracle, flt="T"), tmp_path, qry=qry)
    flow_ran(c, m)
