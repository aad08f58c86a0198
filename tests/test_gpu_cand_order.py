"""The candidate stage of a seed pass -- best diagonal per (query, subject), then a query's candidates in first-touch order -- on PLANTED
pass records, on every path host_seed.hip chooses for it and on the edges of each: the instances of k_q_best (128 / 129, 512 / 513, 2047 /
2048 records of a query) and its overflow at 2049, k_bkt_best with k_cand_order_seg (one and two sub-passes at 16384 / 16385 candidates of
a query, a digit group above its LDS sort and the segmented library sort that redoes the pass) or with the device-wide sort, and the
sorted records with k_cand_order_lds<256> / <2048> (maxseg 256 / 257) or the device-wide sort (2049) in one sort and in two; the tie rules of all three
reductions (equal scores, the minimum first-touch key of a subject whose best diagonal is a later one, equal query positions, the
offset-0 bit, a score of exactly 25 next to one of 24, the sign of the diagonal), in one and in two chunks.

Every set goes through oracle_vs_gpu (the candidates of every query in spill order, rows, counters, the round policy) on poisoned
allocations, and a second, profiled search says which path ordered the candidates: the group.order_*_launches keys (tools/diag/README.md)
are asserted EXACTLY -- a set that does not reach its path fails.

The sets and the model of the stage come from tests/cand_order_inputs.py (checked against the oracle in
tests/test_cand_order_inputs.py); its head says what cannot be built and why.  Every one of the nine keys is asserted non-zero by some
test of this file."""
import pytest

import cand_order_inputs as co
from test_gpu_parity import fs, oracle_vs_gpu  # noqa: F401  (fs is a fixture)

pytestmark = pytest.mark.gpu

BUCKETED = {"SOHIT_BUCKET_MIN": "0"}                              # k_bkt_group, k_bkt_best
GROUPED = {"SOHIT_BUCKET_MIN": "0", "SOHIT_BUCKET_BEST": "0"}     # k_bkt_group, then the records as the sorted grouping leaves them
SORTED = {"SOHIT_BUCKET": "0"}                                    # the sorted grouping: per query below 4096 residues, else sorted records


def kw_of(oracle, chk=50000):
    return dict(ssd=co.SEED, nr=oracle.AA9, ht=co.HT, chk=chk, step=1, v=500, expect=1e-5, flt="F", thr=100000)


def order_paths(fs, ref, qry, kw, sub):
    """{path: passes} of a profiled search: the non-zero group.order_*_launches keys"""
    s = fs.Searcher(profile=True, **kw)
    s.load_ref_bytes(ref)
    s.load_queries_bytes(qry)
    s.search(*sub).close()
    t = s.timing()
    s.close()
    return {k[len("group.order_"):-len("_launches")]: int(v) for k, v in t.items() if k.startswith("group.order_") and k.endswith("_launches") and v}


def check(fs, oracle, tmp_path, monkeypatch, ref, qry, sub, env, want, chk=50000):
    monkeypatch.setenv("SOHIT_POISON", "165")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = kw_of(oracle, chk)
    c, st = oracle_vs_gpu(fs, oracle, ref, kw, tmp_path, sub=sub, qry=qry)
    got = order_paths(fs, ref, qry, kw, sub)
    print("order paths:", got, "candidates:", c["candidates"])
    assert got == want
    return c


def passes_with_candidates(m, sub, chk=None, batch=None):
    """(batch, chunk) pairs in which some query of the range has a hit -- in these sets every subject a query hits is its candidate --:
    the passes that reach the candidate order (one pass per batch and chunk: one length class, hits far below the budget)"""
    out = set()
    for q in range(*sub):
        sid, pos, qp, drop = m.hits(q)
        out |= set(((q - sub[0]) // batch if batch else 0, int(s) // chk if chk else 0) for s in sid[~drop])
    return len(out)


@pytest.fixture(scope="module")
def tier(oracle):
    return co.tier_set(oracle)


@pytest.fixture(scope="module")
def tie(oracle):
    return co.tie_set(oracle)


@pytest.fixture(scope="module")
def seg(oracle):
    return co.seg_set(oracle)


@pytest.mark.parametrize("env", [SORTED, GROUPED], ids=["sorted_grouping", "bucketed_grouping"])
def test_q_best_tiers(fs, oracle, tmp_path, monkeypatch, tier, env):
    """queries of 1, 2, 64, 65, 128, 129, 512, 513, 2047 and 2048 records in one pass: every instance of k_q_best at its first and its last
    record count, runs of 63, 64 and 65 records of one subject"""
    ref, qry, m, w = tier
    c = check(fs, oracle, tmp_path, monkeypatch, ref, qry, w["ranges"]["tiers"], env, {"per_query": 1})
    assert c["candidates"] == sum(len(w["spread"][q]) for q in range(*w["ranges"]["tiers"]))


@pytest.mark.parametrize("name,path", [("tiers_over256", "lds256"), ("over257", "lds2048"), ("over2049", "sort1")])
def test_q_best_overflow_redone_by_the_sorted_flow(fs, oracle, tmp_path, monkeypatch, tier, name, path):
    """a query of 2049 records next to small ones: k_q_best flags, the sorted flow redoes the pass -- with the longest candidate list of
    256 (k_cand_order_lds<256>; the ten tier queries are in this pass), of 257 (<2048>) and of 2049 (the device-wide sort)"""
    ref, qry, m, w = tier
    c = check(fs, oracle, tmp_path, monkeypatch, ref, qry, w["ranges"][name], SORTED, {"per_query_redo": 1, path: 1})
    assert c["candidates"] == sum(len(w["spread"][q]) for q in range(*w["ranges"][name]))


def test_tiers_through_the_bucketed_reduction(fs, oracle, tmp_path, monkeypatch, tier):
    """the same records through k_bkt_best (fewer than 256 queries: the device-wide sort orders them)"""
    ref, qry, m, w = tier
    check(fs, oracle, tmp_path, monkeypatch, ref, qry, w["ranges"]["tiers_over256"], BUCKETED, {"bucket_sort": 1})


TIE_FLOWS = {
    # name: (switches, query range, path)
    "bucket_seg": (BUCKETED, "small", "bucket_seg"),
    "bucket_sort": (dict(BUCKETED, SOHIT_BATCH="128"), "small", "bucket_sort"),
    "per_query_bucketed_grouping": (GROUPED, "small", "per_query"),
    "per_query_sorted_grouping": (SORTED, "small", "per_query"),
    "sorted_records": (SORTED, "all", "lds256"),
}


@pytest.mark.parametrize("chunks", [1, 2])
@pytest.mark.parametrize("flow", sorted(TIE_FLOWS))
def test_tie_rules(fs, oracle, tmp_path, monkeypatch, tie, flow, chunks):
    """equal scores on one subject, the minimum key of a subject whose best diagonal comes later, equal query positions, the offset-0 bit,
    25 next to 24, the three signs of the diagonal (cand_order_inputs.tie_set) under every flow; in two chunks the tie subjects are cut 7 : 8
    and the candidates leave chunk-major.  A batch of 128 queries has no pass of 256: three batches, the device-wide sort (the third batch's
    four queries have their subjects in the second chunk: five passes with candidates in two chunks)."""
    ref, qry, m, w = tie
    env, rng, path = TIE_FLOWS[flow]
    chk = w["chk"] if chunks == 2 else None
    passes = passes_with_candidates(co.BucketModel(oracle, m.refs, m.qrys, chk=chk), w["ranges"][rng], chk, int(env.get("SOHIT_BATCH", 0)))
    assert passes == {("bucket_sort", 1): 3, ("bucket_sort", 2): 5}.get((flow, chunks), chunks)
    check(fs, oracle, tmp_path, monkeypatch, ref, qry, w["ranges"][rng], env, {path: passes}, chk=chk or 50000)


def test_cand_order_seg_sub_passes(fs, oracle, tmp_path, monkeypatch, seg):
    """queries of 16384 (one sub-pass) and 16385 (two) candidates over seventeen and eighteen digits, subjects on both sides of the digit edge
    inside one query position, a query whose candidates sit at its first and its last position; 259 queries in the pass.  The number of
    sub-passes is DESIGNED (the digit arithmetic of tests/test_cand_order_inputs.py), not observed: the profile key is the same for one and
    for two, and what is checked here is that the candidates come out in the oracle's order on either side of the cap"""
    ref, qry, m, w = seg
    c = check(fs, oracle, tmp_path, monkeypatch, ref, qry, w["ranges"]["sub_passes"], BUCKETED, {"bucket_seg": 1})
    assert c["candidates"] >= sum(w["ncand"][q] for q in (w["a1"], w["a2"], w["c"]))


def test_cand_order_seg_digit_group_above_the_cap(fs, oracle, tmp_path, monkeypatch, seg):
    """16400 candidates of one query position and one digit: k_cand_order_seg gives up, the segmented library sort redoes the pass's order"""
    ref, qry, m, w = seg
    c = check(fs, oracle, tmp_path, monkeypatch, ref, qry, w["ranges"]["resort"], BUCKETED, {"bucket_seg_resort": 1})
    assert c["candidates"] >= sum(w["ncand"].values())


def test_seg_set_in_small_batches(fs, oracle, tmp_path, monkeypatch, seg):
    """the same candidates with 128 queries per batch: no pass of 256 queries, the device-wide sort"""
    ref, qry, m, w = seg
    assert passes_with_candidates(m, w["ranges"]["resort"], batch=128) == 3
    check(fs, oracle, tmp_path, monkeypatch, ref, qry, w["ranges"]["resort"], dict(BUCKETED, SOHIT_BATCH="128"), {"bucket_sort": 3})


def test_device_wide_order_in_two_sorts(fs, oracle, tmp_path, monkeypatch):
    """first-touch key + query above 64 bits (a query of 2^18 + 1 residues, a subject of 2^20 + 1, 2055 subjects, 2052 queries in the batch:
    19 + 13 + 21 + 12 = 65): the sorted records of a pass whose longest candidate list is above 2048 are ordered by first-touch key, then
    stably by query"""
    ref, qry, m, w = co.sort2_set(oracle)
    c = check(fs, oracle, tmp_path, monkeypatch, ref, qry, w["range"], SORTED, {"sort2": 1})
    assert c["candidates"] >= co.S2_CANDS - 1 + 2
