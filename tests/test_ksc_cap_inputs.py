"""The guarantees of tests/ksc_cap_inputs.py (the sets of tests/test_gpu_ksc_cap.py), checked without a GPU.  For every set: the quicksort
model is the oracle's permutation on every query's keys, the numpy model of the cap gives the oracle's marks (find_msav_m on every chunk's
index) and the oracle's work query by query, the work of all queries is the seed-hit counter of oracle.blastp_parallel on the same set --
and the DEVIATION TABLE: every wrong variant a query is there for gives another work figure than the reference's rule.  That is what makes
the GPU test's comparison of per-query sums as strong as a comparison of marks on these sets.  Then what the single sets claim: the sizes,
the places of the cut, the leaves of the flush query (and that no LDS instance can flush), the open / closed split of every flow."""
import numpy as np
import pytest

import ksc_cap_inputs as kc


def ranked(oracle, ksc, cnt):
    order = kc.variant_order(oracle, ksc, None)
    c = cnt[order]
    return order, c, np.cumsum(c) - c


@pytest.mark.parametrize("name", kc.SET_NAMES)
def test_model_is_the_oracle_and_the_variants_differ(oracle, tmp_path, name):
    S = kc.get_set(oracle, name)
    model = kc.model_of(oracle, S)
    work, marks = kc.reference_work(oracle, name)
    assert len(model) == len(S.qrys) > 0 and len(S.refs) > len(S.qrys)   # (a search without a range covers min(queries, references))
    for q, (ksc, cnts, limit) in enumerate(model):
        assert limit == S.thr * len(S.qrys[q]) and len(ksc) == S.nk(q)
        perm, _ = kc.qsort_model(-ksc)
        assert perm == oracle.qsort_perm(-ksc), (name, q)                                   # the order
        for c, mk in zip(cnts, marks[q]):
            assert sorted(kc.cap_marks(perm, c, limit).tolist()) == mk.tolist(), (name, q)   # the marks
    assert kc.model_work(oracle, S, model) == work                                           # the work, query by query
    qp, rp = str(tmp_path / "q.fsa"), str(tmp_path / "r.fsa")
    open(qp, "wb").write(S.qry), open(rp, "wb").write(S.ref)
    kw = S.kw(oracle)
    r = oracle.blastp_parallel(qp, rp, "", st=0, ed=len(S.qrys), **kw)
    assert r.nqueries == len(S.qrys) and r.stats["seed_hits"] == sum(work)                   # ... and the trusted counter
    # the deviation table
    bad = kc.undecided(oracle, S, model)
    assert not bad, {S.tag[q]: v for q, v in bad.items()}
    table = {S.tag[q]: {str(v): sum(kc.variant_work(oracle, model[q][0], c, model[q][2], v) for c in model[q][1]) for v in (None,) + tuple(S.need[q])}
             for q in S.need}
    print(name, "thr", S.thr, "work", work, "table", table)


def test_sizes_shapes_and_needs(oracle):
    have = set()
    for name in kc.SHAPES:
        S = kc.get_set(oracle, name)
        assert [S.nk(q) for q in range(len(kc.SIZES))] == list(kc.SIZES) and (S.flt == "T") == (name == "seg")
        have |= set(kc.SIZES)
        for q, nk in enumerate(kc.SIZES):
            assert {"stable", "reverse", "numpy", "early", "late"} <= set(S.need[q]) and (("tier", kc.TIERS.get(nk)) in S.need[q]) == (nk in kc.TIERS)
    S = kc.get_set(oracle, "small")
    assert [S.nk(q) for q in range(len(kc.SMALL))] == list(kc.SMALL)
    have |= set(kc.SMALL)
    assert have >= {1, 2, 6, 7, 8, 31, 32, 33, 63, 64, 65, 128, 129, 512, 513, 1024, 1025, 4096, 4097}
    assert kc.needs_of(1) == () and set(kc.needs_of(2)) == set(kc.needs_of(6)) == {"reverse", "early", "late"} and "stable" in kc.needs_of(7)
    # the key shapes are what the head says: one value, two values, monotone plateaus, ties everywhere
    m = {name: kc.model_of(oracle, kc.get_set(oracle, name))[:len(kc.SMALL if name == "small" else kc.SIZES)] for name in ("tied", "two", "asc", "desc", "small")}
    for ksc, _, _ in m["tied"]:
        assert set(ksc.tolist()) == {30}
    for ksc, _, _ in m["two"]:
        assert set(ksc.tolist()) == {32, 33}
    for ksc, _, _ in m["asc"]:
        assert np.all(np.diff(ksc) >= 0) and ksc[0] < ksc[-1]
    for ksc, _, _ in m["desc"]:
        assert np.all(np.diff(ksc) <= 0) and ksc[0] > ksc[-1]
    for ksc, _, _ in m["small"][1:]:
        assert len(set(ksc.tolist())) < len(ksc)   # ties
    # several patterns: mink is the shorter span and the counts hold both spans' / both alphabets' entries
    S = kc.get_set(oracle, "spans")
    assert S.mink == 6 and S.ssd.count(",") == 1 and kc.get_set(oracle, "alphabets").nr.count("/") == 1
    for name in ("spans", "alphabets"):
        S = kc.get_set(oracle, name)
        one = kc.model_of(oracle, kc.CapSet("one", S.refs, S.qrys, S.thr))
        two = kc.model_of(oracle, S)
        assert all(int(b[1][0].sum()) > int(a[1][0].sum()) for a, b in zip(one, two))


def test_seg_windows_consume_ranks(oracle):
    """every query of the seg set is masked; from 128 windows on a window that holds an x stands in front of the cut (taken, counting
    nothing), and the windows of x alone are refused"""
    S = kc.get_set(oracle, "seg")
    for q, (ksc, (cnt,), limit) in enumerate(kc.model_of(oracle, S)[:len(kc.SIZES)]):
        mq = S.masked(oracle, q)
        assert b"x" in mq and len(mq) == len(S.qrys[q])
        order, c, pre = ranked(oracle, ksc, cnt)
        n = len(kc.cap_marks(order, cnt, limit))
        masked = np.array([b"x" in mq[i:i + kc.K] for i in range(len(ksc))])
        assert not cnt[masked].any() and 0 < n < len(ksc)
        assert not masked[order[:n]].all() and masked[order[n:]].any()
        if S.nk(q) >= 128:
            assert masked[order[:n]].any(), S.tag[q]


@pytest.mark.parametrize("place", kc.PLACES + ("sum",))
def test_cut_places(oracle, place):
    S = kc.get_set(oracle, "closed" if place == "sum" else "cut_" + place)
    assert [S.tag[q] for q in range(4)] == ["%s%d_%s" % (s, n, place) for n in (129, 1025) for s in ("tied", "two")]
    (some, everybody), opens = kc.model_flow(S, kc.model_of(oracle, S))
    for q, (ksc, (cnt,), limit) in enumerate(kc.model_of(oracle, S)):
        order, c, pre = ranked(oracle, ksc, cnt)
        n = len(kc.cap_marks(order, cnt, limit))
        if place.startswith("eq"):
            r = int(place[2:])
            assert pre[r] == limit and n == r + 1 and c[r] > 0 and c[r + 1] > 0   # rank r on the limit and taken, r + 1 refused
        elif place == "first":
            assert n == 1 and c[0] > limit and c[1] > 0
        elif place == "last":
            assert n == len(ksc) and pre[-1] <= limit < c.sum()                   # open for k_cap_all, whole for k_cap
        else:
            assert n == len(ksc) and c.sum() == limit
    assert opens == ([[]] if place == "sum" else [[0, 1, 2, 3]])
    assert (some, everybody) == ((0, 0) if place == "sum" else (0, 1))


def test_flush_query_and_the_lds_instances(oracle):
    S = kc.get_set(oracle, "flush")
    ksc = kc.model_of(oracle, S)[0][0]
    assert len(ksc) == kc.FLUSH_NK > 4096 and set(ksc.tolist()) == {30}
    perm, leaves = kc.qsort_model(-ksc)
    assert leaves == kc.tied_leaves(kc.FLUSH_NK) > kc.WQS_LEAF
    assert max(kc.tied_leaves(n) for n in range(4097, kc.FLUSH_NK)) <= kc.WQS_LEAF      # the smallest such tied query
    for n in (2, 31, 32, 33, 64, 100, 513, 1000, 4097):
        assert kc.qsort_model([0] * n)[1] == kc.tied_leaves(n), n
    # the LDS instances: no family fills a leaf list
    most = {cap: 0 for cap in kc.LDS_LEAFCAP}
    for name in kc.SHAPES:
        for ksc, _, _ in kc.model_of(oracle, kc.get_set(oracle, name))[:len(kc.SIZES)]:
            if len(ksc) <= 4096:
                cap = min(c for c in kc.LDS_LEAFCAP if len(ksc) <= c)
                most[cap] = max(most[cap], kc.qsort_model(-ksc)[1])
    print("most leaves per LDS instance:", most)
    assert all(0 < most[cap] <= kc.LDS_LEAFCAP[cap] // 2 for cap in most)


def test_flow_sets(oracle):
    def flow(name, lazy=True):
        S = kc.get_set(oracle, name)
        return kc.model_flow(S, kc.model_of(oracle, S), lazy)

    assert flow("half") == ((1, 0), [[0, 1, 2, 3]]) and len(kc.get_set(oracle, "half").qrys) == 8      # open * 2 == nq: the open ones
    assert flow("half1") == ((0, 1), [[0, 1, 2, 3, 4]]) and len(kc.get_set(oracle, "half1").qrys) == 8  # one more: everybody
    assert flow("chunks3") == ((6, 0), [[], [1, 3], [2, 3]])
    S = kc.get_set(oracle, "deferred")
    assert flow("deferred") == ((1, 0), [[7]])
    lens = [len(q) for q in S.qrys]
    assert max(lens[:7]) < 512 and lens[7] - kc.K + 1 == kc.FLUSH_NK > 4096 and len(S.qrys) == 8         # length class 4 behind class 0
    assert flow("flush") == ((0, 1), [[0]])
    # the designed queries of a shape set (of the small set: all but the one of one window) are open, the light ones behind them are
    # not and outnumber them: with the orders on demand every tier goes through the open list
    for name in kc.SHAPES:
        assert flow(name) == ((1, 0), [list(range(len(kc.SIZES)))]) and len(kc.get_set(oracle, name).qrys) == 2 * len(kc.SIZES) + 1
    assert flow("small") == ((1, 0), [list(range(1, len(kc.SMALL)))]) and len(kc.get_set(oracle, "small").qrys) == 2 * len(kc.SMALL)
    for name in kc.SET_NAMES:
        assert flow(name, lazy=False)[0] == (0, 0)
