"""The guarantees of tests/cand_order_inputs.py (the sets of tests/test_gpu_cand_order.py), checked without a GPU: every generator is
deterministic, the candidates the oracle reports per query and chunk (Result.cands) are EXACTLY the model's (expected_cands: subject,
score, qi, qj, in spill order) and the planted numbers, the model's passing diagonals are the planted record counts, the oracle's hits
and groups are the model's (nothing unplanned exists), and the tie cases come out of the oracle in the order the head of the file claims.
A set whose oracle answer does not match its design is a wrong set."""
import numpy as np

import cand_order_inputs as co


def kw_of(oracle, chk=50000):
    return dict(ssd=co.SEED, nr=oracle.AA9, ht=co.HT, chk=chk, step=1, v=500, expect=1e-5, flt="F", thr=100000)


def write(tmp_path, ref, qry):
    rp, qp = str(tmp_path / "r.fsa"), str(tmp_path / "q.fsa")
    open(rp, "wb").write(ref)
    open(qp, "wb").write(qry)
    return rp, qp


def same_as_oracle(oracle, m, rp, qp, q, chk=50000):
    """hits and groups of query q alone: the oracle's are the model's"""
    r = oracle.blastp(qp, rp, "", st=q, ed=q + 1, **kw_of(oracle, chk))
    u, c = m.diagonals(q)
    assert (int(c.sum()), len(u)) == (r.stats["seed_hits"], r.stats["groups"]), q
    return r


def test_tier_set(oracle, tmp_path):
    ref, qry, m, w = co.tier_set(oracle)
    assert (ref, qry) == co.tier_set(oracle)[:2]
    assert sorted(w["tier"]) == sorted(co.TIERS) and max(len(q) for q in m.qrys) < 512 and sum(len(s) for s in m.refs) < 100000
    # every tier limit of k_q_best from both sides, and the overflow
    for L in co.Q_BEST_TIERS:
        assert L in w["tier"] and (L + 1 in w["tier"] or L + 1 == 2049)
    rp, qp = write(tmp_path, ref, qry)
    r = oracle.blastp(qp, rp, "", st=0, ed=len(m.qrys), **kw_of(oracle))
    runs = set()
    for q in range(len(m.qrys)):
        got, nrec, ncand = co.expected_cands(oracle, m, q)
        sp = w["spread"][q]
        assert nrec == [sum(sp)] and ncand == [len(sp)], q                 # the planted records and candidates
        assert r.cands(q).tolist() == got, q                              # ... are the oracle's, record by record and in its order
        lo, hi = w["subjects"][q]
        assert sorted(c[0] for c in got) == list(range(lo, hi))
        assert [sum(m.hits_on(q, s).values()) for s in range(lo, hi)] == sp and all(set(m.hits_on(q, s).values()) == {1} for s in range(lo, hi))
        runs |= set(sp)
    assert {1, 2, 63, 64, 65} <= runs
    for R in co.TIERS:
        assert sum(w["spread"][w["tier"][R]]) == R
    assert [(sum(co.OVER[k]), len(co.OVER[k])) for k in ("over256", "over257", "over2049")] == [(2049, 256), (2049, 257), (2049, 2049)]
    # the ranges: no query above 2048 records among the tiers; one in each of the others, the longest candidate list its own
    rg = w["ranges"]
    assert max(sum(w["spread"][q]) for q in range(*rg["tiers"])) == 2048
    for name, longest in (("tiers_over256", 256), ("over257", 257), ("over2049", 2049)):
        qs = range(*rg[name])
        assert len(qs) >= 3 and sorted(sum(w["spread"][q]) for q in qs)[-2:][0] <= 2048 and max(sum(w["spread"][q]) for q in qs) == 2049
        assert max(len(w["spread"][q]) for q in qs) == longest
    assert r.stats["seed_hits"] == r.stats["groups"] == sum(sum(sp) for sp in w["spread"].values())   # nothing unplanned
    for q in (w["tier"][1], w["tier"][2048], w["over"]["over2049"]):
        same_as_oracle(oracle, m, rp, qp, q)


def test_tie_set(oracle, tmp_path):
    ref, qry, m, w = co.tie_set(oracle)
    assert (ref, qry) == co.tie_set(oracle)[:2]
    q, S, chk = w["ties"], w["subj"], w["chk"]
    m2 = co.BucketModel(oracle, m.refs, m.qrys, chk=chk)
    assert co.tie_problems(oracle, m, m2, w) == []
    rp, qp = write(tmp_path, ref, qry)
    r1 = same_as_oracle(oracle, m, rp, qp, q)
    r2 = same_as_oracle(oracle, m2, rp, qp, q, chk)
    got = r1.cands(0).tolist()
    assert got == co.expected_cands(oracle, m, q)[0] and co._same(w["order"], got)
    got2 = r2.cands(0).tolist()
    assert got2 == co.expected_cands(oracle, m2, q, chk)[0] and co._same(w["order2"], got2)
    assert [c[0] < chk for c in got2] == [True] * 7 + [False] * 8 and sorted(map(tuple, got)) == sorted(map(tuple, got2))
    by = {c[0]: c for c in got}
    qpos, spos = w["qpos"], w["spos"]
    rank = {c[0]: i for i, c in enumerate(got)}

    def dist(sname, segname):
        d = spos[(sname, segname)] - qpos[segname]
        return [0, d] if d > 0 else [-d, 0]

    # equal scores: the diagonal visited first, which is not the first one in the subject
    assert by[S["A"]][1:] == [30] + dist("A", "a1") and spos[("A", "a1")] > spos[("A", "a2")]
    assert by[S["B"]][1:] == [31] + dist("B", "b1") and spos[("B", "b3")] < spos[("B", "b1")] < spos[("B", "b2")]
    # the record is the best diagonal, the place the earliest one's
    assert by[S["C"]][1:] == [40] + dist("C", "c2") and qpos["c1"] < qpos["m"] < qpos["c2"] and rank[S["C"]] + 1 == rank[S["M"]]
    # one query position: the higher subject first; J1's real entry in front of its offset-0 entry (J's candidate), J in front of I
    assert S["E2"] == S["E1"] + 1 and rank[S["E2"]] + 1 == rank[S["E1"]]
    assert [S["J2"], S["J1"], S["J"], S["I"]] == [c[0] for c in got[rank[S["J2"]]:rank[S["J2"]] + 4]] and S["J1"] == S["J"] + 1
    assert by[S["J"]][1] >= 78 and m.hits_on(q, S["J"]) == {len(m.refs[S["J"]]) - qpos["quirk"]: 1}   # its only hit: behind its last residue
    # 24 is no record: F's place is the 25's, behind N
    assert by[S["F"]][1:] == [25] + dist("F", "f25") and qpos["f24"] < qpos["n"] < qpos["f25"] and rank[S["N"]] + 1 == rank[S["F"]]
    assert oracle.ungap_chain(m.qrys[q].tobytes(), m.refs[S["F"]].tobytes(), [(qpos["f24"], spos[("F", "f24")])])[0] == 24
    # the sign of the diagonal
    assert by[S["Gp"]][2:] == [0, 37] and by[S["Gn"]][2] > 0 and by[S["Gn"]][3] == 0 and by[S["G0"]][2:] == [0, 0]
    # the fillers: one candidate each at most, 258 and more in all; the last query meets nothing; a pass of 256 and more queries
    lo, hi = w["ranges"]["small"]
    assert hi - lo >= 256 and w["ranges"]["all"] == (0, len(m.qrys)) and len(m.qrys[-1]) >= 4096 and max(len(x) for x in m.qrys[:-1]) < 512
    r = oracle.blastp(qp, rp, "", st=1, ed=len(m.qrys), **kw_of(oracle))
    n = [len(r.cands(k)) for k in range(len(m.qrys) - 1)]
    assert max(n) == 1 and sum(n[:-1]) >= co.N_FILL - 1 and n[-1] == 0


def test_seg_set(oracle, tmp_path):
    ref, qry, m, w = co.seg_set(oracle)
    assert ref == co.seg_set(oracle)[0]
    assert co.seg_problems(m, w) == []
    rp, qp = write(tmp_path, ref, qry)
    lo, hi = w["ranges"]["resort"]
    assert w["ranges"]["sub_passes"] == (lo, hi - 1) and hi - 1 - lo >= 256 and w["b"] == hi - 1
    r = oracle.blastp_parallel(qp, rp, "", st=lo, ed=hi, **kw_of(oracle))
    for q, n in w["ncand"].items():
        got, nrec, ncand = co.expected_cands(oracle, m, q)
        assert nrec == [n] and ncand == [n], q
        assert r.cands(q).tolist() == got, q
    assert w["ncand"][w["a1"]] == co.CO_CAP and w["ncand"][w["a2"]] == co.CO_CAP + 1 and w["ncand"][w["b"]] > co.CO_CAP
    # the first-touch word of this set: 9 bits of query position, 17 of owner + 1, the offset-0 bit; its top 11: (position, owner + 1 >> 15)
    bp, bs = int(np.ceil(np.log2(max(len(x) for x in m.qrys)))), int(np.ceil(np.log2(len(m.refs))))
    assert (bp, bs) == (9, 16)

    def digits(q):
        sid, pos, qp_, drop = m.hits(q)
        return (qp_ << 2) | ((sid + 1) >> (bs + 1 - 2))

    d = digits(w["b"])
    assert len(set(d.tolist())) == 1                                       # one digit group above the cap
    for q in (w["a1"], w["a2"]):
        u, c = np.unique(digits(q), return_counts=True)
        assert len(u) >= 17 and c.max() <= co.CO_CAP                      # every group fits: sub-passes, no fall-back
        first = int(np.searchsorted(np.cumsum(c), co.CO_CAP, side="right"))   # digits of the first sub-pass
        assert (first == len(u)) == (q == w["a1"])
    assert (digits(w["a1"]) & 3).max() == 1 and (digits(w["a1"]) & 3).min() == 0   # both sides of the digit edge inside a position
    d = digits(w["c"]) >> 2
    assert sorted(set(d.tolist())) == [1, 505]
    assert r.stats["seed_hits"] == r.stats["groups"] == sum(len(m.hits(q)[0]) for q in range(lo, hi))   # nothing unplanned
    n = [len(r.cands(q)) for q in range(3, hi - 1)]
    assert max(n) == 1 and sum(n) >= len(n) - 1


def test_sort2_set(oracle, tmp_path):
    ref, qry, m, w = co.sort2_set(oracle)
    assert (ref, qry) == co.sort2_set(oracle)[:2]
    # the widths of the pass: the sort key fits 64 bits, the first-touch key fits, first-touch key + query does not
    bp, bs, bd, bsp, bq = co.sort2_bits(m.refs, m.qrys)
    assert (bp, bs, bd, bsp, bq) == (19, 12, 21, 21, 12)
    assert bq + bs + bd + bp <= 64 and bp + (bs + 1) + bsp <= 64 < bp + (bs + 1) + bsp + bq
    assert bp + (bs + 1) + 1 <= 64 - 11          # (k_cand_order_lds could hold the word: only maxseg keeps it away)
    rp, qp = write(tmp_path, ref, qry)
    lo, hi = w["range"]
    r = oracle.blastp_parallel(qp, rp, "", st=lo, ed=hi, **kw_of(oracle))
    assert r.nqueries == len(m.qrys) == hi
    for q in (0, w["big"], 2, w["long"]):
        got, nrec, ncand = co.expected_cands(oracle, m, q)
        assert r.cands(q).tolist() == got, q
        if q in w["ncand"]:
            assert ncand == [w["ncand"][q]]
    n = len(r.cands(w["big"]))
    assert 2048 < co.S2_CANDS - 1 <= n <= co.S2_CANDS                       # maxseg > 2048: no LDS order
    assert len(m.qrys[w["long"]]) >= 4096 and len(r.cands(w["long"])) == 0   # pmaxq >= 4096: no per-query flow
    assert sum(len(r.cands(q)) for q in range(4, hi)) == 0
    assert r.stats["seed_hits"] == r.stats["groups"] == sum(len(m.hits(q)[0]) for q in range(4))   # nothing unplanned
