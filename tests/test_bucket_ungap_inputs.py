"""The guarantees of tests/bucket_ungap_inputs.py (the sets of tests/test_gpu_bucket_ungap.py), checked without a GPU: every generator is
deterministic, every planted case is there (*_problems() == []: the designed scores, extents, tie positions and bounds are the oracle's
own, oracle.ungap / oracle.ungap_chain on the one pair involved), the model's diagonals are the oracle's (its seed_hits and groups for that
query alone), and the coverage claims hold for both orders of a bucket."""
import numpy as np
import pytest

import bucket_ungap_inputs as bi


def same_as_oracle(oracle, m, path, q, qpath=None, flt="F"):
    r = oracle.blastp(qpath or path, path, "", ssd=bi.SEED, nr=oracle.AA9, ht=bi.HT, chk=50000, step=1, v=500, expect=1e-5, flt=flt, thr=100000, st=q, ed=q + 1)
    u, c = m.diagonals(q)
    assert (int(c.sum()), len(u)) == (r.stats["seed_hits"], r.stats["groups"]), q
    assert int(c.sum()) == m.n_hits([q])


def write(tmp_path, ref, qry=None):
    rp, qp = str(tmp_path / "r.fsa"), None
    open(rp, "wb").write(ref)
    if qry is not None:
        qp = str(tmp_path / "q.fsa")
        open(qp, "wb").write(qry)
    return rp, qp


def test_xdrop_set(oracle, tmp_path):
    fasta, m, cases = bi.xdrop_set(oracle)
    assert fasta == bi.xdrop_set(oracle)[0] and len(m.refs) < 400
    assert bi.xdrop_problems(oracle, m, cases) == []
    # every element of a step in both directions, the lone 16th included; every reachable offset of the first step
    for left in (False, True):
        offs = sorted(set(c[5] for c in cases if c[4] == left))
        assert offs == list(range(bi.XDROP_LEFT_MIN if left else bi.XDROP_RIGHT_MIN, 48))
        assert set(o % 16 for o in offs if o >= 16) == set(range(16))
    # the twins as the oracle scores them: the 30-drop goes on for 6 + 8 more lookups and gains 27, the 31-drop has ended
    for a, b in zip(cases[0::2], cases[1::2]):
        ua = oracle.ungap(m.refs[a[0]].tobytes(), m.refs[a[1]].tobytes(), a[2], a[3])
        ub = oracle.ungap(m.refs[b[0]].tobytes(), m.refs[b[1]].tobytes(), b[2], b[3])
        assert (ua[0] - ub[0], ua[5] - ub[5]) == (27, 14)
    rp, _ = write(tmp_path, fasta)
    for q in (cases[0][0], cases[1][1], cases[-1][0]):
        same_as_oracle(oracle, m, rp, q)


def test_slot_set(oracle, tmp_path):
    ref, qry, m, w = bi.slot_set(oracle)
    assert (ref, qry) == bi.slot_set(oracle)[:2] and len(m.refs) < 400
    assert bi.slot_problems(oracle, m, w) == []
    assert sorted(L for L, left in w["long"]) == sorted(bi.SLOT_LENGTHS * 2)
    lens = {name: sorted(len(m.qrys[q]) for q in range(*r)) for name, r in w["ranges"].items()}
    assert lens["odd"] == [513, 513, 1025, 1025] and lens["over"] == [2049, 2049] and lens["even"][:2] == [6, 7] and lens["even"][-3:] == [2048] * 3
    q, s, qst, sst = w["wrich"]
    assert 19000 <= oracle.ungap(m.qrys[q].tobytes(), m.refs[s].tobytes(), qst, sst)[0] < 32768 - 8192
    # at chk = c0 the second chunk's first sequence loses its offset-0 entry: one hit of qc fewer, one singleton fewer
    m2 = bi.BucketModel(oracle, m.refs, m.qrys, chk=w["c0"])
    assert m2.n_single([w["qc"]]) == m.n_single([w["qc"]]) - 1 and m2.n_hits() == m.n_hits()
    rp, qp = write(tmp_path, ref, qry)
    for q in (w["q6"], w["q7"], w["tiny"][0], w["long"][(512, True)][0], w["long"][(2049, False)][0], w["wrich"][0]):
        same_as_oracle(oracle, m, rp, q, qp)


def test_scan_set(oracle, tmp_path):
    ref, qry, m = bi.scan_set(oracle)
    assert (ref, qry) == bi.scan_set(oracle)[:2]
    assert bi.scan_problems(m) == []
    assert len(m.refs[0]) == len(m.refs[1]) and max(len(q) for q in m.qrys) <= bi.U1_QCAP
    for rev in (False, True):   # both orders of the bucket: heads, lasts and singletons on the first and on the last word of a scan
        on = {"single": set(), "head": set(), "last": set()}
        for q in range(64):
            s1, hd, la, tot = bi.word_offsets(m.sizes_along(q, [0], rev))
            for k, v in (("single", s1), ("head", hd), ("last", la)):
                on[k] |= set(int(x) % 64 for x in v)
        assert all({0, 63} <= v for v in on.values())
        assert [sum(m.sizes_along(q, [0], rev)) % 64 for q in (64, 65)] == [0, 1]
    rp, qp = write(tmp_path, ref, qry)
    for q in (0, 1, 63, 64, 65):
        same_as_oracle(oracle, m, rp, q, qp)


def test_chain_set(oracle, tmp_path):
    fasta, m, w = bi.chain_set(oracle)
    assert fasta == bi.chain_set(oracle)[0] and len(m.refs) < 400
    assert bi.chain_problems(oracle, m, w) == []
    cov = w["cover"]
    assert all(("max", k) in cov for k in range(48)) and all(("gap", g) in cov for g in list(range(17)) + [20])
    # the tie cases: the FIRST position of the maximum, and where the second one lies -- in the same group of three elements, in the next
    # group, in the next step
    for k, same_group, same_step in ((19, True, True), (20, False, True), (30, False, False), (15, False, False)):
        q, h, qst, sst, r1, nxt, tie = cov[("tie", k)]
        assert tie and r1 == k and oracle.ungap(m.refs[q].tobytes(), m.refs[h].tobytes(), qst, sst)[2] == qst + k
        a, b = k % 16, (k + 2) % 16
        assert (k // 16 == (k + 2) // 16) == same_step and (same_step and a // 3 == b // 3 and b != 15) == same_group
    # a gap of 20: the bound falls into the second left step
    q, h, qst, sst, r1, nxt, tie = cov[("gap", 20)]
    assert 16 < nxt - (qst + r1 + 1) <= 32
    rp, _ = write(tmp_path, fasta)
    for q in (w["pair"][0], w["g65"][0], w["copies"][1], cov[("max", 0)][0], cov[("tie", 30)][0], cov[("len", 2048)][0]):
        same_as_oracle(oracle, m, rp, q)


def test_lanes_and_list_sets(oracle, tmp_path):
    ref, qry, m, w = bi.lanes_set(oracle)
    assert (ref, qry) == bi.lanes_set(oracle)[:2] and len(m.refs) > bi.BG_BINS
    assert bi.lanes_problems(oracle, m, w) == []
    # the burst: 64 and more singletons whose score reaches MIN_UNGAP within one step of both passes
    q = w["burst"]
    sid, pos, qp, drop = m.hits(q)
    assert len(sid) >= 64
    for s, p, x in zip(sid, pos, qp):
        u = oracle.ungap(m.qrys[q].tobytes(), m.refs[int(s)].tobytes(), int(x), int(p))
        assert u[0] >= 25 and u[5] <= 16
    rp, qp = write(tmp_path, ref, qry)
    for q in range(3):
        same_as_oracle(oracle, m, rp, q, qp)
    ref, qry, m = bi.list_set(oracle)
    assert (ref, qry) == bi.list_set(oracle)[:2]
    assert bi.list_problems(m) == []
    rp, qp = write(tmp_path, ref, qry)
    for q in range(2):
        same_as_oracle(oracle, m, rp, q, qp)


@pytest.mark.parametrize("target", [bi.BG_CAP - 1, bi.BG_CAP, bi.BG_CAP + 1])
def test_cap_set(oracle, tmp_path, target):
    fasta, m, qs = bi.cap_set(oracle, target)
    assert fasta == bi.cap_set(oracle, target)[0] and qs
    for q in qs:
        assert int(m.kept(q)[1].sum()) == target
    rp, _ = write(tmp_path, fasta)
    same_as_oracle(oracle, m, rp, qs[0], flt="T")


def test_band_set(oracle, tmp_path):
    ref, qry, m = bi.band_set(oracle)
    big = len(m.refs) - 1
    assert len(m.refs[big]) == 6000 and max(len(s) for s in m.qrys) < 256
    on_big = [q for q in range(len(m.qrys)) if 35 in m.hits_on(q, big).values()]
    assert len(on_big) >= 60
    # singletons and chains over the whole width of the long subject: in each of its 13 bands of 2^9 diagonals
    d1 = np.array([d for q in range(len(m.qrys)) for d, n in m.hits_on(q, big).items() if n == 1])
    d2 = np.array([d for q in on_big for d, n in m.hits_on(q, big).items() if n == 35])
    assert len(set(d1 // 512)) >= 12 and len(set(d2 // 512)) >= 12
    rp, qp = write(tmp_path, ref, qry)
    for q in (on_big[0], on_big[-1], 1):
        same_as_oracle(oracle, m, rp, q, qp, flt="T")
