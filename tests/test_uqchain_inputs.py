"""The guarantees of tests/uqchain_inputs.py (the sets of tests/test_gpu_uqchain.py), checked without a GPU: the model's diagonals are the
oracle's own (its seed_hits and groups for that query alone), and every planted case is there: the groups of 2, 3, 64 and 65 hits, the long
groups, neighbouring diagonals, two groups on one subject, the covered and the left-bounded seeds, the leftover counts around every tier
limit, and the one largest query of the cap set."""
import numpy as np

import uqchain_inputs as ci

LIMITS = (512, 4096)   # (any two limits: the GPU test builds the set for the library's)


def oracle_stats(oracle, path, q, qpath=None):
    r = oracle.blastp(qpath or path, path, "", ssd=ci.SEED, nr=oracle.AA9, ht=ci.HT, chk=50000, step=1, v=500, expect=1e-5, flt="T", thr=100000, st=q, ed=q + 1)
    return r.stats["seed_hits"], r.stats["groups"]


def same_as_oracle(oracle, model, path, q, qpath=None):
    u, c = model.diagonals(q)
    assert (int(c.sum()), len(u)) == oracle_stats(oracle, path, q, qpath), q


def test_shape_set(oracle, tmp_path):
    fasta, m, w = ci.shape_set(oracle)
    assert fasta == ci.shape_set(oracle)[0] and 401 <= len(m.refs) <= 800   # (two chunks at chk=400)
    assert all(11 <= len(s) <= 512 for s in m.refs)
    assert ci.shape_set_problems(oracle, m.refs, m, w) == []
    path = str(tmp_path / "s.fsa")
    open(path, "wb").write(fasta)
    for q in (0, w["none"], w["pair"][0], w["g65"][0], w["copies"][2], w["cover_gap"][0], w["long"], w["self64"]):
        same_as_oracle(oracle, m, path, q)
    left = m.left_counts()
    assert left[w["none"]] == 0 and len(m.refs[w["none"]]) == 11 and len(m.refs[w["long"]]) == 512
    assert [left[w["self%d" % c]] for c in (63, 64, 65)] == [63, 64, 65]
    for q in w["copies"]:   # many long groups: longer than a wave, four per query
        assert sum(1 for n in m.groups(q)[1] if n > 200) == 4
    # the chain of the covered seeds as the oracle scores it: the first segment alone, the seeds behind its maximum add nothing
    for name in ("cover", "cover_gap"):
        q, h, d, r1 = w[name]
        qs, hs = m.refs[q].tobytes(), m.refs[h].tobytes()
        first = oracle.ungap(qs, hs, 30, 30 + d)
        gap = 0 if name == "cover" else 3
        locs = [(p, p + d) for p in list(range(30, 40 if gap else 55)) + (list(range(53, 58)) if gap else [])]
        assert first[2] == r1 and oracle.ungap_chain(qs, hs, locs)[0] == first[0]


def test_tier_set(oracle, tmp_path):
    fasta, m, fam = ci.tier_set(oracle, LIMITS)
    assert sorted(fam) == [511, 512, 513, 4095, 4096, 4097] and len(m.refs) >= 256
    assert all(11 <= len(s) <= 512 for s in m.refs)
    path = str(tmp_path / "t.fsa")
    open(path, "wb").write(fasta)
    for c, qs in fam.items():
        assert qs and all(int(m.groups(q)[1].sum()) == c for q in qs)
        same_as_oracle(oracle, m, path, qs[0])
    assert m.left_counts().max() == 4097


def test_band_and_cap_sets(oracle, tmp_path):
    ref, qry, m = ci.band_set(oracle)
    rp, qp = str(tmp_path / "r.fsa"), str(tmp_path / "q.fsa")
    open(rp, "wb").write(ref), open(qp, "wb").write(qry)
    big = len(m.refs) - 1
    assert len(m.qrys) >= 256 and len(m.refs[big]) == 6000 and max(len(s) for s in m.qrys) <= 512
    on_big = [q for q in range(len(m.qrys)) if m.sizes_on(q, big)]
    assert len(on_big) >= 60 and all(max(m.sizes_on(q, big).values()) == 30 for q in on_big[:8])
    for q in (on_big[0], on_big[-1], 1):
        same_as_oracle(oracle, m, rp, q, qp)
    fasta, ms = ci.short_set(oracle)
    assert len(ms.refs) == 4000 and 3900 <= ms.n_groups() and ms.left_counts().sum() < 1024 * 1000
    fasta, m, q = ci.cap_set(oracle)
    left = m.left_counts()
    assert len(m.refs) >= 256 and left[q] == left.max() and np.count_nonzero(left == left[q]) == 1 and left[q] >= 270
    path = str(tmp_path / "c.fsa")
    open(path, "wb").write(fasta)
    same_as_oracle(oracle, m, path, q)
