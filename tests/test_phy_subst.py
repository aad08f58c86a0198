"""The substitution counts and the two distances made from them by their numpy definitions (swiftortho_amd/phy.py pair_index, subst_counts,
boot_subst, distances / boot_distances under kimura and logdet) against literal restatements, closed forms and the identities that tie the
tensor to pair_counts; then tree() and scripts/rbh2phy.py -m kimura | logdet.  No GPU is needed.  The inputs are
tests/phy_subst_inputs.py's; tests/test_gpu_phy_subst.py holds the device to the same definitions.

The command line runs on the five-taxon hit file of tests/phy_boot_inputs.py (written by hand, 17 columns): a test without a GPU cannot
search the six-taxon proteome of tests/phy_inputs.py; that proteome goes through the script in tests/test_gpu_phy_subst.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import phy_boot_inputs as bin_
import phy_subst_inputs as sin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def phy():
    from swiftortho_amd import phy
    return phy


# ---------------------------------------------------------------------------------------------------------
# the tensor
# ---------------------------------------------------------------------------------------------------------
def test_pair_index(phy):
    assert phy.AA20 == sin.AA20
    for T in (2, 3, 4, 7, 65):
        pi = phy.pair_index(T)
        assert pi.dtype == np.int64 and pi.shape == (T * (T - 1) // 2, 2) and [tuple(x) for x in pi.tolist()] == sin.literal_pairs(T)
    assert phy.pair_index(1).shape == (0, 2)


@pytest.mark.parametrize("T,K", [(2, 1), (2, 70), (3, 33), (5, 70), (4, 17)])
def test_subst_counts_equal_the_literal_loop(phy, T, K):
    for m in (sin.mixed(T, K, T + K), sin.asym(T, K), sin.pure(T, K, K)):
        for keep in (np.arange(K), sin.strict_subset(K) if K > 1 else np.arange(1), np.zeros(0, dtype=np.int64)):
            got = phy.subst_counts(m, keep)
            want = sin.literal_subst(m, keep)
            assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)


def test_asym_tables_are_asymmetric(phy):
    """what the designed input is for: below 21 taxa (taxa t and t + 20 hold the same row) a transposed table is a different table for
    every pair, in 30 of the 400 cells on average"""
    N = phy.subst_counts(sin.asym(9, 129), np.arange(129))
    off = [int((n != n.T).sum()) for n in N]
    assert min(off) >= 8 and np.mean(off) > 20


def test_identities_against_pair_counts(phy):
    """over the 20 letters and '-' alone: N.sum() == cmp and trace(N) == same, pair for pair"""
    for T, K, keep in ((7, 400, None), (13, 129, None), (4, 600, sin.strict_subset(600))):
        m = sin.pure(T, K, T)
        keep = np.arange(K) if keep is None else keep
        N, (cmp_, same) = phy.subst_counts(m, keep), phy.pair_counts(m, keep)
        for p, (i, j) in enumerate(sin.literal_pairs(T)):
            assert N[p].sum() == cmp_[i, j] and np.trace(N[p]) == same[i, j]


def test_uncoded_bytes_only_take_away(phy):
    """with X, B, lower case, 0x00 and 0xFF in the rows the tensor counts fewer columns than pair_counts compares"""
    T, K = 6, 300
    m = sin.mixed(T, K, 3)
    N, (cmp_, same) = phy.subst_counts(m, np.arange(K)), phy.pair_counts(m, np.arange(K))
    less = 0
    for p, (i, j) in enumerate(sin.literal_pairs(T)):
        assert N[p].sum() <= cmp_[i, j] and np.trace(N[p]) <= same[i, j]
        less += int(N[p].sum() < cmp_[i, j])
        if 1 in (i, j) or 2 in (i, j):
            assert N[p].sum() == 0          # the rows of '-' and of X
    assert less > 0


def test_boot_subst(phy):
    m = sin.mixed(5, 90, 1)
    keep = sin.strict_subset(90)
    for seed, b in ((0, 0), (2 ** 64 - 1, 3), (7, 2 ** 31 - 1)):
        draws = bin_.literal_columns(seed, b, len(keep))
        got = phy.boot_subst(m, keep, seed, b)
        assert got.dtype == np.int32 and np.array_equal(got, phy.subst_counts(m, keep[draws])) and np.array_equal(got, sin.literal_subst(m, keep[draws]))


# ---------------------------------------------------------------------------------------------------------
# kimura
# ---------------------------------------------------------------------------------------------------------
def test_kimura(phy):
    cmp_ = np.array([[10, 8], [8, 9]])
    same = np.array([[10, 6], [6, 9]])                       # the counts of test_phy.py test_distances
    d = phy.distances(cmp_, same, "kimura")
    p = 1. - 6. / 8.
    assert d.dtype == np.float64 and d[0, 1] == -np.log(1. - p - p * p / 5.) and d[0, 1] == d[1, 0] and d[0, 0] == 0. and d[1, 1] == 0.
    assert not np.signbit(d).any()
    D, ok = phy.boot_distances(cmp_, same, "kimura")
    assert ok is True and np.array_equal(D, d)
    # p = 0.9: 1 - .9 - .81 / 5 < 0
    far = (np.array([[10, 10], [10, 10]]), np.array([[10, 1], [1, 10]]))
    with pytest.raises(ValueError) as e:
        phy.distances(far[0], far[1], "kimura", [b"tA", b"tB"])
    assert all(w in str(e.value) for w in ("tA", "tB", "kimura")) and isinstance(e.value, phy.DistanceRefused)
    assert phy.boot_distances(far[0], far[1], "kimura")[1] is False
    assert phy.distances(far[0], far[1], "poisson")[0, 1] == -np.log(1. - (1. - 1. / 10.))          # poisson still has one there
    with pytest.raises(ValueError) as e:
        phy.distances([[1, 0], [0, 1]], [[1, 0], [0, 1]], "kimura", [b"tA", b"tB"])
    assert all(w in str(e.value) for w in ("tA", "tB", "no compared column"))
    assert phy.boot_distances([[1, 0], [0, 1]], [[1, 0], [0, 1]], "kimura")[1] is False


def test_other_models_are_still_refused(phy):
    cmp_, same = np.array([[10, 8], [8, 9]]), np.array([[10, 6], [6, 9]])
    for bad in ("jc", "wag", "", "LogDet"):
        with pytest.raises(ValueError):
            phy.distances(cmp_, same, bad)
        with pytest.raises(ValueError):
            phy.boot_distances(cmp_, same, bad)
    with pytest.raises(ValueError):
        phy.distances(cmp_, same, "logdet")                  # no tensor given


# ---------------------------------------------------------------------------------------------------------
# logdet
# ---------------------------------------------------------------------------------------------------------
def logdet_of(phy, m, names=None):
    keep = np.arange(m.shape[1])
    return phy.distances(*phy.pair_counts(m, keep), model="logdet", names=names, subst=phy.subst_counts(m, keep))


@pytest.mark.parametrize("a,b", [(8, 1), (3, 1)])
def test_logdet_closed_form(phy, a, b):
    """N = a I + b (J - I) (condition number (a + 19 b) / (a - b): 27 / 7 and 11): float64 slogdet is good to a few 1e-16 here -- measured
    4.4e-16 on both -- and 1e-12 covers any LAPACK build"""
    m = sin.jc_pair(a, b)
    assert m.shape == (2, 20 * a + 380 * b)
    N = phy.subst_counts(m, np.arange(m.shape[1]))[0]
    assert np.array_equal(N, a * np.eye(20, dtype=np.int32) + b * (1 - np.eye(20, dtype=np.int32)))
    D = logdet_of(phy, m)
    assert abs(D[0, 1] - sin.jc_distance(a, b)) <= 1e-12 and D[0, 1] == D[1, 0]


def test_logdet_of_identical_rows(phy):
    """two equal rows that hold all 20 residues: N is diagonal and the distance 0 -- within 1e-15, not exactly: slogdet sums the logarithms
    of the diagonal one after the other, numpy's sum() of log(r) pairwise, and the two sums differ in the last bit (1.8e-16 here)"""
    row = sin.AA[np.arange(100) % 20]
    row[:37] = sin.AA[3]
    D = logdet_of(phy, np.stack([row, row]))
    assert abs(D[0, 1]) <= 1e-15 and D[0, 0] == 0. and D[1, 1] == 0.


def test_logdet_matrix_is_symmetric_bit_for_bit(phy):
    m = sin.pure(7, 700, 5)
    D = logdet_of(phy, m)
    assert D.dtype == np.float64 and D.tobytes() == D.T.copy().tobytes() and (np.diag(D) == 0.).all() and not np.signbit(np.diag(D)).any()
    assert np.isfinite(D).all() and (D[np.triu_indices(7, 1)] > 0).all()
    Db, ok = phy.boot_distances(*phy.pair_counts(m, np.arange(700)), model="logdet", subst=phy.subst_counts(m, np.arange(700)))
    assert ok is True and Db.tobytes() == D.tobytes()
    far = logdet_of(phy, sin.pure(8, 3000, 1))               # taxon 7 is redrawn most, taxon 0 least
    assert far[0, 7] > far[0, 1]


def test_logdet_refusals(phy):
    names = [b"tA", b"tB", b"tC"]
    m = sin.pure(3, 900, 2)
    m[1, m[1] == ord("W")] = sin.GAP                          # tB lacks W
    with pytest.raises(ValueError) as e:
        logdet_of(phy, m, names)
    assert all(w in str(e.value) for w in ("tA", "tB", "logdet")) and isinstance(e.value, phy.DistanceRefused)
    keep = np.arange(900)
    assert phy.boot_distances(*phy.pair_counts(m, keep), model="logdet", subst=phy.subst_counts(m, keep))[1] is False
    # a singular table: both taxa hold the same function of the column in ten values -- every residue occurs, the rank is 10
    k = np.arange(400)
    sing = np.stack([sin.AA[(k % 10) * 2 + (k // 10) % 2], sin.AA[(k % 10) * 2 + (k // 20) % 2]])
    N = phy.subst_counts(sing, k)[0]
    assert (N.sum(0) > 0).all() and (N.sum(1) > 0).all() and np.linalg.matrix_rank(N.astype(float)) < 20
    with pytest.raises(ValueError) as e:
        logdet_of(phy, sing, names[:2])
    assert all(w in str(e.value) for w in ("tA", "tB", "logdet", "singular"))
    assert phy.boot_distances(*phy.pair_counts(sing, k), model="logdet", subst=phy.subst_counts(sing, k))[1] is False
    with pytest.raises(ValueError):
        phy.distances(*phy.pair_counts(m, keep), model="logdet", subst=np.zeros((2, 20, 20), dtype=np.int32))    # three taxa have three pairs


# ---------------------------------------------------------------------------------------------------------
# tree() and the bootstrap
# ---------------------------------------------------------------------------------------------------------
def test_p_and_poisson_on_the_old_stand_ins_keep_their_bytes(phy):
    """tests/phy_boot_inputs.py's Sm has no `subst`: the bytes below are what the code printed before the two models came"""
    sm = bin_.Sm(bin_.conflict_matrix())
    assert not hasattr(sm, "subst")
    assert phy.tree(sm, "p") == b"((t0:0.135135,(t4:0.135135,t5:0.135135):0.135135):0.008108,(t1:0.145946,t2:0.140541):0.029730,t3:0.143243);"
    assert phy.tree(sm, "p", 20, 3) == b"((t0:0.135135,(t4:0.135135,t5:0.135135)1.000:0.135135)0.950:0.008108,(t1:0.145946,t2:0.140541)0.900:0.029730,t3:0.143243);"
    assert phy.tree(sm, "poisson") == b"((t0:0.152389,(t4:0.157541,t5:0.157541):0.209946):0.016388,(t1:0.173703,t2:0.163850):0.045192,t3:0.166215);"
    assert phy.tree(sm, "poisson", 20, 3) == (b"((t0:0.152389,(t4:0.157541,t5:0.157541)1.000:0.209946)0.900:0.016388,(t1:0.173703,t2:0.163850)0.950:0.045192,"
                                              b"t3:0.166215);")
    assert not hasattr(sm, "subst")
    assert phy.Supermatrix([b"a"], None, None, None, None, None, None).subst is None


def test_tree_under_the_new_models(phy):
    m, B, seed = sin.tree_case()
    sm = sin.Sm(m)
    keep = np.arange(m.shape[1])
    for model in ("kimura", "logdet"):
        D = phy.distances(sm.cmp, sm.same, model, sm.taxa, phy.subst_counts(m, keep))
        assert phy.tree(sm, model) == phy.neighbor_joining(D, sm.taxa)
        count, valid, ok, splits = phy.bootstrap_replicates(sm, B, seed, model)
        assert 3 * (B - valid) <= B                          # at most a third dropped: the device test compares real trees
        for b in range(B):
            c, s = phy.boot_counts(m, keep, seed, b)
            Db, good = phy.boot_distances(c, s, model, phy.boot_subst(m, keep, seed, b))
            assert good == ok[b] and (not good or np.array_equal(splits[b], phy.nj_splits(Db)))
        assert phy.tree(sm, model, B, seed) == phy.neighbor_joining(D, sm.taxa, count / float(valid))
    assert np.array_equal(sm.subst, phy.subst_counts(m, keep))           # computed once, kept
    # an input that loses replicates under logdet, but at most a third (the second end-to-end case of the device test)
    few = sin.Sm(sin.pure(5, 200, 1))
    valid = phy.bootstrap_replicates(few, 12, 1, "logdet")[1]
    assert 8 <= valid < 12


def test_conflict_does_not_survive_logdet(phy):
    """why tree_case() stands in for the designed conflict input"""
    with pytest.raises(phy.DistanceRefused):
        phy.tree(bin_.Sm(bin_.conflict_matrix()), "logdet")


def test_device_call_refuses_before_the_device(phy):
    """what so_phy_subst refuses before it looks for a device; without one, everything else is refused too (no CPU fallback)"""
    from swiftortho_amd import build
    build.build(verbose=False)
    m, keep = sin.mixed(4, 40, 1), np.arange(40)
    for mm, kk, b0, nb, word in ((m[:1], keep, 0, 1, "taxa"), (np.full((4097, 2), 65, dtype=np.uint8), keep[:2], 0, 1, "taxa"), (m, keep[:0], 0, 1, "no kept column"),
                                 (m, np.append(keep, 40), 0, 1, "outside"), (m, keep, 2 ** 31 - 1, 2, "2^31"), (m, keep, 0, 32769, "32768")):
        with pytest.raises(RuntimeError) as e:
            phy.device_boot_subst(mm, kk, 1, b0, nb)
        assert word in str(e.value) and "so_phy_subst" in str(e.value), (word, str(e.value))
    import torch
    if not torch.cuda.is_available():
        for call in (lambda: phy.device_subst_counts(m, keep), lambda: phy.device_boot_subst(m, keep, 1, 0, 2)):
            with pytest.raises(RuntimeError) as e:
                call()
            assert "no HIP device" in str(e.value)
        with pytest.raises(ValueError) as e:
            phy.tree(sin.Sm(sin.tree_case()[0]), "logdet", device_stage=True)
        assert "no HIP device" in str(e.value)


# ---------------------------------------------------------------------------------------------------------
# scripts/rbh2phy.py -m
# ---------------------------------------------------------------------------------------------------------
def run_script(tmp_path, extra, case=(20, 30)):
    fasta, sc = bin_.script_case(*case)
    p, f = str(tmp_path / "x.sc"), str(tmp_path / "x.fsa")
    open(p, "wb").write(sc), open(f, "wb").write(fasta)
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "rbh2phy.py"), "-i", p, "-f", f, "-A", "T"] + list(extra), capture_output=True)


@pytest.mark.parametrize("model", ["kimura", "logdet"])
def test_script_models(tmp_path, model):
    T = 5
    tree = str(tmp_path / "x.nwk")
    r = run_script(tmp_path, ("-t", tree, "-m", model))
    assert r.returncode == 0, r.stderr
    bare = open(tree, "rb").read()
    assert bare.endswith(b";\n") and bare.count(b"\n") == 1 and bare.count(b"(") == T - 2
    r2 = run_script(tmp_path, ("-t", tree, "-m", model, "-B", "20", "-S", "5"))
    assert r2.returncode == 0 and r2.stdout == r.stdout
    import re
    lab = open(tree, "rb").read()
    assert lab.count(b"(") == T - 2 and re.sub(rb"\)[01]\.[0-9]{3}:", b"):", lab) == bare and len(re.findall(rb"\)[01]\.[0-9]{3}:", lab)) == T - 3
    if model == "kimura":
        rp = run_script(tmp_path, ("-t", tree, "-m", "p"))
        assert rp.returncode == 0 and rp.stdout == r.stdout and open(tree, "rb").read() != bare            # the same matrix, other branch lengths


def test_script_refusals(tmp_path):
    tree = str(tmp_path / "x.nwk")
    r = run_script(tmp_path, ("-t", tree, "-m", "logdet"), case=(3, 30))          # 90 columns: a residue is missing somewhere
    assert r.returncode == 2 and r.stdout == b"" and b"logdet" in r.stderr and not os.path.exists(tree)
    for bad in ("jc", "wag"):
        r = run_script(tmp_path, ("-t", tree, "-m", bad))                          # as before the two models: the ValueError's exit
        assert r.returncode == 1 and r.stdout == b"" and b"the model is" in r.stderr and not os.path.exists(tree)
