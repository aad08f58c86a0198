"""The substitution counts on the GPU (csrc/phy.hip k_phy_code / k_phy_subst, include/sohit.h so_phy_subst) against the numpy definitions
(swiftortho_amd/phy.py subst_counts, boot_subst) integer for integer, on the designed inputs of tests/phy_subst_inputs.py: device memory
poisoned, every call twice in one process, every taxa and column edge of the MFMA tiles, the replicates, every refusal; then the Kimura and
LogDet trees end to end, with and without the device.

The asymmetric input (`asym`) is the one that decides whether the row, column and accumulator lane maps of v_mfma_i32_32x32x32_i8 are right:
a transposed table differs from the table in about 30 of its 400 cells.

Run on the GPU box:  python -m pytest tests/test_gpu_phy_subst.py -m gpu -q
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import phy_inputs as pin
import phy_subst_inputs as sin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def phy():
    from swiftortho_amd import phy
    return phy


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("SOHIT_POISON", "165")
    monkeypatch.delenv("SOHIT_PHY_BOOT_BATCH", raising=False)


def check_counts(phy, m, keep):
    """device == numpy, dtype and shape included, twice in one process; one host wait"""
    want = phy.subst_counts(m, keep)
    for _ in range(2):
        stats = {}
        got = phy.device_subst_counts(m, keep, stats=stats)
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)
        assert stats == {"waits": 1, "bytes": want.nbytes}
    return want


# ---------------------------------------------------------------------------------------------------------
# the tensor
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", sin.TAXA)
def test_tensor_on_every_edge(phy, T):
    """asym, mixed and pure over every column edge: below, on and past the 16 bytes of a lane, the k-step of 32, and the chunk"""
    for K in sin.COLS:
        keep = np.arange(K)
        check_counts(phy, sin.asym(T, K), keep)
        check_counts(phy, sin.mixed(T, K, T + K), keep)
        check_counts(phy, sin.pure(T, K, T + K), keep)


@pytest.mark.parametrize("T", (2, 7, 13, 65))
def test_tensor_over_a_strict_subset(phy, T):
    for K in (2, 33, 129, sin.CHUNK_COLS + 40):
        keep = sin.strict_subset(K, T)
        assert 0 < len(keep) < K and (np.diff(keep) > 0).all()
        check_counts(phy, sin.asym(T, K), keep)
        check_counts(phy, sin.mixed(T, K, T), keep)


def test_tensor_identities(phy):
    """on the 20 letters and '-' the device's tensor sums to the device's own pair counts"""
    T, K = 9, 700
    m = sin.pure(T, K, 1)
    N = phy.device_subst_counts(m, np.arange(K))
    cmp_, same = phy.device_build(pin.tasks_from_matrix(m), 1.)[3:]
    for p, (i, j) in enumerate(sin.literal_pairs(T)):
        assert N[p].sum() == cmp_[i, j] and np.trace(N[p]) == same[i, j]


def test_largest_case_and_many_ranges(phy):
    """65 taxa x 3000 columns: 11 x 11 workgroup tiles, the columns in several ranges of whole chunks with a ragged last one"""
    T, K = 65, 3000
    check_counts(phy, sin.asym(T, K), np.arange(K))
    check_counts(phy, sin.mixed(T, K, 9), sin.strict_subset(K, 9))
    # two taxa, one tile: the columns are cut chunk by chunk, and the count that ends a range is in
    for K in (sin.CHUNK_COLS, 2 * sin.CHUNK_COLS, 2 * sin.CHUNK_COLS + 1, 5 * sin.CHUNK_COLS - sin.K_STEP):
        check_counts(phy, sin.asym(2, K), np.arange(K))


# ---------------------------------------------------------------------------------------------------------
# replicates
# ---------------------------------------------------------------------------------------------------------
def check_boot(phy, m, keep, seed, b0, nb):
    want = [phy.boot_subst(m, keep, seed, b0 + k) for k in range(nb)]
    for _ in range(2):
        got = phy.device_boot_subst(m, keep, seed, b0, nb)
        assert got.dtype == np.int32 and got.shape == (nb,) + want[0].shape
        for k in range(nb):
            assert np.array_equal(got[k], want[k]), (b0, k)


@pytest.mark.parametrize("T", (2, 7, 33))
def test_boot_subst(phy, T):
    for K in (1, 33, sin.CHUNK_COLS + 1):
        m = sin.mixed(T, K, 3) if K > 1 else sin.asym(T, K)
        keep = np.arange(K)
        check_boot(phy, m, keep, 12345, 0, 1)
        check_boot(phy, m, keep, 2 ** 64 - 1, 3, 5)
    m = sin.asym(T, 200)
    check_boot(phy, m, sin.strict_subset(200), 2 ** 64 - 1, 2 ** 31 - 2, 2)          # the last two replicates there are
    check_boot(phy, m, sin.strict_subset(200), 0, 0, 5)


# ---------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------
def test_refusals(phy):
    m = sin.mixed(4, 40, 1)
    keep = np.arange(40)
    want = phy.subst_counts(m, keep)
    none = np.zeros(0, dtype=np.int64)
    wide = np.full((4097, 4), 65, dtype=np.uint8)
    big = np.full((4096, 1), 65, dtype=np.uint8)                  # 8 386 560 pairs: 13.4 GB a tensor
    cases = ((m[:1], keep, 0, 1, "taxa"), (wide, np.arange(4), 0, 1, "taxa"), (m, none, 0, 1, "no kept column"), (m, np.append(keep, 40), 0, 1, "outside"),
             (m, np.append(keep, -1), 0, 1, "outside"), (m, keep, 2 ** 31 - 1, 2, "2^31"), (m, keep, 0, 32769, "32768"),
             (big, np.arange(1), 0, 32768, "bytes"))
    for mm, kk, b0, nb, word in cases:
        with pytest.raises(RuntimeError) as e:
            phy.device_boot_subst(mm, kk, 7, b0, nb)
        assert word in str(e.value) and "so_phy_subst" in str(e.value), (word, str(e.value))
        if b0 == 0 and nb == 1:
            with pytest.raises(RuntimeError) as e:
                phy.device_subst_counts(mm, kk)
            assert word in str(e.value), (word, str(e.value))
        assert np.array_equal(phy.device_subst_counts(m, keep), want)              # a valid call still works
    with pytest.raises(RuntimeError) as e:
        phy.device_boot_subst(big, np.arange(1), 7, 0, 32768)
    assert str(4096 * 4095 // 2 * 1600 * 32768) in str(e.value)                     # the bytes it would take
    with pytest.raises(RuntimeError, match="device index out of range"):
        phy.device_subst_counts(m, keep, device=4096)
    with pytest.raises(ValueError):
        phy.device_boot_subst(m, keep, 7, 0, 0)
    assert np.array_equal(phy.device_boot_subst(m, keep, 7, 2, 1)[0], phy.boot_subst(m, keep, 7, 2))


# ---------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["kimura", "logdet"])
def test_trees_with_and_without_the_device(phy, monkeypatch, model):
    m, B, seed = sin.tree_case()
    for matrix, B, seed in ((m, B, seed), (sin.pure(5, 200, 1), 12, 1)):              # the second one loses three replicates under logdet
        host, dev = sin.Sm(matrix), sin.Sm(matrix)
        assert phy.tree(dev, model, 0, seed, True) == phy.tree(host, model, 0, seed)
        want = phy.bootstrap_replicates(host, B, seed, model)
        assert 3 * (B - want[1]) <= B                                               # at most a third dropped: trees are compared
        for batch in ("", "1", "2"):                                                # one device call for all, then forced batches
            monkeypatch.setenv("SOHIT_PHY_BOOT_BATCH", batch)
            got = phy.bootstrap_replicates(dev, B, seed, model, device_stage=True)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1] and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
        monkeypatch.delenv("SOHIT_PHY_BOOT_BATCH")
        assert phy.tree(dev, model, B, seed, True) == phy.tree(host, model, B, seed)
        if model == "logdet":
            assert dev.subst.dtype == np.int32 and np.array_equal(dev.subst, host.subst)


def test_end_to_end_script(phy, tmp_path):
    """the six-taxon proteome of tests/phy_inputs.py through rbh2phy.py -A T -t x -m kimura | logdet: a Newick line of T - 2 opening
    brackets, the same line under -B (labels aside), and -G T writes the bytes of -G F"""
    import re
    from swiftortho_amd import fsearch
    from test_gpu_phy import SEARCH_KW
    fa = pin.six_taxa_proteome()
    p, sc = str(tmp_path / "x.fsa"), str(tmp_path / "x.sc")
    open(p, "wb").write(fa)
    s = fsearch.Searcher(**SEARCH_KW)
    try:
        s.load_ref_bytes(fa)
        s.load_queries_bytes(fa)
        hits = s.search(cigar=True)
        hits.write(sc)
        hits.close()
    finally:
        s.close()

    def run(model, g, boot):
        tree = str(tmp_path / ("x_%s_%s%s.nwk" % (model, g, boot)))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "rbh2phy.py"), "-i", sc, "-f", p, "-A", "T", "-G", g, "-t", tree, "-m", model, "-B", boot],
                           capture_output=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout, open(tree, "rb").read()

    label = rb"\)[01]\.[0-9]{3}:"
    for model, runs in (("logdet", (("T", "12"), ("F", "12"), ("T", "0"))), ("kimura", (("F", "20"), ("F", "0")))):
        out = {(g, b): run(model, g, b) for g, b in runs}
        (g, b), (_, bare) = runs[0], out[runs[-1]]
        for stdout, nwk in out.values():
            assert stdout == out[runs[0]][0] and nwk.endswith(b";\n") and nwk.count(b"\n") == 1 and nwk.count(b"(") == 6 - 2
        assert re.sub(label, b"):", out[g, b][1]) == bare and len(re.findall(label, out[g, b][1])) == 3 and not re.findall(label, bare)
        if model == "logdet":
            assert out["T", "12"] == out["F", "12"]
