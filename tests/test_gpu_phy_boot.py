"""The bootstrap of the species tree on the GPU (csrc/phy.hip, include/sohit.h so_phy_boot_counts / so_phy_nj_splits / so_phy_boot) against
the numpy definitions (swiftortho_amd/phy.py) array for array and bit set for bit set, on the designed inputs of tests/phy_boot_inputs.py:
device memory poisoned, every call twice in one process, every batch edge, every refusal; then scripts/rbh2phy.py -B on a proteome of six
taxa.  The walk (k_phy_nj) is also run beyond one pass of its 256 lanes and on both sides of its LDS limit: test_nj_splits_wide,
test_nj_ties_across_a_lanes_columns, test_boot_wide; nj_tier in the result says where the clade bit sets were kept.

Observed on an MI355X, numpy reference included (it is nearly all of it: one device call of the four wide matrices takes 0.014 s at 257
taxa and 0.14 s at 641, in either tier):
test_nj_splits_wide 0.4 s at 255 - 257 taxa, 2.1 s at 513, 3.6 s at 640, 3.7 s at 641; test_nj_ties_across_a_lanes_columns 1.9 s;
test_boot_wide 0.6 s at 257 x 96 and 1.8 s at 641 x 80.  No path disagreed with numpy.  Deviation check, each change alone in the kernel:
a lane's argmin that replaces only on a smaller Q fails test_nj_ties_across_a_lanes_columns and nothing else; a cross-wave pick on Q
alone fails that test and the stacks of 128, 129, 256, 513, 640 and 641 taxa.

Run on the GPU box:  python -m pytest tests/test_gpu_phy_boot.py -m gpu -q
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import phy_boot_inputs as bin_
import phy_inputs as pin

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


# ---------------------------------------------------------------------------------------------------------
# so_phy_boot_counts
# ---------------------------------------------------------------------------------------------------------
def check_counts(phy, m, keep, seed, b0, nb):
    want = [phy.boot_counts(m, keep, seed, b0 + k) for k in range(nb)]
    for _ in range(2):
        cmp_, same = phy.device_boot_counts(m, keep, seed, b0, nb)
        assert cmp_.dtype == np.int64 and cmp_.shape == same.shape == (nb, len(m), len(m))
        for k in range(nb):
            assert (cmp_[k] == want[k][0]).all() and (same[k] == want[k][1]).all(), (len(m), len(keep), seed, b0 + k)


@pytest.mark.parametrize("T", bin_.COUNT_TAXA)
def test_boot_counts(phy, T):
    """taxa around the 64 x 64 tile, kept columns around the 16-byte padding and beyond one LDS chunk; one replicate and five, from
    replicate 0 and from a later one, the largest seed; row 1 of the matrix is all '-'"""
    for K in bin_.COUNT_COLS:
        m = bin_.count_matrix(T, K + 9)
        keep = np.sort(np.random.RandomState(K).choice(K + 9, size=K, replace=False))
        check_counts(phy, m, keep, 2 ** 64 - 1, 0, 1)
        check_counts(phy, m, keep, 12345, 3, 5)
    m = bin_.count_matrix(T, 40)
    check_counts(phy, m, np.arange(40), 0, 2 ** 31 - 2, 2)                    # the last two replicates there are


def test_boot_counts_draw_the_literal_columns(phy):
    """one taxon pair, every column another letter pair: the counts name the drawn columns themselves"""
    K = 17
    m = np.stack([pin.AA[np.arange(K) % 20], pin.AA[np.arange(K) % 20]])
    m[1, ::2] = pin.AA[(np.arange(K)[::2] + 1) % 20]                           # even columns differ
    cmp_, same = phy.device_boot_counts(m, np.arange(K), 7, 5, 3)
    for k in range(3):
        draws = bin_.literal_columns(7, 5 + k, K)
        assert cmp_[k].tolist() == [[K, K], [K, K]] and same[k, 0, 1] == sum(1 for d in draws if d % 2 == 1)


# ---------------------------------------------------------------------------------------------------------
# so_phy_nj_splits
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nj_want(T, nb):
    from swiftortho_amd import phy
    D = bin_.nj_gpu_stack(T, nb)
    return D, np.stack([phy.nj_splits(D[k]) for k in range(nb)])


@pytest.mark.parametrize("T", bin_.NJ_GPU_TAXA)
def test_nj_splits(phy, T):
    """taxa around the words of the bit sets; random matrices (every rounding counts), additive trees, all-equal distances (every step a
    tie) and duplicated taxa (zero distances); one matrix and seven; the bit sets in the LDS and in global scratch"""
    for nb in (1, 7):
        D, want = nj_want(T, nb)
        for in_global in (False, True, False):
            got = phy.device_nj_splits(D, clades_in_global=in_global)
            assert got.dtype == np.uint64 and got.shape == want.shape == (nb, T - 3, (T + 63) // 64)
            assert (got == want).all(), (T, nb, in_global, np.argwhere((got != want).any(axis=(1, 2))).ravel().tolist())


def same_walk(got, want, label):
    """word for word; a mismatch names the input and the first join that differs"""
    assert got.dtype == np.uint64 and got.shape == want.shape, (label, got.shape, want.shape)
    assert (got == want).all(), (label, "first differing join, device words, numpy words:", bin_.first_difference(got, want))


@pytest.mark.parametrize("T", bin_.NJ_WIDE_TAXA)
def test_nj_splits_wide(phy, T):
    """more taxa than the walk has lanes: second and third passes of the row sums, the argmin, the new row and the live list, five to eleven
    clade words, and the two sides of the LDS limit -- 640 taxa ask for 58880 bytes of LDS, 641 would need 64100 and go to global scratch by
    themselves; nj_tier says which one ran"""
    D = bin_.nj_wide_stack(T)
    want = np.stack([bin_.nj_wide_want(T, k) for k in range(len(D))])
    assert want.shape == (4, T - 3, (T + 63) // 64)
    for in_global in (False, True):
        stats = {}
        got = phy.device_nj_splits(D, clades_in_global=in_global, stats=stats)
        assert stats == {"nj_tier": bin_.nj_tier(T, in_global)}, (T, in_global, stats)
        assert stats["nj_tier"] == (2 if in_global or T > 640 else 1)
        assert got.shape == want.shape
        for k, kind in enumerate(bin_.NJ_WIDE_KINDS):
            same_walk(got[k], want[k], (T, kind, "global" if in_global else "default"))
        assert set(bin_.as_tuples(got[bin_.NJ_WIDE_KINDS.index("additive")])) == bin_.additive_inner_splits(T), (T, in_global)


def test_nj_ties_across_a_lanes_columns(phy):
    """two cherries tie bit for bit; the winner has the lowest (row, column).  A lane owns columns b, b + 256, b + 512 and meets the loser
    before the winner, the winner before the loser, or the winner on the larger column; or the two sit in different waves.  The first two
    joins are the input file's literal sets; the rest of the walk (ties at every later step) is numpy's"""
    T = bin_.CHERRY_T
    D = np.stack([bin_.cherries(T, pairs) for pairs, _, _ in bin_.CHERRY_CASES])
    for in_global in (False, True):
        stats = {}
        got = phy.device_nj_splits(D, clades_in_global=in_global, stats=stats)
        assert stats == {"nj_tier": 2 if in_global else 1}
        for k, (pairs, first, second) in enumerate(bin_.CHERRY_CASES):
            assert bin_.as_tuples(got[k, :2]) == [bin_.canonical(first, T), bin_.canonical(second, T)], (pairs, in_global, bin_.as_tuples(got[k, :2]))
            same_walk(got[k], bin_.cherry_want(k), (T, pairs, in_global))


def test_nj_tier_of_the_narrow_calls(phy):
    """no walk below four taxa; the LDS where nothing asks otherwise; the scratch under the flag"""
    for T, in_global, want in ((3, False, 0), (3, True, 0), (4, False, 1), (4, True, 2), (129, False, 1)):
        stats = {}
        phy.device_nj_splits(bin_.nj_gpu_stack(T, 1) if T > 3 else np.zeros((1, 3, 3)), clades_in_global=in_global, stats=stats)
        assert stats == {"nj_tier": want} and want == bin_.nj_tier(T, in_global), (T, in_global, stats)


def test_nj_splits_small_cases(phy):
    for _, D in bin_.nj_cases():
        got = phy.device_nj_splits(D[None])
        assert bin_.as_tuples(got[0]) == bin_.literal_nj_splits(D.tolist())
    assert phy.device_nj_splits(np.zeros((2, 3, 3))).shape == (2, 0, 1)


def test_nj_splits_refusals(phy):
    good = bin_.nj_gpu_stack(9, 3)
    want = np.stack([phy.nj_splits(d) for d in good])
    cases = []
    for bad in (np.nan, np.inf):
        D = good.copy()
        D[1, 2, 4] = D[1, 4, 2] = bad
        cases.append((D, "not finite"))
    D = good.copy()
    D[2, 3, 5] = np.nextafter(D[2, 3, 5], 9.)
    cases += [(D, "not symmetric"), (np.zeros((1, 1, 1)), "taxa"), (np.zeros((1, 4097, 4097)), "taxa"), (np.zeros((0, 5, 5)), "matrices")]
    for D, word in cases:
        with pytest.raises(RuntimeError) as e:
            phy.device_nj_splits(D)
        assert word in str(e.value), (word, str(e.value))
        assert (phy.device_nj_splits(good) == want).all()


# ---------------------------------------------------------------------------------------------------------
# so_phy_boot
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def boot_want(key):
    from swiftortho_amd import phy
    _, sm, B, seed, _ = [c for c in bin_.boot_cases() if c[0] == key][0]
    return sm, B, seed, phy.bootstrap_replicates(sm, B, seed)


def same_boot(got, want):
    assert got[0].dtype == np.int32 and got[0].tolist() == want[0].tolist()
    assert got[1] == want[1] and got[2].tolist() == want[2].tolist()
    assert got[3].dtype == np.uint64 and got[3].shape == want[3].shape and (got[3] == want[3]).all()


@pytest.mark.parametrize("key", [c[0] for c in bin_.boot_cases()])
def test_boot(phy, key):
    sm, B, seed, want = boot_want(key)
    for _ in range(2):
        stats = {}
        same_boot(phy.bootstrap_replicates(sm, B, seed, device_stage=True, stats=stats), want)
        assert stats == {"waits": 1, "batches": 1}
    count, valid = phy.bootstrap(sm, B, seed, device_stage=True)
    assert count.tolist() == want[0].tolist() and valid == want[1]
    assert phy.tree(sm, boot=B, seed=seed, device_stage=True) == phy.tree(sm, boot=B, seed=seed)


@pytest.mark.parametrize("key", ["kept_with_holes", "sparse"])
def test_boot_batch_edges(phy, monkeypatch, key):
    """B = 7 in batches of 1, 3 and 7 (the sparse input: 12 in batches of 1, 5 and 12): the same results, a wait per batch"""
    sm, B, seed, want = boot_want(key)
    for batch in (1, 3 if B == 7 else 5, B, B + 9):
        monkeypatch.setenv("SOHIT_PHY_BOOT_BATCH", str(batch))
        stats = {}
        same_boot(phy.bootstrap_replicates(sm, B, seed, device_stage=True, stats=stats), want)
        n = -(-B // min(batch, B))
        assert stats == {"waits": n, "batches": n}


@pytest.mark.parametrize("key", ["conflict", "sparse", "T65"])
def test_boot_poisson(phy, monkeypatch, key):
    """the poisson path: counts and trees on the device, the logarithm on the host"""
    sm, B, seed, _ = boot_want(key)
    want = phy.bootstrap_replicates(sm, B, seed, "poisson")
    for batch in ("", "3"):
        monkeypatch.setenv("SOHIT_PHY_BOOT_BATCH", batch)
        same_boot(phy.bootstrap_replicates(sm, B, seed, "poisson", device_stage=True), want)
    monkeypatch.delenv("SOHIT_PHY_BOOT_BATCH")
    assert phy.tree(sm, "poisson", B, seed, True) == phy.tree(sm, "poisson", B, seed)


@pytest.mark.parametrize("T,K,B", bin_.WIDE_BOOT)
def test_boot_wide(phy, monkeypatch, T, K, B):
    """the fused path beyond one pass of the walk's lanes and beyond its LDS limit: replicates are dropped (their S * W > 256 zero words take
    more than one pass), two workgroups of k_phy_boot_support at 641 taxa; at 257 also in batches of 3, each of which starts on a dropped
    replicate, and the poisson path, whose trees are so_phy_nj_splits'"""
    sm, seed, want = bin_.wide_boot_want(T, K, B)
    assert 0 < want[1] < B and want[3].shape[1] * want[3].shape[2] > 256
    for batch in ("", "3") if T == 257 else ("",):
        monkeypatch.setenv("SOHIT_PHY_BOOT_BATCH", batch)
        stats = {"nj_tier": None}
        got = phy.bootstrap_replicates(sm, B, seed, device_stage=True, stats=stats)
        for b in np.flatnonzero(got[2] & want[2]).tolist():
            same_walk(got[3][b], want[3][b], (T, K, "replicate %d" % b, batch))
        same_boot(got, want)
        assert all((got[3][b] == 0).all() for b in range(B) if not want[2][b])
        n = -(-B // 3) if batch else 1
        assert stats == {"waits": n, "batches": n, "nj_tier": bin_.nj_tier(T)}, stats
    monkeypatch.delenv("SOHIT_PHY_BOOT_BATCH")
    if T == 257:
        want = bin_.wide_boot_want(T, K, B, "poisson")[2]
        assert want[1] > 0
        same_boot(phy.bootstrap_replicates(sm, B, seed, "poisson", device_stage=True), want)


def test_boot_refusals(phy):
    sm, B, seed, want = boot_want("conflict")
    T, L = sm.matrix.shape
    ref = phy.tree_splits(phy.distances(sm.cmp, sm.same))
    none = np.zeros(0, dtype=np.int64)
    wide = np.full((4097, 4), 65, dtype=np.uint8)
    cases = ((sm.matrix[:1], sm.keep, 3, ref[:0], "taxa"), (wide, np.arange(4), 3, np.zeros((4094, 65), dtype=np.uint64), "taxa"),
             (sm.matrix, none, 3, ref, "no kept column"), (sm.matrix, sm.keep, 0, ref, "replicate"), (sm.matrix, sm.keep, -4, ref, "replicate"),
             (sm.matrix, sm.keep, 2 ** 31, ref, "2^31"), (sm.matrix, np.append(sm.keep, L), 3, ref, "outside"), (sm.matrix, np.append(sm.keep, -1), 3, ref, "outside"))
    for m, keep, nb, r, word in cases:
        with pytest.raises(RuntimeError) as e:
            phy.device_boot(m, keep, seed, nb, r, True)
        assert word in str(e.value), (word, str(e.value))
        got = phy.device_boot(sm.matrix, sm.keep, seed, B, ref, True)
        same_boot(got, want)
        with pytest.raises(RuntimeError) as e:
            phy.device_boot_counts(m, keep, seed, 0, nb)
        assert word in str(e.value), (word, str(e.value))
        cmp_, same = phy.device_boot_counts(sm.matrix, sm.keep, seed, 2, 1)
        assert (cmp_[0] == phy.boot_counts(sm.matrix, sm.keep, seed, 2)[0]).all() and (same[0] == phy.boot_counts(sm.matrix, sm.keep, seed, 2)[1]).all()
    with pytest.raises(RuntimeError):
        phy.device_boot_counts(sm.matrix, sm.keep, seed, 2 ** 31 - 1, 2)            # replicate 2^31
    with pytest.raises(ValueError):
        phy.bootstrap(bin_.Sm(sm.matrix, keep=sm.keep[:0]), 3, device_stage=True)


# ---------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------
def test_end_to_end_script(phy, tmp_path):
    """the six-taxon proteome of test_gpu_phy.py through rbh2phy.py -A T -t x -B 16: -G T and -G F write the same bytes, and so does the
    one-process pipeline"""
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
    out = {}
    for g, boot in (("T", "16"), ("F", "16"), ("T", "0")):
        tree = str(tmp_path / ("x_%s%s.nwk" % (g, boot)))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "rbh2phy.py"), "-i", sc, "-f", p, "-A", "T", "-G", g, "-g", ".5", "-t", tree, "-B", boot],
                           capture_output=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out[g, boot] = (r.stdout, open(tree, "rb").read())
    assert out["T", "16"] == out["F", "16"] and out["T", "16"][0] == out["T", "0"][0]
    labels = re.findall(rb"\)([01]\.[0-9]{3}):", out["T", "16"][1])
    assert len(labels) == 3 and all(x in {b"%.3f" % (c / 16.) for c in range(17)} for x in labels)
    assert re.sub(rb"\)[01]\.[0-9]{3}:", b"):", out["T", "16"][1]) == out["T", "0"][1]
    from swiftortho_amd import pipeline
    newick, sm, t = pipeline.species_tree_from_search(p, gap_share=.5, boot=16, boot_seed=1, **SEARCH_KW)
    assert newick + b"\n" == out["T", "16"][1] and t["boot"] == 16 and 0 < t["boot_valid"] <= 16
    assert sm.matrix.shape[0] == 6 and phy.tree(sm, boot=16, device_stage=True) == newick
