"""The gene concordance factors on the GPU (csrc/phy.hip, include/sohit.h so_phy_gene / so_phy_gene_counts / so_phy_nj_subsets) against the
numpy definitions (swiftortho_amd/phy.py) array for array and bit set for bit set, on the designed inputs of tests/phy_gene_inputs.py:
device memory poisoned, every call twice in one process, the tile and word edges of the taxa, both tiers of the walk, every family width
around the 16-byte padding and beyond one LDS chunk, every batch edge, every refusal; then tree(concordance=True), scripts/rbh2phy.py -K
and the one-process pipeline with and without the device: the same bytes.

Observed on an MI355X, numpy reference included (it is nearly all of it): test_gene_wide 1.5 s at 640 taxa and 1.6 s at 641,
test_script_with_and_without_the_device 0.6 s, every other test below 0.25 s; the module 5.4 s.  No path disagreed with numpy.

Run on the GPU box:  python -m pytest tests/test_gpu_phy_gene.py -m gpu -q
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import phy_boot_inputs as bin_
import phy_gene_inputs as gin
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
    monkeypatch.delenv("SOHIT_PHY_GENE_BATCH", raising=False)


@functools.lru_cache(maxsize=None)
def want(key, arg=None):
    """the numpy definitions on a designed input, computed once per process -> (case, fam_off, ref, present, (decisive, concordant, ok,
    n_present, splits))"""
    from swiftortho_amd import phy
    case = getattr(gin, key)(*(() if arg is None else (arg,)))
    case = case[0] if isinstance(case, tuple) else case
    T = len(case.taxa)
    r = phy.family_ranges(case.keep, case.col_off)
    ref = phy.tree_splits(phy.distances(case.cmp, case.same))
    res = phy.gene_concordance(case, want_splits=True)
    present = np.zeros((len(r) - 1, (T + 63) // 64), dtype=np.uint64)
    for f in range(len(r) - 1):
        present[f] = phy.family_present(phy.pair_counts(case.matrix, case.keep[r[f]:r[f + 1]])[0])
    return case, r, ref, present, res


def same_gene(got, wanted, present):
    """(decisive, concordant, ok, n_present, present, splits) of device_gene against the definitions"""
    dec, con, ok, npres, splits = wanted
    assert got[0].dtype == got[1].dtype == got[3].dtype == np.int32 and got[2].dtype == bool
    assert np.array_equal(got[2], ok) and np.array_equal(got[3], npres)
    assert got[4].dtype == np.uint64 and np.array_equal(got[4], present)
    assert got[5].dtype == np.uint64 and got[5].shape == splits.shape
    for f in range(len(ok)):
        assert np.array_equal(got[5][f], splits[f]), ("family", f, bin_.first_difference(got[5][f], splits[f]))
    assert np.array_equal(got[0], dec) and np.array_equal(got[1], con)


def fused(phy, key, arg=None, **kw):
    case, r, ref, present, res = want(key, arg)
    stats = {}
    got = phy.device_gene(case.matrix, case.keep, r, ref, want_splits=True, stats=stats, **kw)
    same_gene(got, res, present)
    return stats


# ---------------------------------------------------------------------------------------------------------
# so_phy_gene: the fused call
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", gin.GPU_TAXA)
def test_gene_edges(phy, T):
    """the tile and word edges of the taxa; families on A and on B, lacking taxon 0, lacking the last taxon of a word, with exactly 3 and
    exactly 4 present taxa, with no kept column and a dropped one"""
    case, _, _, present, res = want("edge_case", T)
    assert int((~res[2]).sum()) == 1 and res[3][case.names.index("three")] == 3 and res[3][case.names.index("four")] == 4
    assert res[3][case.names.index("empty")] == 0 and not (present[case.names.index("no_taxon0")][0] & np.uint64(1))
    for _ in range(2):
        stats = fused(phy, "edge_case", T)
        assert stats == {"waits": 1, "batches": 1, "nj_tier": 1}
    without = phy.device_gene(case.matrix, case.keep, want("edge_case", T)[1], want("edge_case", T)[2])
    assert without[4] is None and without[5] is None and np.array_equal(without[0], res[0]) and np.array_equal(without[1], res[1])


def test_gene_hand_table(phy):
    fused(phy, "hand_case")
    fused(phy, "ghost_case")


@pytest.mark.parametrize("T", gin.WIDE_TAXA)
def test_gene_wide(phy, T):
    """the two sides of the walk's LDS tier: 640 taxa keep the clade bit sets in the LDS, 641 in global scratch"""
    stats = fused(phy, "wide_case", T)
    assert stats["nj_tier"] == bin_.nj_tier(T) == (1 if T == 640 else 2)


def test_gene_widths(phy):
    """families of 0, 1, 15, 16, 17, 63, 64, 65 and 3000 kept columns on a table whose rows all differ, keep with holes"""
    case, r, _, _, _ = want("width_case")
    assert np.diff(r).tolist() == list(gin.WIDTHS)
    fused(phy, "width_case")
    fused(phy, "width_case", timed=True)


@pytest.mark.parametrize("F", (1, gin.FORCED_BATCH, gin.FORCED_BATCH + 1))
def test_gene_batch_edges(phy, monkeypatch, F):
    """F = 1, F at the forced batch size and one more: the same results, a wait per batch"""
    assert fused(phy, "batch_case", F) == {"waits": 1, "batches": 1, "nj_tier": 1}
    monkeypatch.setenv("SOHIT_PHY_GENE_BATCH", str(gin.FORCED_BATCH))
    n = -(-F // gin.FORCED_BATCH)
    assert fused(phy, "batch_case", F) == {"waits": n, "batches": n, "nj_tier": 1}


# ---------------------------------------------------------------------------------------------------------
# so_phy_gene_counts, so_phy_nj_subsets, and the three-call path
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,arg", [("width_case", None), ("edge_case", 65), ("edge_case", 130), ("hand_case", None)])
def test_gene_counts(phy, key, arg):
    case, r, _, _, _ = want(key, arg)
    F = len(r) - 1
    wc, ws = phy.family_counts(case.matrix, case.keep, case.col_off)
    for _ in range(2):
        cmp_, same = phy.device_gene_counts(case.matrix, case.keep, r)
        assert cmp_.dtype == same.dtype == np.int64 and np.array_equal(cmp_, wc) and np.array_equal(same, ws)
    for f0, nf in ((0, 1), (F - 1, 1), (1, F - 2)):
        cmp_, same = phy.device_gene_counts(case.matrix, case.keep, r, f0, nf)
        assert np.array_equal(cmp_, wc[f0:f0 + nf]) and np.array_equal(same, ws[f0:f0 + nf])


@pytest.mark.parametrize("T", bin_.NJ_GPU_TAXA)
def test_nj_subsets_with_every_taxon_is_nj_splits(phy, T):
    D = bin_.nj_gpu_stack(T, 3)
    full = np.zeros((3, (T + 63) // 64), dtype=np.uint64)
    for t in range(T):
        full[:, t >> 6] |= np.uint64(1 << (t & 63))
    for in_global in (False, True):
        stats = {}
        got = phy.device_nj_subsets(D, full, clades_in_global=in_global, stats=stats)
        assert np.array_equal(got, phy.device_nj_splits(D, clades_in_global=in_global)) and stats == {"nj_tier": 2 if in_global else 1}


@pytest.mark.parametrize("T", (9, 65, 130))
def test_nj_subsets_on_random_matrices(phy, T):
    """every rounding counts: random symmetric matrices, NaN outside present x present (never read), subsets that lack taxon 0, the last
    taxon of a word, all but 3 and all but 4 taxa"""
    rng = np.random.RandomState(T)
    subsets = [list(range(1, T)), [t for t in range(T) if t != min(63, T - 1)], sorted(rng.choice(T, size=T // 2, replace=False).tolist()), [1, 4, T - 1], [0, 2, 3, T - 2]]
    D = np.stack([bin_.random_symmetric(T, seed=k) for k in range(len(subsets))])
    present = np.zeros((len(subsets), (T + 63) // 64), dtype=np.uint64)
    for k, sub in enumerate(subsets):
        out = np.ones(T, dtype=bool)
        out[sub] = False
        D[k][out, :] = np.nan
        D[k][:, out] = np.nan
        for t in sub:
            present[k, t >> 6] |= np.uint64(1 << (t & 63))
    wanted = np.stack([phy.nj_splits_subset(np.nan_to_num(D[k]), present[k]) for k in range(len(subsets))])
    for in_global in (False, True):
        got = phy.device_nj_subsets(D, present, clades_in_global=in_global)
        for k in range(len(subsets)):
            assert np.array_equal(got[k], wanted[k]), (T, k, in_global, bin_.first_difference(got[k], wanted[k]))


@pytest.mark.parametrize("model", ("poisson", "kimura"))
def test_three_call_path_equals_the_fused_call_and_numpy(phy, monkeypatch, model):
    """poisson and kimura: counts and trees on the device, the logarithm on the host; with model p forced down the same road the three
    calls give what the fused call gives"""
    case = gin.hand_case()[0]
    wanted = phy.gene_concordance(case, model, want_splits=True)
    for batch in ("", "2"):
        monkeypatch.setenv("SOHIT_PHY_GENE_BATCH", batch)
        got = phy.gene_concordance(case, model, device_stage=True, want_splits=True)
        assert all(np.array_equal(g, w) for g, w in zip(got, wanted))
    monkeypatch.delenv("SOHIT_PHY_GENE_BATCH")
    for key, arg in (("hand_case", None), ("edge_case", 65)):
        case, r, ref, present, res = want(key, arg)
        cmp_, same = phy.device_gene_counts(case.matrix, case.keep, r)
        pres = phy.family_present(cmp_)
        dist = [phy.gene_distances(cmp_[f], same[f], pres[f]) for f in range(len(pres))]
        ok = np.array([d[1] for d in dist])
        splits = np.zeros_like(res[4])
        splits[ok] = phy.device_nj_subsets(np.stack([d[0] for d, g in zip(dist, ok) if g]), pres[ok])
        dec, con = phy.concordance(ref, pres, splits, ok)
        same_gene((dec, con, ok, phy._popcount(pres).astype(np.int32), pres, splits), res, present)


# ---------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------
def test_gene_refusals(phy):
    case, r, ref, present, res = want("hand_case")
    T, L = case.matrix.shape
    wide = np.full((4097, 4), 65, dtype=np.uint8)
    bad_keep = case.keep.copy()
    bad_keep[3] = L
    neg_keep = case.keep.copy()
    neg_keep[0] = -1
    falls = r.copy()
    falls[2] = falls[3] + 1
    cases = ((case.matrix[:1], case.keep, r, ref[:0], "taxa"), (wide, np.arange(4), np.array([0, 4]), np.zeros((4094, 65), dtype=np.uint64), "taxa"),
             (case.matrix, case.keep, r + 1, ref, "fam_off"), (case.matrix, case.keep, np.append(r[:-1], r[-1] - 1), ref, "fam_off"), (case.matrix, case.keep, falls, ref, "fam_off"),
             (case.matrix, case.keep, r[:1], ref, "families"), (case.matrix, bad_keep, r, ref, "outside"), (case.matrix, neg_keep, r, ref, "outside"))
    for m, keep, off, rf, word in cases:
        with pytest.raises(RuntimeError) as e:
            phy.device_gene(m, keep, off, rf, True)
        assert word in str(e.value), (word, str(e.value))
        same_gene(phy.device_gene(case.matrix, case.keep, r, ref, True), res, present)
        with pytest.raises(RuntimeError) as e:
            phy.device_gene_counts(m, keep, off)
        assert word in str(e.value), (word, str(e.value))
    from swiftortho_amd import _lib
    import ctypes as C
    Lb = _lib.load()
    ptr = lambda a: C.c_void_p(np.ascontiguousarray(a).ctypes.data)
    out = _lib.SoPhyGeneResult()
    for flags in (4, -1):
        assert Lb.so_phy_gene(0, T, L, ptr(case.matrix), len(case.keep), ptr(case.keep), len(r) - 1, ptr(r), ptr(ref), flags, C.byref(out)) == 1
        assert b"unknown flag bits" in Lb.so_phy_last_error() and not out.ok
    assert Lb.so_phy_gene_counts(0, T, L, ptr(case.matrix), len(case.keep), ptr(case.keep), len(r) - 1, ptr(r), 0, 1, 1, C.byref(out)) == 1
    assert b"unknown flag bits" in Lb.so_phy_last_error()
    assert Lb.so_phy_gene(99, T, L, ptr(case.matrix), len(case.keep), ptr(case.keep), len(r) - 1, ptr(r), ptr(ref), 0, C.byref(out)) == 1
    assert b"device" in Lb.so_phy_last_error()
    for f0, nf in ((0, 0), (-1, 2), (len(r) - 1, 1), (2, len(r))):
        with pytest.raises(RuntimeError) as e:
            phy.device_gene_counts(case.matrix, case.keep, r, f0, nf)
        assert "families" in str(e.value)
    good_D = np.stack([bin_.random_symmetric(9, seed=1)])
    some = np.array([[0b110110110]], dtype=np.uint64)
    wanted = phy.nj_splits_subset(good_D[0], some[0])
    for D, P, word in ((np.zeros((1, 1, 1)), np.ones((1, 1), dtype=np.uint64), "taxa"), (np.zeros((0, 5, 5)), np.zeros((0, 1), dtype=np.uint64), "matrices"),
                       (good_D, np.array([[1 << 9]], dtype=np.uint64), "beyond")):
        with pytest.raises(RuntimeError) as e:
            phy.device_nj_subsets(D, P)
        assert word in str(e.value), (word, str(e.value))
    for bad, word in ((np.nan, "not finite"), (np.inf, "not finite"), (None, "not symmetric")):
        D = good_D.copy()
        if bad is None:
            D[0, 2, 4] = np.nextafter(D[0, 2, 4], 9.)
        else:
            D[0, 2, 4] = D[0, 4, 2] = bad
        with pytest.raises(RuntimeError) as e:
            phy.device_nj_subsets(D, some)
        assert word in str(e.value)
        D[0, 2, 4], D[0, 4, 2] = good_D[0, 2, 4], good_D[0, 4, 2]
        D[0, 0, 4] = D[0, 3, 0] = np.nan if bad is None else bad        # outside present x present: never read
        assert np.array_equal(phy.device_nj_subsets(D, some)[0], wanted)


# ---------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------
def test_tree_labels_are_the_same_bytes(phy):
    for key, arg in (("hand_case", None), ("edge_case", 65)):
        case = want(key, arg)[0]
        for kw in (dict(), dict(boot=6), dict(model="kimura"), dict(model="poisson", boot=4)):
            assert phy.tree(case, concordance=True, device_stage=True, **kw) == phy.tree(case, concordance=True, **kw), (key, kw)
    with pytest.raises(phy.ConcordanceRefused):
        phy.tree(want("hand_case")[0], "logdet", concordance=True, device_stage=True)


def test_script_with_and_without_the_device(tmp_path):
    fasta, sc = gin.script_case()
    p, f = str(tmp_path / "x.sc"), str(tmp_path / "x.fsa")
    open(p, "wb").write(sc), open(f, "wb").write(fasta)
    out = {}
    for g in ("T", "F"):
        tree, tsv = str(tmp_path / ("x_%s.nwk" % g)), str(tmp_path / ("x_%s.tsv" % g))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "rbh2phy.py"), "-i", p, "-f", f, "-A", "T", "-G", g, "-t", tree, "-K", "T", "-k", tsv, "-B", "5"],
                           capture_output=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out[g] = (r.stdout, open(tree, "rb").read(), open(tsv, "rb").read())
    assert out["T"] == out["F"] and out["T"][1].count(b"/") == 7 and out["T"][2].count(b"\n") == 8


def test_pipeline_with_and_without_the_device(phy, tmp_path):
    """the six-taxon proteome of test_gpu_phy.py: one process from the FASTA file to the labelled tree"""
    from swiftortho_amd import pipeline
    from test_gpu_phy import SEARCH_KW
    p = str(tmp_path / "x.fsa")
    open(p, "wb").write(pin.six_taxa_proteome())
    newick, sm, t = pipeline.species_tree_from_search(p, gap_share=.5, concordance=True, **SEARCH_KW)
    again, _, t2 = pipeline.species_tree_from_search(p, gap_share=.5, concordance=True, device_stage=False, **SEARCH_KW)
    assert newick == again and np.array_equal(t["gcf"]["decisive"], t2["gcf"]["decisive"]) and np.array_equal(t["gcf"]["concordant"], t2["gcf"]["concordant"])
    assert t["gcf"]["decisive"].max() > 0 and newick == phy.tree(sm, concordance=True) and newick != phy.tree(sm)
    bare, _, t3 = pipeline.species_tree_from_search(p, gap_share=.5, **SEARCH_KW)
    assert bare == phy.tree(sm) and "gcf" not in t3
