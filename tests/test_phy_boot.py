"""The bootstrap of the species tree by its numpy definitions (swiftortho_amd/phy.py boot_columns, boot_counts, boot_distances, nj_splits,
tree_splits, split_support, bootstrap, the labelled Newick) against literal restatements in Python ints, floats and lists, and
scripts/rbh2phy.py -B.  No GPU is needed.  The inputs are tests/phy_boot_inputs.py's; tests/test_gpu_phy_boot.py holds the device to the
same definitions on the same inputs."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import phy_boot_inputs as bin_
import phy_inputs as pin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def phy():
    from swiftortho_amd import phy
    return phy


# ---------------------------------------------------------------------------------------------------------
# boot_columns, boot_counts, boot_distances
# ---------------------------------------------------------------------------------------------------------
def test_boot_columns_equal_the_literal_loop(phy):
    for seed in (0, 1, 2 ** 64 - 1):
        for b in (0, 2 ** 31 - 1):
            for K in (1, 2, 63, 1000):
                got = phy.boot_columns(seed, b, K)
                assert got.dtype == np.int64 and got.tolist() == bin_.literal_columns(seed, b, K), (seed, b, K)
                assert K != 1 or got.tolist() == [0]
    assert phy.boot_columns(5, 3, 0).tolist() == []
    draws = phy.boot_columns(1, 0, 1000)
    assert draws.min() >= 0 and draws.max() < 1000 and 580 <= len(set(draws.tolist())) <= 680      # (about 1 - 1 / e of the columns)
    assert phy.boot_columns(1, 1, 1000).tolist() != draws.tolist() and phy.boot_columns(2, 0, 1000).tolist() != draws.tolist()
    for bad in ((-1, 0, 5), (2 ** 64, 0, 5), (0, 2 ** 31, 5), (0, 0, 2 ** 31)):
        with pytest.raises(ValueError):
            phy.boot_columns(*bad)


def test_boot_counts_and_distances(phy):
    m = pin.gap_matrix(np.random.RandomState(3), 5, 40, .2)
    keep = np.asarray([0, 3, 4, 9, 10, 11, 20, 39])
    for b in (0, 6):
        cols = [int(keep[d]) for d in bin_.literal_columns(9, b, len(keep))]
        want = pin.literal_pair_counts(m, cols)
        got = phy.boot_counts(m, keep, 9, b)
        assert got[0].dtype == np.int64 and (got[0] == want[0]).all() and (got[1] == want[1]).all()
    cmp_, same = np.asarray([[4, 2], [2, 4]]), np.asarray([[4, 1], [1, 4]])
    D, ok = phy.boot_distances(cmp_, same, "p")
    assert ok is True and D.tolist() == [[0., .5], [.5, 0.]] and (D == phy.distances(cmp_, same, "p")).all()
    D, ok = phy.boot_distances(cmp_, same, "poisson")
    assert ok is True and (D == phy.distances(cmp_, same, "poisson")).all()
    assert phy.boot_distances([[4, 0], [0, 4]], [[4, 0], [0, 4]], "p")[1] is False               # no compared column: dropped under either model
    assert phy.boot_distances([[4, 0], [0, 4]], [[4, 0], [0, 4]], "poisson")[1] is False
    assert phy.boot_distances([[4, 2], [2, 4]], [[4, 0], [0, 4]], "p")[1] is True                # p = 1: a distance under p, none under poisson
    assert phy.boot_distances([[4, 2], [2, 4]], [[4, 0], [0, 4]], "poisson")[1] is False
    with pytest.raises(ValueError):
        phy.boot_distances(cmp_, same, "jc")


# ---------------------------------------------------------------------------------------------------------
# nj_splits
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bin_.nj_cases(), ids=lambda c: c[0])
def test_nj_splits_equal_the_literal_walk(phy, case):
    _, D = case
    T = len(D)
    got = phy.nj_splits(D)
    assert got.dtype == np.uint64 and got.shape == (max(T - 3, 0), (T + 63) // 64)
    assert bin_.as_tuples(got) == bin_.literal_nj_splits(D.tolist())


def test_nj_splits_word_edges_and_sum_order(phy):
    """65 taxa: a split has two words and the complement stops at bit T; the sequential row sums are what the literal loop adds up"""
    D = bin_.random_symmetric(65)
    assert bin_.as_tuples(phy.nj_splits(D)) == bin_.literal_nj_splits(D.tolist())
    s = phy.nj_splits(bin_.all_equal(65))
    assert s.shape == (62, 2) and (s[:, 0] & np.uint64(1) == 0).all() and (s[:, 1] <= np.uint64(1)).all()
    D = bin_.random_symmetric(200)
    assert (np.cumsum(D, axis=1)[:, -1] != D.sum(1)).any()           # the two orders differ: the definition has to name one


@pytest.mark.parametrize("T", [4, 5, 9, 30])
def test_nj_splits_recover_an_additive_tree(phy, T):
    edges, D = bin_.additive(T)
    want = {bin_.canonical(s, T) for s in pin.tree_splits(edges, T) if 1 < len(s) < T - 1}
    got = bin_.as_tuples(phy.nj_splits(D))
    assert len(got) == T - 3 and set(got) == want
    assert set(bin_.as_tuples(phy.tree_splits(D))) == want


def test_cherries_tie_to_the_lowest_row_then_column(phy):
    """two cherries with the same Q bit for bit: the literal walk joins the one of the lowest (row, column) first, then the other"""
    T = bin_.CHERRY_SMALL_T
    for pairs, first, second in bin_.CHERRY_SMALL_CASES:
        D = bin_.cherries(T, pairs)
        assert sorted(set(D[np.triu_indices(T, 1)].tolist())) == [2., 20.] and (D == D.T).all()
        walk = bin_.literal_nj_splits(D.tolist())
        assert walk[:2] == [bin_.canonical(first, T), bin_.canonical(second, T)], pairs
        assert bin_.as_tuples(phy.nj_splits(D)) == walk, pairs


def test_cherries_at_600_taxa(phy):
    """the same ties where a lane of the device's walk owns three columns: the definition gives the joins the input file states"""
    T = bin_.CHERRY_T
    for k, (pairs, first, second) in enumerate(bin_.CHERRY_CASES):
        got = bin_.as_tuples(bin_.cherry_want(k)[:2])
        assert got == [bin_.canonical(first, T), bin_.canonical(second, T)], pairs


@pytest.mark.parametrize("T", [257, 641])
def test_nj_splits_recover_a_wide_additive_tree(phy, T):
    """beyond 256 taxa and beyond the LDS limit of the device's walk: the additive member of the wide stack gives its own tree"""
    want = bin_.additive_inner_splits(T)
    got = bin_.as_tuples(bin_.nj_wide_want(T, bin_.NJ_WIDE_KINDS.index("additive")))
    assert len(want) == T - 3 and len(got) == T - 3 and set(got) == want


def test_wide_taxa_sit_on_the_walks_edges():
    """csrc/tune.h and csrc/phy.hip restated: 640 taxa are the last whose clade bit sets fit the LDS budget of the walk.  A change of
    PHY_NJ_LDS_BYTES, PHY_NJ_THREADS or nj_lds_bytes has to move NJ_WIDE_TAXA along"""
    tune = open(os.path.join(ROOT, "swiftortho_amd", "csrc", "tune.h")).read()
    assert int(re.search(r"#define PHY_NJ_THREADS (\d+)u", tune).group(1)) == bin_.NJ_THREADS == 256
    assert int(re.search(r"#define PHY_NJ_LDS_BYTES (\d+)u", tune).group(1)) == bin_.NJ_LDS_BYTES == 61440
    src = open(os.path.join(ROOT, "swiftortho_amd", "csrc", "phy.hip")).read()
    assert "return (size_t)T * 8u + (in_lds ? (size_t)T * W * 8u : 0u) + (size_t)T * 4u;" in src
    assert bin_.nj_lds_bytes(640) == 58880 <= bin_.NJ_LDS_BYTES < 64100 == bin_.nj_lds_bytes(641)
    assert bin_.nj_lds_bytes(641, False) == 641 * 12 and bin_.nj_lds_bytes(129) < 4700
    assert [bin_.nj_tier(T) for T in (3, 4, 640, 641)] == [0, 1, 1, 2] and bin_.nj_tier(4, True) == 2 and bin_.nj_tier(3, True) == 0
    T = bin_.NJ_WIDE_TAXA
    assert T == (255, 256, 257, 513, 640, 641) and [-(-t // 256) for t in T] == [1, 1, 2, 3, 3, 3] and [(t + 63) // 64 for t in T] == [4, 4, 5, 9, 10, 11]
    assert all(t - 3 > 256 for t, _, _ in bin_.WIDE_BOOT[1:]) and (257 - 3) * 5 > 256       # two workgroups of splits; a dropped replicate's zeros: two passes


def test_nj_splits_small_and_refusals(phy):
    assert phy.nj_splits(np.zeros((3, 3))).shape == (0, 1) and phy.nj_splits(np.zeros((2, 2))).shape == (0, 1)
    assert bin_.as_tuples(phy.nj_splits(bin_.two_minima())) == [(0b111100,), (0b001100,), (0b110000,)]      # (0, 1) first, the lowest of the equal minima: its clade holds taxon 0 and is complemented
    for bad in (np.nan, np.inf, -np.inf):
        D = bin_.additive(6)[1]
        D[2, 4] = D[4, 2] = bad
        with pytest.raises(ValueError):
            phy.nj_splits(D)
    with pytest.raises(ValueError):
        phy.nj_splits(np.zeros((3, 4)))


# ---------------------------------------------------------------------------------------------------------
# the labelled Newick
# ---------------------------------------------------------------------------------------------------------
def test_labelled_newick(phy):
    for T in (2, 3, 4, 7, 12):
        D = bin_.random_symmetric(T)
        names = [b"t%d" % k for k in range(T)]
        bare = phy.neighbor_joining(D, names)
        assert phy.neighbor_joining(D, names, None) == bare
        S = max(T - 3, 0)
        support = np.arange(S) / 8. + .0004
        lab = phy.neighbor_joining(D, names, support)
        assert re.sub(rb"\)[0-9.]+:", b"):", lab) == bare and lab.count(b")") == bare.count(b")")
        labels = re.findall(rb"\)([0-9.]+):", lab.replace(b");", b""))
        assert sorted(labels) == sorted(b"%.3f" % v for v in support) and len(labels) == S
        # the label of join t sits on the clade join t made: tree_splits in join order
        splits = bin_.as_tuples(phy.tree_splits(D))
        found = pin.newick_splits(re.sub(rb"\)[0-9.]+:", b"):", lab), [n.decode() for n in names])
        assert len(splits) == S and all(frozenset(k for k in range(T) if s[k // 64] >> (k % 64) & 1) in found for s in splits)
    lab = phy.neighbor_joining(bin_.additive(4)[1], [b"A", b"B", b"C", b"D"], [.95])
    assert re.fullmatch(rb"\(\([A-D]:[-0-9.]+,[A-D]:[-0-9.]+\)0\.950:[-0-9.]+,[A-D]:[-0-9.]+,[A-D]:[-0-9.]+\);", lab), lab
    with pytest.raises(ValueError):
        phy.neighbor_joining(bin_.additive(5)[1], [b"A", b"B", b"C", b"D", b"E"], [.5])


def test_label_sits_on_its_own_clade(phy):
    """every label is read back next to the clade it closes"""
    T = 9
    D = bin_.random_symmetric(T)
    names = ["t%d" % k for k in range(T)]
    splits = bin_.as_tuples(phy.tree_splits(D))
    lab = phy.neighbor_joining(D, names, [t / 10. for t in range(T - 3)]).decode()
    for t, s in enumerate(splits):
        at = lab.index(")%.3f:" % (t / 10.))
        depth, k = 0, at
        while True:                                  # back to the matching '('
            depth += {")": 1, "(": -1}.get(lab[k], 0)
            if depth == 0:
                break
            k -= 1
        inside = {int(x) for x in re.findall(r"t(\d+):", lab[k:at])}
        assert bin_.canonical(inside, T) == s


# ---------------------------------------------------------------------------------------------------------
# split_support, bootstrap
# ---------------------------------------------------------------------------------------------------------
def case(key):
    return [c for c in bin_.boot_cases() if c[0] == key][0]


def test_split_support(phy):
    ref = np.asarray([[2], [12], [48]], dtype=np.uint64)
    rep = np.asarray([[[12], [2], [7]], [[2], [12], [48]], [[48], [48], [48]], [[9], [9], [9]]], dtype=np.uint64)
    assert phy.split_support(ref, rep, [True, True, False, True]).tolist() == [2, 2, 1]
    got = phy.split_support(ref, rep, [True] * 4)
    assert got.dtype == np.int32 and got.tolist() == [2, 2, 2]
    two = np.asarray([[5, 1], [5, 2]], dtype=np.uint64)                        # equal first words: every word is compared
    assert phy.split_support(two, two[None, ::-1], [True]).tolist() == [1, 1] and phy.split_support(two, two[None, :1].repeat(2, 1), [True]).tolist() == [1, 0]


def test_one_tree_gets_full_support(phy):
    _, sm, B, seed, _ = case("one_tree")
    want = bin_.one_tree_matrix()[1]
    assert set(bin_.as_tuples(phy.tree_splits(phy.distances(sm.cmp, sm.same)))) == want
    count, valid = phy.bootstrap(sm, B, seed)
    assert valid == B and count.dtype == np.int32 and count.tolist() == [B] * (len(sm.taxa) - 3)
    nwk = phy.tree(sm, boot=B, seed=seed)
    assert nwk.count(b")1.000:") == len(sm.taxa) - 3 and re.sub(rb"\)1\.000:", b"):", nwk) == phy.tree(sm)


def test_conflict_equals_the_literal_count(phy):
    _, sm, B, seed, _ = case("conflict")
    ref = phy.tree_splits(phy.distances(sm.cmp, sm.same))
    count, ok, reps = bin_.literal_bootstrap(sm.matrix, sm.keep, B, seed, ref)
    got = phy.bootstrap_replicates(sm, B, seed)
    assert got[0].tolist() == count and got[1] == B and got[2].tolist() == ok
    assert [bin_.as_tuples(s) for s in got[3]] == reps
    at = bin_.as_tuples(ref).index(bin_.canonical({1, 2}, 6))                  # the 70 % split is in the printed tree, the 30 % one is not
    assert 0 < count[at] < B and count[bin_.as_tuples(ref).index(bin_.canonical({4, 5}, 6))] == B
    assert phy.bootstrap(sm, B, seed)[0].tolist() == count
    stats = {}
    assert (b")%.3f:" % (count[at] / float(B))) in phy.tree(sm, boot=B, seed=seed, stats=stats) and stats == {"boot": B, "boot_valid": B}


def test_sparse_matrix_drops_replicates(phy):
    _, sm, B, seed, _ = case("sparse")
    ref = phy.tree_splits(phy.distances(sm.cmp, sm.same))
    count, ok, reps = bin_.literal_bootstrap(sm.matrix, sm.keep, B, seed, ref)
    got = phy.bootstrap_replicates(sm, B, seed)
    assert got[2].tolist() == ok and 0 < got[1] == sum(ok) < B and got[0].tolist() == count
    assert all((got[3][b] == 0).all() for b in range(B) if not ok[b])
    c, valid = phy.bootstrap(sm, B, seed)
    assert c.tolist() == count and valid == sum(ok)
    for model in ("p", "poisson"):
        c, valid = phy.bootstrap(sm, B, seed, model)
        assert valid <= sum(ok) and (c <= valid).all()


@pytest.mark.parametrize("T,K,B", bin_.WIDE_BOOT)
def test_wide_boot_cases_drop_and_keep(phy, T, K, B):
    """what the device test of these inputs rests on, from the numpy reference alone: the two last taxa share one compared column; a
    replicate is dropped, one is kept, and a split of the printed tree is counted"""
    sm, seed, (count, valid, ok, splits) = bin_.wide_boot_want(T, K, B)
    assert sm.cmp[T - 2, T - 1] == 1 and (sm.cmp > 0).all()
    assert 0 < valid == int(ok.sum()) < B and (count > 0).any() and (count <= valid).all()
    assert all((splits[b] == 0).all() == (not ok[b]) for b in range(B)) and splits.shape[1] * splits.shape[2] > 256
    if (T, K, B) == (257, 96, 8):
        assert ok.tolist() == [False, True, True, False, True, True, False, True]         # batches of 3: each starts on a dropped replicate
        assert 0 < bin_.wide_boot_want(T, K, B, "poisson")[2][1] <= valid
    else:
        assert ok.tolist() == [False, True, True]


def test_every_other_input_keeps_every_replicate(phy):
    """what lets the device tests compare counts: no replicate of these inputs is dropped, so none can be dropped to pass"""
    for key, sm, B, seed, all_valid in bin_.boot_cases():
        got = phy.bootstrap_replicates(sm, B, seed)
        assert (got[1] == B) == all_valid, key
        assert got[0].shape == (max(len(sm.taxa) - 3, 0),) and (got[0] <= got[1]).all()


def test_bootstrap_refusals(phy):
    _, sm, B, seed, _ = case("conflict")
    for bad in (0, -1, 2 ** 31):
        with pytest.raises(ValueError):
            phy.bootstrap(sm, bad)
    none = bin_.Sm(np.full((4, 6), 45, dtype=np.uint8))
    none.cmp = none.cmp + 1                                                   # (a printed tree, and no replicate with a distance)
    with pytest.raises(ValueError) as e:
        phy.bootstrap(none, 3)
    assert "none of the 3 replicates" in str(e.value)
    empty = bin_.Sm(bin_.conflict_matrix(), keep=[])
    empty.cmp, empty.same = sm.cmp, sm.same
    with pytest.raises(ValueError):
        phy.bootstrap(empty, 3)


# ---------------------------------------------------------------------------------------------------------
# scripts/rbh2phy.py -B
# ---------------------------------------------------------------------------------------------------------
def run_script(tmp_path, extra=()):
    fasta, sc = bin_.script_case()
    p, f = str(tmp_path / "x.sc"), str(tmp_path / "x.fsa")
    open(p, "wb").write(sc), open(f, "wb").write(fasta)
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "rbh2phy.py"), "-i", p, "-f", f, "-A", "T"] + list(extra), capture_output=True)


def test_script_labels(tmp_path):
    tree = str(tmp_path / "x.nwk")
    bare = run_script(tmp_path, ("-t", tree))
    assert bare.returncode == 0, bare.stderr
    today = open(tree, "rb").read()
    assert today.count(b"(") == 3 and not re.search(rb"\)[0-9.]+:", today)
    for flags in (("-B", "0"), ("-B", "0", "-S", "7"), ("-B0",)):
        r = run_script(tmp_path, ("-t", tree) + flags)
        assert r.returncode == 0 and r.stdout == bare.stdout and open(tree, "rb").read() == today
    r = run_script(tmp_path, ("-t", tree, "-B", "8"))
    assert r.returncode == 0, r.stderr
    lab = open(tree, "rb").read()
    assert r.stdout == bare.stdout and len(re.findall(rb"\)[01]\.[0-9]{3}:", lab)) == 2 and re.sub(rb"\)[01]\.[0-9]{3}:", b"):", lab) == today
    again = run_script(tmp_path, ("-t", tree, "-B", "8", "-S", "1"))
    assert again.returncode == 0 and open(tree, "rb").read() == lab


def test_script_refusals(tmp_path):
    tree = str(tmp_path / "x.nwk")
    for flags in (("-B", "8"), ("-t", tree, "-B", "-1"), ("-t", tree, "-B", "1.5"), ("-t", tree, "-B", "many"), ("-t", tree, "-B", str(2 ** 31)),
                  ("-t", tree, "-B", "8", "-S", "-1"), ("-t", tree, "-B", "8", "-S", str(2 ** 64)), ("-t", tree, "-B", "8", "-S", "x")):
        r = run_script(tmp_path, flags)
        assert r.returncode == 2 and r.stdout == b"" and r.stderr.startswith(b"rbh2phy: -B"), (flags, r.stderr)
        assert not os.path.exists(tree)


# ---------------------------------------------------------------------------------------------------------
# batch_size and replicate_trees: how many items a device call takes, and the one loop every replicate and family goes through
# ---------------------------------------------------------------------------------------------------------
def test_batch_size(phy, monkeypatch):
    env = "SOHIT_PHY_BOOT_BATCH"
    monkeypatch.delenv(env, raising=False)
    assert phy.batch_size(5000, 1 << 20) == 1024 and phy.batch_size(5000, 1 << 20, env) == 1024      # what 2^30 bytes hold
    assert phy.batch_size(5, 1 << 20) == 5 and phy.batch_size(0, 1 << 20) == 1                          # n below it; one at least
    assert phy.batch_size(10 ** 6, 1) == 32768 and phy.batch_size(10 ** 6, 0) == 32768 and phy.batch_size(10, 0) == 10   # the cap; bytes_each = 0
    monkeypatch.setenv(env, "7")
    assert phy.batch_size(5000, 1 << 20, env) == 7 and phy.batch_size(5, 1 << 20, env) == 5 and phy.batch_size(5000, 0, env) == 7
    assert phy.batch_size(5000, 1 << 20) == 1024 and phy.batch_size(5000, 1 << 20, "SOHIT_PHY_GENE_BATCH") == 1024      # (another switch, or none)
    monkeypatch.setenv(env, "1000000")
    assert phy.batch_size(10 ** 6, 1 << 20, env) == 32768
    for off in ("0", "-3", ""):
        monkeypatch.setenv(env, off)
        assert phy.batch_size(5000, 1 << 20, env) == 1024


def _trees(phy, T, n, step, drop=()):
    """replicate_trees over n replicates of a T-taxon matrix with numpy callbacks; a replicate in `drop` has no distance ->
    (ok, splits, calls, the calls counts_of reported, the idx of every walk call)"""
    m = pin.gap_matrix(np.random.RandomState(11), T, 60, .1)
    keep = np.arange(60)
    made, walks = [], []

    def counts_of(i0, k):
        made.append(1 + i0 % 2)
        return [(b,) + phy.boot_counts(m, keep, 4, b) for b in range(i0, i0 + k)], made[-1]

    def distance_of(batch, j):
        b, cmp_, same = batch[j]
        D, ok = phy.boot_distances(cmp_, same, "p")
        return D, ok and b not in drop

    def trees_of(D, idx):
        walks.append(list(idx))
        return np.stack([phy.nj_splits(d) for d in D])
    S, W = max(T - 3, 0), (T + 63) // 64
    ok, splits, calls = phy.replicate_trees(n, step, counts_of, distance_of, trees_of, S, W)
    assert ok.dtype == bool and ok.shape == (n,) and splits.dtype == np.uint64 and splits.shape == (n, S, W)
    # the literal loop, item by item
    for b in range(n):
        D, good = phy.boot_distances(*phy.boot_counts(m, keep, 4, b), model="p")
        good = good and b not in drop
        assert bool(ok[b]) is good and (splits[b] == (phy.nj_splits(D) if good else 0)).all(), (T, n, step, b)
    return ok, splits, calls, made, walks


def test_replicate_trees_any_step_gives_the_literal_loop(phy):
    first = None
    for step in (1, 3, 7):
        ok, splits, calls, made, walks = _trees(phy, 5, 7, step, drop=(2,))
        assert ok.tolist() == [True, True, False, True, True, True, True] and splits[:2].any() and not splits[2].any()
        assert len(made) == -(-7 // step) and len(walks) == len(made) - (step == 1) and calls == sum(made) + len(walks)   # (step 1: the dropped one is a batch)
        assert sorted(sum(walks, [])) == [0, 1, 3, 4, 5, 6]
        first = first or (ok, splits)
        assert (ok == first[0]).all() and (splits == first[1]).all()


def test_replicate_trees_walk_only_where_a_tree_is_due(phy):
    ok, splits, calls, made, walks = _trees(phy, 5, 7, 3, drop=(3, 4, 5))          # the middle batch has no item left: no walk call, zeros
    assert walks == [[0, 1, 2], [6]] and calls == sum(made) + 2 and not ok[3:6].any() and not splits[3:6].any() and ok[[0, 1, 2, 6]].all()
    ok, splits, calls, made, walks = _trees(phy, 3, 7, 3)                           # three taxa: no split, no walk call at all
    assert walks == [] and calls == sum(made) and ok.all() and splits.shape == (7, 0, 1)
    ok, splits, calls, made, walks = _trees(phy, 5, 0, 3)                           # nothing to do
    assert made == [] and walks == [] and calls == 0 and ok.shape == (0,)
