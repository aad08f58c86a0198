"""The component stage of `find_cluster -a mcl` on the CPU: find_cluster.group_numbers() is the numpy definition pulled out of cnc(); a
plain-Python restatement of the closed form the device kernels compute (tests/cnc_inputs.py `closed_form`) equals it on every generator
input and on seeded random graphs, and every single deviation of that restatement is told apart by a named input.  All comparisons are
integer or boolean and exact.  The refusals of so_cnc_groups that come before anything touches a device are checked here too."""
import json
import os

import numpy as np
import pytest

import cnc_inputs as ci
from conftest import GOLD
from mcl_scipy_oracle import scipy_mcl
from test_find_cluster import cluster_cases

N_RANDOM = 2000


def original_lines(X, Y, Z, n):
    """the lines cnc() ran before group_numbers() was pulled out of it, word for word"""
    from swiftortho_amd.find_cluster import _numbered_components
    nrow = len(X)
    best = np.full(n, -np.inf)
    np.maximum.at(best, X, Z)
    np.maximum.at(best, Y, Z)
    a = np.concatenate([X, Y])
    b = np.concatenate([Y, X])
    ridx = np.concatenate([np.arange(nrow) * 2, np.arange(nrow) * 2 + 1])   # (x, y) of a row before its (y, x)
    tie = np.concatenate([Z, Z]) == best[a]
    a, b, ridx = a[tie], b[tie], ridx[tie]
    o = np.lexsort((ridx, -a))
    genes1, comp1_of_node = _numbered_components(a[o], b[o])
    comp1 = np.zeros(n, dtype=np.int64)
    comp1[genes1] = comp1_of_node
    cX, cY = comp1[X], comp1[Y]
    m = (cX != 0) & (cY != 0)
    k0, k1 = np.minimum(cX[m], cY[m]), np.maximum(cX[m], cY[m])
    nc = int(comp1.max()) + 2
    key = k0 * nc + k1
    _, first = np.unique(key, return_index=True)
    first.sort()
    nodes2, comp2_of_node = _numbered_components(k0[first], k1[first])
    group_of_comp = np.full(nc, -1, dtype=np.int64)
    group_of_comp[nodes2] = comp2_of_node
    grp = group_of_comp[comp1]
    return comp1, grp


def same(got, X, Y, comp1, grp):
    return np.array_equal(got[0], comp1) and np.array_equal(got[1], grp) and np.array_equal(got[2], ci.keep_rows(X, Y, grp))


@pytest.mark.parametrize("name", sorted(ci.inputs()))
def test_group_numbers_and_closed_form_on_the_generator(name):
    from swiftortho_amd import find_cluster as fc
    X, Y, Z, n = ci.inputs()[name]
    comp1, grp = fc.group_numbers(X, Y, Z, n)
    assert comp1.dtype == np.int64 and grp.dtype == np.int64 and len(comp1) == len(grp) == n
    if len(X):
        want = original_lines(X, Y, Z, n)
        assert np.array_equal(comp1, want[0]) and np.array_equal(grp, want[1])
        assert sorted(set(np.concatenate([X, Y]).tolist())) == list(range(n))            # every gene occurs in some row ...
        seq = np.stack([X, Y], 1).reshape(-1)
        assert np.array_equal(seq[np.sort(np.unique(seq, return_index=True)[1])], np.arange(n))   # ... numbered by first appearance
    else:
        assert n == 0 and len(comp1) == 0
    assert same(ci.closed_form(X, Y, Z, n), X, Y, comp1, grp)


def test_closed_form_on_random_small_graphs():
    from swiftortho_amd import find_cluster as fc
    ties = selfs = repeats = merged = 0
    for seed in range(N_RANDOM):
        X, Y, Z, n = ci.random_small(seed)
        comp1, grp = fc.group_numbers(X, Y, Z, n)
        want = original_lines(X, Y, Z, n)
        assert np.array_equal(comp1, want[0]) and np.array_equal(grp, want[1]), seed
        assert same(ci.closed_form(X, Y, Z, n), X, Y, comp1, grp), seed
        ties += len(Z) > len(set(Z.tolist()))
        selfs += bool(np.any(X == Y))
        repeats += len(set(zip(X.tolist(), Y.tolist()))) < len(X)
        merged += bool(np.any(grp > 0))
    assert ties > N_RANDOM // 2 and selfs > N_RANDOM // 4 and repeats > N_RANDOM // 4 and merged > N_RANDOM // 20


def test_the_inputs_hold_what_they_promise():
    from swiftortho_amd import find_cluster as fc
    I = ci.inputs()
    res = {k: fc.group_numbers(*v) for k, v in I.items() if len(v[0])}
    for k in (2, 63, 64, 65, 257, 5000):
        for order in ("up", "down", 7):
            X, Y, Z, n = I["chain%d_%s" % (k, order)]
            assert n == k and len(X) == k - 1 and not res["chain%d_%s" % (k, order)][0].any()      # one level-1 component
        up, down, mixed = (I["chain%d_%s" % (k, o)] for o in ("up", "down", 7))
        assert np.all(up[1] == up[0] + 1) and np.all(down[1] == down[0] + 1)
        assert up[2][0] == 1.0 and (k == 2 or down[2][0] == float(k - 1))                           # rising / falling along the gene numbers
        assert k < 63 or np.any(np.abs(mixed[0] - mixed[1]) != 1)
    for leaves in (64, 65, 1025):
        a, b = I["star%d_hub0" % leaves], I["star%d_hub_last" % leaves]
        assert a[3] == b[3] == leaves + 1 and np.all(a[0] == 0) and np.all(b[0][-leaves:] == leaves)
        assert not res["star%d_hub0" % leaves][0].any() and not res["star%d_hub_last" % leaves][0].any()
    assert I["complete40"][3] == 40 and len(I["complete40"][0]) == 780
    for v in (255, 256, 257, 1023, 1024, 1025):
        assert I["genes%d" % v][3] == v and len(I["rows%d" % v][0]) == v
        assert res["genes%d" % v][0].max() > 2 and res["rows%d" % v][0].max() > 2
    for k in (65, 300):
        for name in ("component_chain%d" % k, "component_chain%d_shuffled" % k):
            comp1, grp = res[name]
            assert comp1.max() == k and set(grp.tolist()) == {-1, 0} and int((grp == 0).sum()) == 2 * k   # level 2: one chain of k components
    # the component-0 rule
    X, Y, Z, n = I["component_zero_rule"]
    comp1, grp = res["component_zero_rule"]
    keep = ci.keep_rows(X, Y, grp)
    c = comp1 == comp1[n - 1]
    assert comp1[n - 1] == 0 and int(c.sum()) == 3 and np.all(grp[c] == -1)                         # it does not merge, its genes get -1
    cross = c[X] != c[Y]
    assert int(cross.sum()) == 2 and len(set(comp1[X[cross]].tolist() + comp1[Y[cross]].tolist()) - {0}) == 2   # rows to two other components
    inner = c[X] & c[Y]
    assert int(inner.sum()) == 2 and np.all(keep[inner]) and not np.any(keep[cross])                # its inner rows are kept
    zero = (grp[X] == 0) & (grp[Y] == 0)
    assert int(zero.sum()) == 3 and not np.any(keep[zero]) and int((grp == 1).sum()) == 4            # group 0 is there and dropped
    assert keep.tolist() == [False] * 3 + [True] * 4 + [False] * 2 + [True]
    # level-2 order: group numbers against component numbers, both ways round
    for name, sign in (("level2_opposite", -1), ("level2_same", 1)):
        comp1, grp = res[name]
        assert sorted(set(grp.tolist())) == [-1, 0, 1, 2, 3]
        lowest = [int(comp1[grp == g].min()) for g in range(4)]
        assert lowest == sorted(lowest, reverse=sign < 0) and len(set(lowest)) == 4
    assert not np.array_equal(res["level2_5"][1], res["level2_6"][1])
    # self pairs
    X, Y, Z, n = I["self_pair_only_row"]
    comp1, grp = res["self_pair_only_row"]
    assert X[0] == Y[0] == 0 and int(((X == 0) | (Y == 0)).sum()) == 1 and int((comp1 == comp1[0]).sum()) == 1 and comp1[0] != 0
    X, Y, Z, n = I["self_pair_beside_heavier"]
    assert X[0] == Y[0] and Z[0] < Z[1] and X[1] == X[0]
    # weights
    X, Y, Z, n = I["repeated_pair_two_weights"]
    assert (X[0], Y[0]) == (X[2], Y[2]) and Z[0] != Z[2]
    assert np.all(I["negative_weights"][2][:-1] < 0)
    Z = I["signed_zeros"][2]
    assert int(np.signbit(Z[Z == 0]).sum()) == 2 and int((Z == 0).sum()) == 4
    Z = I["infinities"][2]
    assert int((Z == np.inf).sum()) == 2 and int((Z == -np.inf).sum()) == 4
    for name in ("family_a", "family_b"):
        X, Y, Z, n = I[name]
        assert 19000 <= n <= 21000 and 95000 <= len(X) <= 105000
        assert res[name][0].max() > 500 and np.any(res[name][1] == -1)
    assert res["family_a"][1].max() >= 1 and res["family_b"][1].max() > 100                       # bridges everywhere / few bridges


# a deviation -> an input on which it differs from group_numbers
DEVIATION_TABLE = {"min_label": "level2_same", "first_best_only": "two_best_neighbours", "signed_zero": "signed_zeros", "rank_by_component": "level2_opposite",
                   "component0_merges": "component_zero_rule", "keep_group0": "component_zero_rule"}


@pytest.mark.parametrize("deviation", ci.DEVIATIONS)
def test_every_single_deviation_is_told_apart(deviation):
    from swiftortho_amd import find_cluster as fc
    assert sorted(DEVIATION_TABLE) == sorted(ci.DEVIATIONS)
    X, Y, Z, n = ci.inputs()[DEVIATION_TABLE[deviation]]
    comp1, grp = fc.group_numbers(X, Y, Z, n)
    assert same(ci.closed_form(X, Y, Z, n), X, Y, comp1, grp)
    assert not same(ci.closed_form(X, Y, Z, n, deviation), X, Y, comp1, grp)
    differing = [k for k, v in ci.inputs().items() if len(v[0]) <= 3000 and not same(ci.closed_form(*v, deviation), v[0], v[1], *fc.group_numbers(*v))]
    assert DEVIATION_TABLE[deviation] in differing


@pytest.mark.parametrize("name,variant", cluster_cases())
def test_goldens_through_the_stage_argument(name, variant):
    """cnc() still prints the golden text -- by default, with group_numbers named, and with the restatement as the stage (three results:
    the stage's own keep flags are used)"""
    from swiftortho_amd import find_cluster as fc
    meta = json.load(open(os.path.join(GOLD, "clu_%s.json" % name)))
    a = fc.parse(["find_cluster.py", "-i", "x"] + meta["variants"][variant])
    want = open(os.path.join(GOLD, "clu_%s.%s.mcl" % (name, variant))).read()
    seen = []

    def spy(X, Y, Z, n):
        seen.append(n)
        return fc.group_numbers(X, Y, Z, n)
    for stage in (None, spy, ci.closed_form):
        groups = fc.cnc(open(os.path.join(GOLD, meta["input"])), float(a["-I"]), mcl=scipy_mcl, groups=stage)
        assert "".join("\t".join(g) + "\n" for g in groups) == want
    assert len(seen) == 1 and seen[0] > 0


def test_nan_weight_keeps_the_numpy_stage(monkeypatch):
    """device_stage=True with a NaN weight: the device stage is not called"""
    from swiftortho_amd import find_cluster as fc
    lines = ["a|1\ta|2\t1.0\n", "a|2\ta|3\tnan\n", "b|1\tb|2\t2.0\n", "b|2\tb|3\t2.0\n", "c|1\tc|2\t1.0\n"]

    def never(*a, **k):
        raise AssertionError("the device stage was called")
    monkeypatch.setattr(fc, "device_group_numbers", never)
    with np.errstate(all="ignore"):
        assert fc.cnc(lines, 1.5, mcl=scipy_mcl, device_stage=True) == fc.cnc(lines, 1.5, mcl=scipy_mcl)


def test_flag_table_and_manual_carry_the_stage_switch(capsys):
    from swiftortho_amd import find_cluster as fc
    assert fc.DEFAULTS["-G"] == "F"
    assert fc.parse(["find_cluster.py", "-i", "x", "-G", "t"])["-G"] == "t" and fc.parse(["find_cluster.py", "-i", "x", "-GT"])["-G"] == "T"
    fc.manual_print()
    assert "  -G: " in capsys.readouterr().out


REFUSALS = [("nan", lambda X, Y, Z, n: (X, Y, np.where(np.arange(len(Z)) == 1, np.nan, Z), n), "NaN"),
            ("gene_above", lambda X, Y, Z, n: (np.where(np.arange(len(X)) == 2, n, X), Y, Z, n), "outside 0 .. n_genes - 1"),
            ("gene_below", lambda X, Y, Z, n: (X, np.where(np.arange(len(X)) == 0, -1, Y), Z, n), "outside 0 .. n_genes - 1"),
            ("gene_without_row", lambda X, Y, Z, n: (X, Y, Z, n + 1), "occurs in no row"),
            ("negative_genes", lambda X, Y, Z, n: (X[:0], Y[:0], Z[:0], -1), "bad arguments")]


def refused(case):
    """(return code, message, the result structure) of a refused call on the component-0 input, through the C ABI"""
    import ctypes as C
    from swiftortho_amd import _lib
    L = _lib.load()
    name, change, message = case
    X, Y, Z, n = change(*ci.inputs()["component_zero_rule"])
    x, y, z = np.ascontiguousarray(X, dtype=np.int32), np.ascontiguousarray(Y, dtype=np.int32), np.ascontiguousarray(Z, dtype=np.float64)
    res = _lib.SoCncResult()
    res.n_genes = 77                                      # (the call clears the structure before anything else)
    rc = L.so_cnc_groups(0, int(n), len(x), x.ctypes.data, y.ctypes.data, z.ctypes.data, C.byref(res))
    return rc, L.so_cnc_last_error().decode(), res


@pytest.fixture(scope="module")
def built():
    from swiftortho_amd import build
    build.build(verbose=False)


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals_come_before_the_device(case, built):
    """what so_cnc_groups refuses it refuses on the host, before it looks for a device: non-zero, the message, no result allocated"""
    rc, msg, res = refused(case)
    assert rc != 0 and case[2] in msg, msg
    assert not res.comp1 and not res.grp and not res.keep and res.n_genes == 0 and res.n_keep == 0
    import ctypes as C
    from swiftortho_amd import _lib
    L = _lib.load()
    x = np.zeros(1, dtype=np.int32)
    z = np.zeros(1)
    assert L.so_cnc_groups(0, 1, -1, x.ctypes.data, x.ctypes.data, z.ctypes.data, C.byref(res)) != 0 and "bad arguments" in L.so_cnc_last_error().decode()
    assert L.so_cnc_groups(0, 1 << 31, 0, None, None, None, C.byref(res)) != 0 and "2^31" in L.so_cnc_last_error().decode()
    assert L.so_cnc_groups(0, 1, 1, x.ctypes.data, x.ctypes.data, z.ctypes.data, None) != 0


def test_component_stage_fails_loudly_without_a_gpu(built):
    """no CPU path: the device stage reports the missing device"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from swiftortho_amd import find_cluster as fc
    with pytest.raises(RuntimeError) as e:
        fc.device_group_numbers(*ci.inputs()["one_pair"])
    assert "HIP" in str(e.value)
