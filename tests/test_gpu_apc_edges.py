"""so_apc (swiftortho_amd/csrc/apc.hip) on the inputs of tests/apc_edge_inputs.py -- every lane / wave / chunk length, named ties,
directed lists, two diagonal entries, an order-revealing column, non-finite, denormal and signed-zero scores -- against the literal
oracle (tests/apc_numpy_oracle.py): labels equal, R and A equal BIT FOR BIT (same_bits: the sign of a zero counts, a NaN equals a NaN).
tests/test_apc_edges.py shows without a GPU that these inputs hold what they promise and tell each single deviation of the kernels from
the oracle."""
import numpy as np
import pytest

import apc_edge_inputs as X
from apc_edge_inputs import same_bits

pytestmark = pytest.mark.gpu


def device(entries, damp, rounds):
    from swiftortho_amd import find_cluster as fc
    row, col, score, n = entries
    lab, r, a = fc.device_apc(row, col, score, n, damp, rounds=rounds)
    assert lab.dtype == np.int64 and r.dtype == np.float32 and a.dtype == np.float32
    return lab, r, a


def differing(got, want):
    x, y = got.view(np.uint32), want.view(np.uint32)
    return int(((x != y) & ~(np.isnan(got) & np.isnan(want))).sum())


def check(what, got, want):
    print(what, "labels differing", int((got[0] != want[0]).sum()), "R differing", differing(got[1], want[1]), "A differing", differing(got[2], want[2]),
          "of", len(want[1]), "NaN", int(np.isnan(want[1]).sum() + np.isnan(want[2]).sum()))
    assert np.array_equal(got[0], want[0]), what
    assert same_bits(got[1], want[1]), what
    assert same_bits(got[2], want[2]), what


@pytest.mark.parametrize("name,damp", X.RUNS, ids=["%s-d%s" % r for r in X.RUNS])
def test_device_equals_oracle(name, damp):
    """rounds 1, 2, 3 and 10 (the carried maxima and the ties show from round 2 on), 100 for the hub at W + 1 and the two-hub graphs"""
    want = X.snapshots(name, damp)
    for t in X.rounds_of(name):
        check("%s damp %s rounds %d" % (name, damp, t), device(X.entries(name), damp, t), want[t])


@pytest.mark.parametrize("name", sorted(X.e_cases()))
def test_ordered_column_bits(name):
    """the diagonal's A after one round holds the float32 of the column's float64 sum IN ENTRY ORDER: the literal bit patterns"""
    row, col, _, _ = X.entries(name)
    diag = int(np.flatnonzero((row == 0) & (col == 0))[0])
    for damp, bits in zip((0.0, 0.5), X.e_cases()[name][1]):
        got = device(X.entries(name), damp, 1)
        print(name, damp, "A of the diagonal %#x, expected %#x" % (int(got[2].view(np.uint32)[diag]), bits))
        assert int(got[2].view(np.uint32)[diag]) == bits
        check("%s damp %s" % (name, damp), got, X.snapshots(name, damp)[1])


def _one_damp(name):
    damps = X.REGISTRY[name][2]
    return 0.5 if 0.5 in damps else damps[0]


@pytest.mark.parametrize("name", X.NAMES)
def test_permuted_entry_order(name):
    """the same entries in a second, seeded order against the oracle OF THAT ORDER: the grouping by row and column keeps whatever order
    it is given, and the result goes back to it"""
    damp = _one_damp(name)
    want = X.snapshots(name, damp, True)
    for t in (1, 3):
        check("%s permuted, damp %s rounds %d" % (name, damp, t), device(X.permuted(name), damp, t), want[t])


STALE = ("A_L%d_hub5_heavy" % (X.W + 1), "C3_odd_genes", "F%d_nan_lane0_each_chunk" % (X.W + 6))


@pytest.mark.parametrize("poison", ["0xFF", "0x5A"])
@pytest.mark.parametrize("name", STALE)
def test_stale_device_memory(name, poison, monkeypatch):
    """every fresh device allocation pre-filled (so_apc reads SOHIT_POISON per call): nothing rests on what an allocation held"""
    assert name in X.REGISTRY
    monkeypatch.setenv("SOHIT_POISON", poison)
    damp = _one_damp(name)
    for t in (1, 3, 10):
        check("%s poison %s rounds %d" % (name, poison, t), device(X.entries(name), damp, t), X.snapshots(name, damp)[t])


def test_calls_do_not_depend_on_the_call_before():
    """a long-row input, then a short one, then back, in one process: each result equals the oracle's, whatever ran before"""
    long_, short = "A_L%d_hub0_heavy" % (3 * X.W + 1), "A_L%d_hub0_heavy" % X.LM
    assert X.plan(*[X.entries(long_)[j] for j in (0, 1, 3)])[1] and not X.plan(*[X.entries(short)[j] for j in (0, 1, 3)])[1]
    for name in (long_, short, long_, short, short, "C5_full", short, long_):
        check(name + " in sequence", device(X.entries(name), 0.5, 3), X.snapshots(name, 0.5)[3])
