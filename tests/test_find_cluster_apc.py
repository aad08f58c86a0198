"""`find_cluster -a apc` (swiftortho_amd/find_cluster.py: apc_entries, device_apc, apc; libsohit so_apc, csrc/apc.hip) against stdout of
the REAL reference script bin/find_cluster.py -a apc captured by tools/refharness/make_apc_goldens.py, and against the literal
restatement of its loop (tests/apc_numpy_oracle.py).  The loop itself runs on the GPU: the `gpu` tests go through it (and the CLI) and
demand the oracle's labels and float32 stores VALUE FOR VALUE -- every operation is an IEEE add, multiply or compare in a fixed order;
the CPU tests check the host bookkeeping -- parsing, numbering, preference entries, read-out -- with the oracle plugged in, which pins
that oracle on the same goldens."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from apc_graphs import GRAPHS, _apc_graph, _entries
from apc_numpy_oracle import apc_rounds, numpy_apc
from conftest import GOLD, ROOT

CLI = os.path.join(ROOT, "bin", "find_cluster.py")


def apc_cases():
    out = []
    for f in sorted(os.listdir(GOLD)):
        if f.startswith("apc_") and f.endswith(".json"):
            for v in json.load(open(os.path.join(GOLD, f)))["variants"]:
                out.append((f[4:-5], v))
    return out


CASES = apc_cases()


def test_the_goldens_are_all_there():
    names = {n for n, _ in CASES}
    assert names == {"hub_edges", "odd_rows", "taxa3_dense", "taxa4_colon", "taxa5", "taxa8_big", "toy_default"}
    assert {v for n, v in CASES if n == "taxa8_big"} == {"default", "d0.95", "b1000"}
    big = lambda v: open(os.path.join(GOLD, "apc_taxa8_big.%s.apc" % v)).read()
    assert big("b1000") == big("default")            # the batch size cannot change a result
    assert big("d0.95") != big("default")            # the damping factor can
    assert {v for n, v in CASES if n == "hub_edges"} == {"default", "d0.9"}
    hub = lambda v: open(os.path.join(GOLD, "apc_hub_edges.%s.apc" % v)).read()
    assert hub("d0.9") != hub("default") and hub("d0.9").count("\n") >= 3 and hub("default").count("\n") >= 3


def as_sets(text):
    return sorted(tuple(sorted(l.split("\t"))) for l in text.split("\n") if l)


def _case(name, variant):
    from swiftortho_amd import find_cluster as fc
    meta = json.load(open(os.path.join(GOLD, "apc_%s.json" % name)))
    flags = meta["variants"][variant]
    a = fc.parse(["find_cluster.py", "-i", "x"] + flags)
    want = open(os.path.join(GOLD, "apc_%s.%s.apc" % (name, variant))).read()
    return os.path.join(GOLD, meta["input"]), flags, float(a["-d"]), want


def _text(groups):
    return "".join("\t".join(g) + "\n" for g in groups)


@pytest.mark.parametrize("name,variant", CASES)
def test_groups_match_reference(name, variant):
    """host bookkeeping + the literal oracle of the loop reproduce the reference's stdout"""
    from swiftortho_amd import find_cluster as fc
    inp, _, damp, want = _case(name, variant)
    got = _text(fc.apc(open(inp), damp, loop=numpy_apc))
    assert as_sets(got) == as_sets(want)
    assert got == want


@pytest.mark.parametrize("name", ["taxa8_big", "taxa4_colon"])
def test_entries_native_tokeniser_equals_python_loop(name, monkeypatch):
    """the entry list read through libsohit's tokeniser (forced: small inputs normally take the Python loop), from bytes and from an open
    file, equals the literal loop's"""
    from swiftortho_amd import find_cluster as fc
    inp = _case(name, "default")[0]
    data = open(inp, "rb").read()
    monkeypatch.setenv("SOHIT_TSV_NATIVE", "0")
    ref = fc.apc_entries(data)
    monkeypatch.setenv("SOHIT_TSV_NATIVE", "1")
    monkeypatch.setenv("SOHIT_TSV_MIN", "0")
    assert fc._edge_columns_native(data) is not None
    for src in (data, open(inp), open(inp).readlines()):
        got = fc.apc_entries(src)
        assert got[0] == ref[0] and got[4] == ref[4]
        for a, b in zip(got[1:4], ref[1:4]):
            assert a.dtype == b.dtype and np.array_equal(a, b)


def test_apc_entries_odd_rows(monkeypatch):
    """fc2mat's parsing on the odd-rows fixture, by hand: the x > y row is skipped before numbering (t2|z never gets a number); genes
    are numbered by first appearance, x before y, also on the row whose weight is unparsable; '1.5rm3' counts as 1.5; the repeated
    pair and the self pair give entries of their own; the preference is -20 x the number of distinct prefixes before '|'"""
    from swiftortho_amd import find_cluster as fc
    inp = os.path.join(GOLD, "apc_odd_rows.orth")
    for force_native in (False, True):
        if force_native:
            monkeypatch.setenv("SOHIT_TSV_MIN", "0")
        names, row, col, score, n = fc.apc_entries(open(inp))
        assert names == ["t1|a", "t1|b", "t1|c", "t2|d", "nopipe", "u1|lost", "u2|lost", "t3|e", "t3|f", "t2|g"]
        assert n == 10
        kept = [(0, 1, 3.5), (0, 1, 1.25), (2, 2, 2.0), (1, 3, 4.0), (4, 3, 1.0), (2, 3, 1.5), (0, 3, 6.0), (7, 8, 7.5), (1, 7, 0.5), (9, 8, 7.5), (9, 7, 7.5),
                (2, 9, 0.25)]
        assert len(row) == len(col) == len(score) == 2 * len(kept) + n == 34
        assert row.dtype == np.int32 and col.dtype == np.int32 and score.dtype == np.float32
        for e, (x, y, w) in enumerate(kept):
            assert (row[2 * e], col[2 * e], score[2 * e]) == (x, y, np.float32(w))
            assert (row[2 * e + 1], col[2 * e + 1], score[2 * e + 1]) == (y, x, np.float32(w))
        assert row[24:].tolist() == col[24:].tolist() == list(range(10))
        assert score[24:].tolist() == [-20.0 * 6] * 10            # prefixes t1, t2, nopipe, u1, u2, t3
    with pytest.raises(ValueError):
        fc.apc_entries(["a\tb\n"])                                 # neither three nor four fields: raises, as the reference does
    with pytest.raises(ValueError):
        fc.apc_entries(b"OT\ta\tb\t1.0\textra\n" * 3)
    assert fc.apc([]) == [] and fc.apc(b"") == []


def test_apc_read_out_is_pluggable_and_ordered():
    """groups = components of the gene -> exemplar graph, genes in number order, members in the reference's set order"""
    from swiftortho_amd import find_cluster as fc
    lines = ["OT\tg|%d\tg|%d\t1.0\n" % (i, i + 1) for i in range(5)]
    seen = {}

    def loop(row, col, score, n, damp):
        seen.update(n=n, damp=damp, entries=len(row))
        return np.array([1, 1, 3, 3, 4, 4]), None, None
    assert fc.apc(lines, 0.75, loop=loop) == [["g|0", "g|1"], ["g|2", "g|3"], ["g|4", "g|5"]]
    assert seen == {"n": 6, "damp": 0.75, "entries": 16}


def test_apc_fails_loudly_without_a_gpu():
    """the loop has no CPU path: so_apc reports the missing device, and so does the command"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from swiftortho_amd import build, find_cluster as fc
    build.build(verbose=False)
    with pytest.raises(RuntimeError) as e:
        fc.device_apc([0, 1, 0, 1], [1, 0, 0, 1], [1., 1., -40., -40.], 2, 0.5)
    assert "HIP" in str(e.value)
    r = subprocess.run([sys.executable, CLI, "-i", os.path.join(GOLD, "apc_odd_rows.orth"), "-a", "apc"], capture_output=True, text=True)
    assert r.returncode != 0 and "HIP" in r.stderr and r.stdout == ""


@pytest.mark.parametrize("flags,word", [(["-a", "sap"], "pysapc"), (["-a", "apc", "-b", "0"], "-b"), (["-a", "apc", "-b", "-5"], "-b"), (["-a", "apcx"], "preference"),
                                        (["-a", "AP"], "preference"), (["-a", "foo"], "unknown"), ([], "apc")])
def test_refused_modes_exit_2(flags, word, tmp_path):
    r = subprocess.run([sys.executable, CLI, "-i", os.path.join(GOLD, "apc_odd_rows.orth")] + flags, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 2 and r.stdout == ""
    assert word in r.stderr and "mcl" in r.stderr and "apc" in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_so_apc_refuses_bad_input():
    """argument checks come before the device is touched: gene numbers out of range and more than 2^24 genes are reported, not run"""
    from swiftortho_amd import build, find_cluster as fc
    build.build(verbose=False)
    with pytest.raises(RuntimeError) as e:
        fc.device_apc([0, 2], [1, 0], [1., 1.], 2, 0.5)
    assert "outside" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        fc.device_apc([0], [0], [1.], 2 ** 24 + 1, 0.5)
    assert "2^24" in str(e.value)


# ---- random graphs --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_snapshots(graph, damp):
    """the oracle's state after rounds 1, 2, 3, 10 and 100 of ONE run (a run of t rounds is the first t rounds of a longer one)"""
    _, row, col, score, n = _entries(graph)
    return {t + 1: snap for t, snap in enumerate(apc_rounds(row, col, score, n, damp, 100)) if t + 1 in (1, 2, 3, 10, 100)}


def test_graphs_hold_what_they_promise():
    names, row, col, score, n = _entries("hubs")
    deg = np.bincount(row, minlength=n)
    assert deg[names.index("t4|HUB")] >= 1101 and deg[names.index("t3|hub")] >= 71
    assert deg[names.index("t5|alone")] == 1 and deg[names.index("t6|alone")] == 1        # the preference entry only
    for g in GRAPHS:
        names, row, col, score, n = _entries(g)
        assert len(row) < 15000
        deg = np.bincount(row, minlength=n)
        assert deg.max() >= 71 and deg[names.index("t5|alone")] == 1
        pairs = row.astype(np.int64) * n + col
        assert len(np.unique(pairs)) < len(pairs)                                          # repeated pairs
        off = row != col
        assert len(np.unique(score[off])) < 0.7 * off.sum() / 2                            # many equal weights
        assert np.any((row == col)[:len(row) - n])                                         # a self pair among the rows
    assert np.bincount(_entries("dense")[1]).min() == 1 and np.median(np.bincount(_entries("dense")[1])) > 64


def test_oracle_wrapper_equals_its_generator():
    _, row, col, score, n = _entries("families")
    snaps = _oracle_snapshots("families", 0.5)
    for t in (0, 2):
        lab, r, a = numpy_apc(row, col, score, n, 0.5, rounds=t)
        if t == 0:
            assert np.array_equal(lab, np.arange(n)) and not r.any() and not a.any()
        else:
            assert np.array_equal(lab, snaps[t][0]) and np.array_equal(r, snaps[t][1]) and np.array_equal(a, snaps[t][2])


@pytest.mark.gpu
@pytest.mark.parametrize("damp", [0.5, 0.9])
@pytest.mark.parametrize("rounds", [1, 2, 3, 10, 100])
@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_device_apc_equals_oracle(graph, rounds, damp):
    """labels equal, R and A equal value for value (float32): full equality, not a tolerance.  Rounds 2 and 3: the never-reset row
    maxima only show from the second round on."""
    from swiftortho_amd import find_cluster as fc
    _, row, col, score, n = _entries(graph)
    want = _oracle_snapshots(graph, damp)[rounds]
    lab, r, a = fc.device_apc(row, col, score, n, damp, rounds=rounds)
    assert lab.dtype == np.int64 and r.dtype == np.float32 and a.dtype == np.float32
    print(graph, rounds, damp, "labels differing", int((lab != want[0]).sum()), "R differing", int((r != want[1]).sum()), "A differing", int((a != want[2]).sum()),
          "of", len(r))
    assert np.array_equal(lab, want[0])
    assert np.array_equal(r, want[1])
    assert np.array_equal(a, want[2])


@pytest.mark.gpu
def test_device_apc_zero_rounds_and_empty():
    from swiftortho_amd import find_cluster as fc
    lab, r, a = fc.device_apc([0, 1, 0, 1, 2], [1, 0, 0, 1, 2], [1., 1., -40., -40., -40.], 4, 0.5, rounds=0)
    assert lab.tolist() == [0, 1, 2, 3] and not r.any() and not a.any()
    lab, r, a = fc.device_apc([0, 1, 0, 1, 2], [1, 0, 0, 1, 2], [1., 1., -40., -40., -40.], 4, 0.5, rounds=5)
    want = numpy_apc([0, 1, 0, 1, 2], [1, 0, 0, 1, 2], [1., 1., -40., -40., -40.], 4, 0.5, rounds=5)
    assert np.array_equal(lab, want[0]) and np.array_equal(r, want[1]) and np.array_equal(a, want[2])
    assert lab[3] == 3                                   # a gene without any entry keeps its own number
    lab, r, a = fc.device_apc([], [], [], 0, 0.5)
    assert len(lab) == len(r) == len(a) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,variant", CASES)
def test_groups_match_reference_device_apc(name, variant):
    """the product path: the loop on the GPU"""
    from swiftortho_amd import find_cluster as fc
    inp, _, damp, want = _case(name, variant)
    got = _text(fc.apc(open(inp), damp))
    assert as_sets(got) == as_sets(want)
    assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize("name,variant", CASES)
def test_find_cluster_cli_apc(name, variant, tmp_path):
    inp, flags, _, want = _case(name, variant)
    r = subprocess.run([sys.executable, CLI, "-i", inp] + flags, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == want
    assert os.listdir(str(tmp_path)) == []
    assert not os.path.exists(inp + ".npy")


@pytest.mark.gpu
def test_find_cluster_cli_apc_is_case_insensitive(tmp_path):
    inp, _, _, want = _case("odd_rows", "default")
    r = subprocess.run([sys.executable, CLI, "-i", inp, "-aAPC"], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0 and r.stdout == want
