"""Reciprocal best hits and the core-gene table (swiftortho_amd/rbh.py; scripts/get_rbh.py, scripts/rbh2phy.py) against what the REAL
reference scripts gave (tests/golden/rbh_*.json, tools/refharness/make_rbh_goldens.py): the pairs byte for byte, the groups list for
list.  CPU only: the numpy definitions the kernels of csrc/rbh.hip are held to (tests/test_gpu_rbh.py), and both scripts with -G F."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rbh_inputs as ri
from conftest import ROOT


@pytest.fixture(scope="module")
def rbh():
    from swiftortho_amd import rbh
    return rbh


def _cols(name):
    from swiftortho_amd import find_orth
    return find_orth.columns_from_text(ri.golden(name)[0])


def _groups(rbh, cols, table):
    return [[i.decode() for i in g] for g in rbh.core_groups(cols.names, table)]


def test_goldens_cover_the_designed_inputs():
    names = ri.golden_names()
    assert set(ri.BUILDERS) <= set(names) and {"taxa5", "taxa3_dense", "taxa4_colon", "taxa12"} <= set(names)
    # the counts measured with the real scripts when the stage was specified
    assert [ri.golden(n)[2]["pairs"].count("\n") for n in ("taxa5", "taxa3_dense", "taxa4_colon")] == [360, 89, 246]
    assert [len(g) for g in ri.golden("taxa5")[2]["groups"][""]] == [5] * 17
    assert [len(g) for g in ri.golden("taxa3_dense")[2]["groups"][""]] == [3] * 20 and ri.golden("taxa3_dense")[2]["groups"]["tx02"] == []
    # -r with a taxon other than the largest: the gene is missing from its own group, which still reaches 11 / 12
    other = [r for r in ri.golden("taxa12")[2]["groups"] if r]
    assert other and all(ri.golden("taxa12")[2]["groups"][r] and all(len(g) == 11 for g in ri.golden("taxa12")[2]["groups"][r]) for r in other)
    assert ri.golden("edge_absent_taxon")[2]["raises"] == [""]
    assert ri.golden("edge_pairs")[2]["pairs"] == "a|m1\tb|m1\na|m2\tb|m2\na|m2\tb|m2\na|m8\tb|m8\n"


def test_designed_inputs_hold_what_they_promise(rbh):
    cols = _cols("edge_runs")
    q = np.asarray(cols.q)
    b = np.flatnonzero(np.concatenate([[True], q[1:] != q[:-1], [True]]))
    lens = np.diff(b).tolist()
    assert lens[:10] == [1, 2, 63, 128, 30, 64, 65, 129, 256, 257] and b[5] == 224 and b[6] == 288 and lens[-1] == 1
    assert ri.golden("edge_runs")[2]["pairs"].count("\n") >= 5
    cols = _cols("edge_taxa")
    tax, taxa = rbh.name_taxa(cols.names)
    run = np.cumsum(np.concatenate([[0], np.asarray(cols.q)[1:] != np.asarray(cols.q)[:-1]]))
    per_run = [len(set(tax[np.asarray(cols.s)[run == r]].tolist())) for r in range(int(run[-1]) + 1)]
    assert {1, 2, 63, 64, 65, 300} <= set(per_run) and len(taxa) == 301


@pytest.mark.parametrize("shape", ri.RUN_SHAPES)
@pytest.mark.parametrize("n", ri.RUN_SIZES)
def test_run_shapes_hold_what_they_promise(n, shape):
    """the heads stand on the rows the shape names, and the numpy answer is not trivially empty: a core gene for every shape above one
    row, and a pair wherever the table has two runs -- "one" has none by definition: a single run proposes every pair key once, and a
    pair is a key proposed twice (asserted as such)"""
    cols, fasta, starts, pairs, tables = ri.run_shape_case(n, shape)
    q = np.asarray(cols.q)
    heads = np.flatnonzero(np.concatenate([[True], q[1:] != q[:-1]]))
    assert len(q) == n and heads.tolist() == starts.tolist()
    want = {"each": list(range(n)), "one": [0], "cut": [0] + [c for c in ri.RUN_CUTS if c < n]}[shape]
    assert heads.tolist() == want
    if shape == "cut":
        assert set(heads.tolist()) >= {c for c in (255, 256, 257, 8191, 8192, 8193, 32767, 32768) if c < n}
    if n > 1:
        assert len(tables["ta"].genes) >= 1 and bool((tables["ta"].fwd >= 0).any())
        assert (len(heads) == 1) == (shape == "one")
        assert len(pairs[0]) == (0 if shape == "one" else len(heads) // 2) and (shape == "one" or len(pairs[0]) >= 1)


@pytest.mark.parametrize("name", ri.golden_names())
def test_pairs_numpy(rbh, name):
    cols = _cols(name)
    a, b = rbh.reciprocal_best_hits(cols)
    assert rbh.rbh_lines(cols.names, a, b) == ri.golden(name)[2]["pairs"].encode()


@pytest.mark.parametrize("name,ref", ri.golden_ref_cases())
def test_groups_numpy(rbh, name, ref):
    sc, fasta, meta = ri.golden(name)
    cols = _cols(name)
    if ref in meta["raises"]:
        with pytest.raises(ValueError) as e:
            rbh.core_table(cols, fasta, ref)
        assert "not among the taxa of the FASTA" in str(e.value)
        return
    table = rbh.core_table(cols, fasta, ref)
    assert _groups(rbh, cols, table) == meta["groups"][ref]


@pytest.mark.parametrize("name", ri.golden_names())
def test_script_get_rbh(tmp_path, name):
    sc, _, meta = ri.golden(name)
    p = str(tmp_path / "in.sc")
    open(p, "wb").write(sc)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "get_rbh.py"), p], capture_output=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == meta["pairs"].encode()


def run_rbh2phy(tmp_path, name, ref, extra=()):
    """scripts/rbh2phy.py on a golden -> (completed process, groups of -o, groups read back from the .fsa files)"""
    sc, fasta, meta = ri.golden(name)
    p, f, o = str(tmp_path / "in.sc"), str(tmp_path / "in.fsa"), str(tmp_path / "groups.tsv")
    open(p, "wb").write(sc)
    open(f, "wb").write(fasta)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "rbh2phy.py"), "-i", p, "-f", f, "-o", o] + (["-r", ref] if ref else []) + list(extra),
                       capture_output=True)
    if r.returncode != 0:
        return r, None, None
    groups = [l.split("\t") for l in open(o).read().split("\n") if l]
    files = []
    for k in range(len(groups)):
        recs = open(p + "_alns_tmp/%d.fsa" % k).read().split("\n")
        assert recs[-1] == "" and len(recs) == 2 * len(groups[k]) + 1 and all(s and not s.startswith(">") for s in recs[1:-1:2])
        files.append([h[1:].split()[0] for h in recs[0:-1:2]])
    assert not os.path.exists(p + "_alns_tmp/%d.fsa" % len(groups))
    return r, groups, files


@pytest.mark.parametrize("name,ref", ri.golden_ref_cases())
def test_script_rbh2phy(tmp_path, name, ref):
    meta = ri.golden(name)[2]
    r, groups, files = run_rbh2phy(tmp_path, name, ref)
    if ref in meta["raises"]:
        assert r.returncode != 0 and b"not among the taxa of the FASTA" in r.stderr
        return
    assert r.returncode == 0, r.stderr[-2000:]
    assert groups == files == meta["groups"][ref]
    assert b"not part of this port" in r.stderr and r.stdout == b""


def test_fsa_files_carry_header_and_sequence(tmp_path):
    r, groups, _ = run_rbh2phy(tmp_path, "edge_core", "")
    assert r.returncode == 0 and groups == [["A|1", "B|2", "C|1"], ["A|2", "B|3", "C|2"]]
    assert open(str(tmp_path / "in.sc") + "_alns_tmp/0.fsa").read() == "".join(">%s some description\nACDEFGHIKLMNPQRSTVWY\n" % i for i in groups[0])


def test_fasta_taxa_order(rbh):
    fa = b">b|1 x\nAC\n>c|1\nAC\n>c|2\nAC\n>a|1\nAC\n>b|2\nAC\n>d|9\nAC\n>a|2\r\nAC\r\n>solo\nAC\n>a|3"
    assert rbh.fasta_taxa(fa) == [b"a", b"b", b"c", b"d", b"solo"]      # a: 3 genes; b before c (first appearance); then the singles
    assert rbh.fasta_taxa(b">x|1\nA\n>y|1") == [b"x", b"y"] and rbh.fasta_taxa(b"") == []
    assert rbh.fasta_taxa(b">x:1\n>x:2\n>y:1\n", sep=":") == [b"x", b"y"]


def test_nan_takes_the_literal_loop(rbh, monkeypatch):
    calls = []
    literal = rbh._literal_winners
    monkeypatch.setattr(rbh, "_literal_winners", lambda *a: calls.append(a[2]) or literal(*a))
    sc, fasta, meta = ri.golden("edge_nan")
    cols = _cols("edge_nan")
    assert np.isnan(cols.score).sum() == 5
    a, b = rbh.reciprocal_best_hits(cols)
    assert rbh.rbh_lines(cols.names, a, b) == meta["pairs"].encode() and calls == [False]
    assert _groups(rbh, cols, rbh.core_table(cols, fasta, "b")) == meta["groups"]["b"] and calls == [False, True]
    cols = _cols("edge_ties")
    rbh.reciprocal_best_hits(cols)
    assert calls == [False, True]                                       # numbers never go there


def test_literal_loops_agree_with_numpy_on_numbers(rbh):
    for name in ("edge_runs", "edge_ties", "edge_pairs", "taxa3_dense"):
        cols = _cols(name)
        tax, taxa = rbh.name_taxa(cols.names)
        wq, ws, nrun = rbh.winners(cols, tax, len(taxa))
        lq, ls, lrun = rbh._literal_winners(cols, tax, False)
        assert nrun == lrun and wq.tolist() == lq.tolist() and ws.tolist() == ls.tolist()
        sq, ss, _ = rbh._literal_winners(cols, tax, True)               # (the sorted walk lists a run's winners in another order)
        assert sorted(zip(sq.tolist(), ss.tolist())) == sorted(zip(wq.tolist(), ws.tolist()))


def test_score_spellings_are_one_number():
    cols = _cols("edge_ties")
    nm = cols.names.tolist()
    rows = [k for k in range(len(cols.q)) if nm[cols.q[k]] == b"a|seven" and nm[cols.s[k]] in (b"b|seven_002", b"b|seven_003", b"b|seven_004")]
    assert len(rows) == 3 and cols.score[rows].tolist() == [7., 7., 7.]


def _call(L, lib, n=1, n_names=2, tax=(0, 1), n_taxa=2, ref=-1, flags=0, q=(0,), s=(1,)):
    q, s = np.asarray(q, dtype=np.int32), np.asarray(s, dtype=np.int32)
    sco, tax = np.ones(len(q)), np.asarray(tax, dtype=np.int32)
    out = lib.SoRbhResult()
    rc = L.so_rbh_cols(0, n, q.ctypes.data, s.ctypes.data, sco.ctypes.data, n_names, tax.ctypes.data, n_taxa, ref, flags, C.byref(out))
    msg = L.so_rbh_last_error().decode()
    if rc == 0:
        L.so_rbh_free(C.byref(out))
    else:
        assert not any((out.rbh_a, out.rbh_b, out.core_gene, out.core_fwd, out.core_rec))   # nothing left allocated
    return rc, msg


def test_refusals_before_the_device():
    """what so_rbh_cols refuses before it looks for a device; without one, everything else is refused too (no CPU fallback)"""
    from swiftortho_amd import build
    build.build(verbose=False)
    from swiftortho_amd import _lib
    L = _lib.load()
    for kw, word in ((dict(n=1 << 31), "2^31 rows"), (dict(tax=(0, 2)), "taxon"), (dict(ref=2), "ref_taxon"), (dict(ref=-2), "ref_taxon"), (dict(flags=1), "flags"),
                     (dict(n=-1), "bad arguments"), (dict(n_names=1 << 31), "2^31 names")):
        rc, msg = _call(L, _lib, **kw)
        assert rc != 0 and word in msg, (kw, msg)
    assert L.so_rbh_cols(0, 0, None, None, None, 0, None, 0, -1, 0, None) != 0 and "NULL" in L.so_rbh_last_error().decode()
    import torch
    if not torch.cuda.is_available():
        from swiftortho_amd import rbh
        rc, msg = _call(L, _lib)
        assert rc != 0 and "no HIP device" in msg
        with pytest.raises(RuntimeError) as e:
            rbh.device_reciprocal_best_hits(_cols("edge_one"))
        assert "HIP" in str(e.value)
        with pytest.raises(RuntimeError):
            rbh.device_core_table(_cols("edge_core"), ri.golden("edge_core")[1])
