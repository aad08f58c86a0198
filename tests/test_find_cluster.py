"""MCL clustering counterpart (swiftortho_amd/find_cluster.py) against stdout of the REAL reference script
bin/find_cluster.py -a mcl captured by tools/refharness/make_cluster_goldens.py, plus hand-checkable graphs.
The Markov loop itself runs on the GPU (so_mcl): the `gpu` tests go through it (and the CLI); the CPU tests check the host
bookkeeping -- graph components, batching, matrix construction, read-out -- with the scipy ORACLE of the loop plugged in
(tests/mcl_scipy_oracle.py), which pins that oracle on the same goldens."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLD, ROOT
from mcl_scipy_oracle import scipy_mcl


def cluster_cases():
    out = []
    for f in sorted(os.listdir(GOLD)):
        if f.startswith("clu_") and f.endswith(".json"):
            for v in json.load(open(os.path.join(GOLD, f)))["variants"]:
                out.append((f[4:-5], v))
    return out


def as_sets(text):
    """scripts/mcl_cmp.py's view of a clustering: a set of gene sets"""
    return sorted(tuple(sorted(l.split("\t"))) for l in text.split("\n") if l)


def _groups(name, variant, mcl):
    from swiftortho_amd import find_cluster as fc
    meta = json.load(open(os.path.join(GOLD, "clu_%s.json" % name)))
    a = fc.parse(["find_cluster.py", "-i", "x"] + meta["variants"][variant])
    kw = {"mcl": mcl} if mcl else {}
    return fc.cnc(open(os.path.join(GOLD, meta["input"])), float(a["-I"]), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name,variant", cluster_cases())
def test_groups_match_reference_device_mcl(name, variant):
    """the product path: Markov loop on the GPU"""
    groups = _groups(name, variant, None)
    got = "".join("\t".join(g) + "\n" for g in groups)
    want = open(os.path.join(GOLD, "clu_%s.%s.mcl" % (name, variant))).read()
    assert as_sets(got) == as_sets(want)
    assert got == want


@pytest.mark.gpu
def test_device_mcl_equals_scipy_oracle_matrix():
    """so_mcl returns scipy's final matrix: same structure (storage order, stored zeros), values within one float32 ulp (the
    inflation is a correctly rounded double pow on the device, libm powf on the host)"""
    from swiftortho_amd import find_cluster as fc
    meta = json.load(open(os.path.join(GOLD, "clu_taxa4_colon.json")))
    lines = [l.split("\t", 1)[1] for l in open(os.path.join(GOLD, meta["input"])) if l.split("\t")[1] <= l.split("\t")[2]]
    names, ip, ix, dv = fc.block_matrix(lines)
    for infl in (1.5, 2.0, 4.0):
        a, b = fc.device_mcl(ip, ix, dv, infl), scipy_mcl(ip, ix, dv, infl)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.allclose(a[2], b[2], rtol=3e-7, atol=0)
        assert fc.surviving_pairs(*a) == fc.surviving_pairs(*b)


def _family_graph(seed, nfam, famsize):
    rng = np.random.default_rng(seed)
    lines = []
    for f in range(nfam):
        names = ["t%d|f%dg%d" % (k % 7, f, k) for k in range(famsize)]
        for i in range(famsize):
            for j in range(i + 1, famsize):
                if rng.random() < 0.6:
                    a, b = sorted((names[i], names[j]))
                    lines.append("%s\t%s\t%r\n" % (a, b, float(np.round(10 ** rng.uniform(-2, 2), 4))))
    for _ in range(nfam * 3):   # weak bridges
        f, g = rng.integers(0, nfam, 2)
        a, b = sorted(("t0|f%dg0" % f, "t1|f%dg1" % g))
        if a != b:
            lines.append("%s\t%s\t0.01\n" % (a, b))
    return lines + lines[:5]    # repeated pairs: the last line wins


@pytest.mark.gpu
@pytest.mark.parametrize("seed,nfam,famsize,inflation,rounds", [(1, 40, 12, 1.5, 100), (2, 6, 70, 1.5, 100), (3, 3, 150, 2.0, 100), (5, 2, 400, 1.4, 100),
                                                                (4, 25, 30, 1.5, 3), (4, 25, 30, 2.0, 3)])
def test_device_mcl_random_graphs_vs_scipy(seed, nfam, famsize, inflation, rounds):
    """random family graphs: dense families (rows of 70-400 entries: thousands of products per output row, i.e. the global-scratch
    tables of the expansion kernel, not only the LDS ones), weak links between families, duplicate lines, weights over four decades.
    Runs cut after 2-6 rounds end on a matrix full of pruned (stored) zeros, which the reference's read-out zips against: structure
    identical to scipy's (storage order, stored zeros), values within one ulp, identical read-out.
    (Runs that go 100 rounds WITHOUT converging -- inflation <= 1.05 -- are not compared: numpy's float32 power on this CPU is the
    AVX512 SVML routine, which differs from libm's powf and from the correctly rounded value in ~20 % of inputs by one ulp; a hundred
    non-contracting rounds amplify that, so the reference itself does not reproduce such a run across CPU types.  For the same reason a
    run stopped where many entries sit AT the pruning threshold -- inflation 3.0 cut after two rounds, inflation 1.5 after six -- shows a
    handful of flipped decisions against this host's numpy; such cases are not in the list.)
    The round in which the loop stops and whether it converged (so_mcl_result.rounds, .converged) are the oracle's: in these runs the
    maximum of the last check is exactly 0 and the one before it is far above atol, with numpy's power and with the exact one alike,
    so the decision does not hang on the power routine.  (Short runs are compared bit for bit in tests/test_gpu_mcl.py.)"""
    from swiftortho_amd import find_cluster as fc
    names, ip, ix, dv = fc.block_matrix(_family_graph(seed, nfam, famsize))
    got, want = {}, {}
    a, b = fc.device_mcl(ip, ix, dv, inflation, rounds=rounds, info=got), scipy_mcl(ip, ix, dv, inflation, rounds=rounds, info=want)
    assert got == {"rounds": want["rounds"], "converged": want["converged"]}
    assert (want["rounds"] < 100 and want["converged"] == 1) if rounds == 100 else (want["rounds"], want["converged"]) == (rounds, 0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.allclose(a[2], b[2], rtol=1e-6, atol=1e-12)
    assert fc.surviving_pairs(*a) == fc.surviving_pairs(*b)
    if rounds < 100:
        assert int((b[2] == 0).sum()) > 100     # the stored-zero case is really exercised


@pytest.mark.parametrize("name,variant", cluster_cases())
def test_groups_match_reference(name, variant):
    groups = _groups(name, variant, scipy_mcl)
    got = "".join("\t".join(g) + "\n" for g in groups)
    want = open(os.path.join(GOLD, "clu_%s.%s.mcl" % (name, variant))).read()
    assert as_sets(got) == as_sets(want)        # the groups as sets (what config 5 diffs)
    assert got == want                          # and the same text: group order and member order too


@pytest.mark.parametrize("name,variant", cluster_cases())
def test_groups_match_reference_native_tokeniser(name, variant, monkeypatch):
    """the same goldens with the relation file read through libsohit's tokeniser (so_tsv_*; forced: small inputs normally take the
    Python loop), and with the file handed over as bytes"""
    from swiftortho_amd import find_cluster as fc
    monkeypatch.setenv("SOHIT_TSV_MIN", "0")
    meta = json.load(open(os.path.join(GOLD, "clu_%s.json" % name)))
    data = open(os.path.join(GOLD, meta["input"]), "rb").read()
    assert fc._edge_columns_native(data) is not None
    a = fc.parse(["find_cluster.py", "-i", "x"] + meta["variants"][variant])
    want = open(os.path.join(GOLD, "clu_%s.%s.mcl" % (name, variant))).read()
    for src in (data, open(os.path.join(GOLD, meta["input"]))):
        got = "".join("\t".join(g) + "\n" for g in fc.cnc(src, float(a["-I"]), mcl=scipy_mcl))
        assert got == want


def test_columnar_cnc_equals_line_by_line_semantics(monkeypatch):
    """random family graphs with repeated pairs (same pair, different weight texts), three-column rows, x > y rows, CRLF line ends, a
    last line without newline and small batches (chk): the native tokeniser and the Python loop give the same groups"""
    from swiftortho_amd import find_cluster as fc
    lines = _family_graph(11, 30, 9)
    lines += [l.replace("\t0.01\n", "\t0.010\n") for l in lines[-8:]] + ["t3|zz\tt1|aa\t5.0\n", "t9|b\tt9|a\t1.0\n"]
    for text in ("".join("OT\t" + l for l in lines), "".join(lines), "".join("OT\t" + l for l in lines).replace("\n", "\r\n"), "".join(lines)[:-1]):
        for chk in (10 ** 7, 20):
            monkeypatch.setenv("SOHIT_TSV_NATIVE", "0")
            ref = fc.cnc(text.encode(), 1.5, chk, mcl=scipy_mcl)
            monkeypatch.setenv("SOHIT_TSV_NATIVE", "1")
            monkeypatch.setenv("SOHIT_TSV_MIN", "0")
            assert fc._edge_columns_native(text.replace("\r\n", "\n").encode() if text.endswith("\n") else (text[:-1] + "\n").encode()) is not None
            assert fc.cnc(text.encode(), 1.5, chk, mcl=scipy_mcl) == ref
            assert len(ref) >= 1


def test_hand_checkable_graphs():
    """Two cliques joined by one weak edge split at I = 2; a clique stays whole.  The reference's numbering accidents, by hand:
    best-neighbour components are numbered in popitem() order (last gene of the file first), so the LAST clique of the file is
    level-1 component 0, is never merged (`if X and Y`, 1533) and is clustered in the shared block -1; level-2 groups are
    numbered in file order, so the FIRST clique of the file is level-2 group 0 and is dropped (`if cx and cy and cx == cy`, 1584)."""
    from swiftortho_amd import find_cluster as fc

    def clique(names, w):
        return ["OT\t%s\t%s\t%s\n" % (a, b, w) for i, a in enumerate(names) for b in names[i + 1:]]

    a, b = ["a|1", "a|2", "a|3", "a|4"], ["b|1", "b|2", "b|3", "b|4"]
    lines = clique(["z|0", "z|1", "z|2"], 1.0) + clique(a, 1.0) + clique(b, 1.0) + ["OT\ta|1\tb|1\t0.05\n"] + clique(["c|1", "c|2", "c|3"], 2.0)
    groups = [sorted(g) for g in fc.cnc(lines, 2.0, mcl=scipy_mcl)]
    assert groups == [["c|1", "c|2", "c|3"], sorted(a), sorted(b)]   # block -1 first, then level-2 groups ascending; z|* dropped
    # without the bridge nothing changes; with a strong bridge and gentle inflation the two cliques stay together
    strong = clique(["z|0", "z|1"], 1.0) + clique(a, 1.0) + clique(b, 1.0) + ["OT\ta|%d\tb|%d\t1.0\n" % (i, j) for i in (1, 2, 3, 4) for j in (1, 2, 3, 4)]
    groups = [sorted(g) for g in fc.cnc(strong + clique(["c|1", "c|2"], 1.0), 1.2, mcl=scipy_mcl)]
    assert sorted(a + b) in groups


@pytest.mark.gpu
def test_find_cluster_cli(tmp_path):
    meta = json.load(open(os.path.join(GOLD, "clu_taxa4_colon.json")))
    inp = os.path.join(GOLD, meta["input"])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "find_cluster.py"), "-i", inp, "-a", "mcl", "-I", "1.5"], capture_output=True,
                       text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == open(os.path.join(GOLD, "clu_taxa4_colon.I1.5.mcl")).read()
    assert os.listdir(str(tmp_path)) == []
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "find_cluster.py"), "-i", inp], capture_output=True, text=True)
    assert r.returncode == 2 and "mcl" in r.stderr      # default -a apc: not provided


def _zero_column_cases():
    """CSR blocks whose column 0 sums to zero in some round of the loop: (a) gene 0 has only zero-weight edges from the start;
    (b) gene 0's column holds forty equal entries, which inflation 4 pushes below the pruning threshold after the first expansion:
    the column holds stored zeros only from round 2 on, while the other columns keep their heavy diagonals."""
    from scipy import sparse
    rng = np.random.default_rng(7)
    n = 12
    a = np.zeros((n, n), dtype=np.float32)
    for i in range(1, n):
        for j in range(i, n):
            if i == j or rng.random() < 0.5:
                a[i, j] = a[j, i] = np.float32(rng.uniform(0.5, 3.0))
    m = sparse.lil_matrix(a)
    ma = sparse.csr_matrix(m)
    # explicit zeros in row / column 0
    ip, ix, dv = ma.indptr.astype(np.int64), ma.indices.astype(np.int32), ma.data.astype(np.float32)
    rows = [list(zip(ix[ip[i]:ip[i + 1]], dv[ip[i]:ip[i + 1]])) for i in range(n)]
    rows[0] = [(0, np.float32(0)), (1, np.float32(0))]
    rows[1] = [(0, np.float32(0))] + rows[1]
    ipa = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    ixa = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    dva = np.array([v for r in rows for _, v in r], dtype=np.float32)
    # (b): genes 1..40 on a ring with heavy self loops (their columns keep entries above the threshold), gene 0 tied to all of them:
    # column 0 = forty equal entries, row 0 = forty weak ones, no self loop
    n2 = 41
    b = np.zeros((n2, n2), dtype=np.float32)
    for i in range(1, n2):
        b[i, i] = 10.0
        j = 1 + (i % 40)
        b[i, j] = b[j, i] = 1.0
        b[i, 0] = 1.0
        b[0, i] = 0.01
    mb = sparse.csr_matrix(b)
    return [("zero_weight_gene", ipa, ixa, dva, 1.5), ("pruned_column", mb.indptr.astype(np.int64), mb.indices.astype(np.int32), mb.data.astype(np.float32), 4.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", [0, 1])
def test_device_mcl_zero_sum_first_column(case, monkeypatch):
    """normalize() adds (index of the first column with a non-zero sum) / 1000 when some column sums to zero (find_cluster.py:636-646):
    0.0 only while column 0 itself has a sum.  Both cases make column 0 sum to zero; the scipy oracle and the device loop must agree
    (no NaN from 0 / 0, same convergence decision)."""
    import mcl_scipy_oracle as mo
    from swiftortho_amd import find_cluster as fc
    name, ip, ix, dv, infl = _zero_column_cases()[case]
    seen = []
    real = mo._normalize

    def spy(x):
        y = np.asarray(x.sum(0))[0]
        seen.append(bool(y.min() == 0 and y.max() > 0 and y[0] == 0))
        real(x)
    monkeypatch.setattr(mo, "_normalize", spy)
    for rounds in (1, 2, 4, 100):
        seen.clear()
        ginfo, winfo = {}, {}
        got = fc.device_mcl(ip, ix, dv.copy(), infl, rounds=rounds, info=ginfo)
        want = mo.scipy_mcl(ip.copy(), ix.copy(), dv.copy(), infl, rounds=rounds, info=winfo)   # (scipy normalises the data array it is handed in place)
        assert ginfo == {"rounds": winfo["rounds"], "converged": winfo["converged"]} == {"rounds": rounds, "converged": 0}, (name, rounds)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, rounds)
        assert np.allclose(got[2], want[2], rtol=1e-6, atol=1e-12, equal_nan=True), (name, rounds)
        assert np.isnan(got[2]).sum() == np.isnan(want[2]).sum()
        if rounds >= 2:
            assert any(seen), "%s: column 0 never summed to zero -- the case does not test what it says" % name
