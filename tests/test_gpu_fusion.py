"""Gene-fusion links on the GPU (csrc/fusion.hip, include/sohit.h so_fusion_cols / so_fusion_records) against the numpy definition
(swiftortho_amd/fusion.py fusion_links) -- arrays and all counters, integer for integer -- on the designed tables of
tests/fusion_inputs.py (whose promises tests/test_fusion.py asserts): every interval, coverage, representative, homology and taxon rule
alone; runs of 0 .. 257 representatives, one run of 3000 (4.5 M pairs: several strides of the fixed grid, the decode in single and in
double precision), 20 000 short runs (the scans and the run search across block edges), a run in which every pair is a link, tables
without a row, an eligible row or a link; device memory poisoned; the records call on the same rows; every refusal; two calls with the
same arrays; scripts/fusion_links.py, scripts/run_all_fast.py -F T and pipeline.fusion_links_from_search with and without the device,
byte for byte; a hand-built proteome with one fusion, end to end.

Run on the GPU box:  python -m pytest tests/test_gpu_fusion.py -m gpu -q
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fusion_inputs as fi
from conftest import ROOT

pytestmark = pytest.mark.gpu

SCRIPT = os.path.join(ROOT, "scripts", "fusion_links.py")
SEARCH_KW = dict(ssd="111111", nr="AST,CFILMVY,DN,EQ,G,H,KR,P,W", ht=12000017, chk=50000, step=1, v=500, expect=1e-5, flt="T")


@pytest.fixture(scope="module")
def fu():
    from swiftortho_amd import fusion
    return fusion


@pytest.fixture(autouse=True)
def poisoned(monkeypatch):
    monkeypatch.setenv("SOHIT_POISON", "165")


def same(got, want):
    for name in ("row_a", "row_b"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype == np.int32 and np.array_equal(g, w), name
    assert got.link.dtype == want.link.dtype == np.int64 and got.link.shape == want.link.shape and np.array_equal(got.link, want.link)
    assert got.counters() == want.counters()


def device(fu, case, stats=None, **kw):
    return fu.device_fusion_links(case.table, case.tax, stats=stats, **dict(case.params, **kw))


@pytest.mark.parametrize("name", sorted(fi.designed()))
def test_designed_tables(fu, name):
    case = fi.designed()[name]
    stats = {}
    got = device(fu, case, stats)
    same(got, case.definition())
    assert fi.as_pairs(got) == sorted(case.links)
    assert stats["waits"] == (0 if len(case.table) == 0 else 2 if len(got) else 1)


@pytest.mark.parametrize("max_overlap", (0, 5))
@pytest.mark.parametrize("same_taxon", (True, False))
def test_rules_under_other_parameters(fu, max_overlap, same_taxon):
    """every designed table once more at the other overlap bound and taxon rule than it was designed for: the definition alone says"""
    for name, case in sorted(fi.designed().items()):
        kw = dict(case.params, max_overlap=max_overlap, same_taxon=same_taxon)
        same(fu.device_fusion_links(case.table, case.tax, **kw), fu.fusion_links(case.table, case.tax, **kw))


def test_run_sizes(fu):
    case = fi.run_sizes_case()
    want = case.definition()
    got = device(fu, case)
    same(got, want)
    assert got.n_reps == sum(fi.RUN_SIZES) and got.n_pairs == sum(m * (m - 1) // 2 for m in fi.RUN_SIZES) and len(got) > 0
    for kw in (dict(max_overlap=40), dict(same_taxon=False), dict(num=0, den=1)):
        p = dict(case.params, **kw)
        same(fu.device_fusion_links(case.table, case.tax, **p), fu.fusion_links(case.table, case.tax, **p))


def test_one_long_run(fu):
    case = fi.long_run_case()
    want = case.definition()
    stats = {}
    got = device(fu, case, stats)
    same(got, want)
    assert got.n_pairs == 3000 * 2999 // 2 and len(got) > 10000 and stats["waits"] == 2
    same(device(fu, case), want)                                        # twice: the same arrays


def test_many_short_runs(fu):
    case = fi.short_runs_case()
    want = case.definition()
    got = device(fu, case)
    same(got, want)
    assert got.n_runs > 15000 and len(got) > 1000


@pytest.mark.parametrize("seed", range(6))
def test_random_tables(fu, seed):
    case = fi.random_case(seed)
    same(device(fu, case), case.definition())


# ---------------------------------------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------------------------------------
def _upload(rec):
    import torch
    return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()


def by_names(names, links):
    """the links as ids: what does not depend on the numbering of the names"""
    nm = names.tolist()
    return [(nm[c], nm[a], nm[b]) + tuple(rest) for c, a, b, *rest in links.link.tolist()]


@pytest.mark.parametrize("which", ("run_sizes", "random", "representatives"))
def test_records_path(fu, which):
    """so_hit records on the device (uploaded with torch), the id lists in another order than the names: the column call's links"""
    case = {"run_sizes": fi.run_sizes_case, "random": lambda: fi.random_case(2), "representatives": fi.representative_case}[which]()
    rec, qids, sids = fi.records_of(case.table)
    p = case.params
    names, got = fu.device_fusion_links_from_records(_upload(rec), qids, sids, p["max_overlap"], p["num"], p["den"], p["same_taxon"])
    want = device(fu, case)
    # (the record call numbers the names in their byte order, the designed table in order of creation: rows, counters and ids are one)
    assert names.tolist() == sorted(case.table.names.tolist())
    assert np.array_equal(got.row_a, want.row_a) and np.array_equal(got.row_b, want.row_b) and got.counters() == want.counters() and len(got) > 0
    assert by_names(names, got) == by_names(case.table.names, case.definition())


def test_records_path_edges(fu):
    import torch
    case = fi.representative_case()
    rec, qids, sids = fi.records_of(case.table)
    names, got = fu.device_fusion_links_from_records(torch.zeros(0, dtype=torch.uint8, device="cuda"), qids, sids)
    assert len(got) == 0 and got.counters() == dict.fromkeys(fu.COUNTERS, 0)
    for field, v, word in (("qidx", len(qids), "qidx lies outside"), ("qidx", -1, "qidx lies outside"), ("sidx", len(sids), "sidx lies outside"),
                           ("qst", 0, "qst < 1"), ("sed", 0, "sed < sst"), ("slen", -1, "slen < 0")):
        r2 = rec.copy()
        r2[field][4] = v
        with pytest.raises(RuntimeError) as e:
            fu.device_fusion_links_from_records(_upload(r2), qids, sids)
        assert word in str(e.value) and str(e.value).startswith("so_fusion_records: ")
    names, got = fu.device_fusion_links_from_records(_upload(rec), qids, sids)        # a refusal leaves nothing behind
    assert by_names(names, got) == by_names(case.table.names, case.definition()) and len(got) == 3


# ---------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------
def test_refusals(fu):
    import torch
    case = fi.dense_case(8)
    t, tax = case.table, case.tax
    want = case.definition()

    def changed(col, v):
        bad = fu.Table(t.names, *(getattr(t, k).copy() for k in ("q", "s", "qst", "qed", "sst", "sed", "slen", "qlen")))
        getattr(bad, col)[3] = v
        return bad

    cases = [(dict(max_overlap=-1), "max_overlap"), (dict(max_overlap=1 << 31), "max_overlap"), (dict(num=-1), "0 <= num <= den < 2^20"),
             (dict(num=11, den=10), "0 <= num <= den < 2^20"), (dict(num=1, den=1 << 20), "0 <= num <= den < 2^20"), (dict(num=0, den=0), "0 <= num <= den < 2^20"),
             (dict(n_taxa=1), "taxon outside"), (dict(device=torch.cuda.device_count()), "device")]
    cases += [(dict(table=changed(c, v)), w) for c, v, w in (("qst", 0, "qst < 1"), ("qed", 5, "qed < qst"), ("sst", 0, "sst < 1"), ("sed", 0, "sed < sst"),
                                                              ("slen", -1, "slen < 0"), ("s", len(tax), "name code"), ("q", -1, "name code"))]
    for change, word in cases:
        kw = dict(case.params, **change)
        with pytest.raises(RuntimeError) as e:
            fu.device_fusion_links(kw.pop("table", t), tax, **kw)
        assert word in str(e.value) and str(e.value).startswith("so_fusion_cols: "), (change, str(e.value))
        same(device(fu, case), want)                                    # a refusal leaves nothing behind: the next call is served
    import ctypes as C
    from swiftortho_amd import _lib
    L, res = _lib.load(), _lib.SoFusionResult()
    none = [None] * 8
    assert L.so_fusion_cols(0, 0, *none, 0, None, 0, 0, 7, 10, 4, C.byref(res)) == 1 and b"unknown flag bits" in L.so_fusion_last_error()
    assert L.so_fusion_cols(0, 1 << 31, *none, 0, None, 0, 0, 7, 10, 1, C.byref(res)) == 1 and b"2^31 rows" in L.so_fusion_last_error()
    assert L.so_fusion_cols(0, 3, *none, 0, None, 0, 0, 7, 10, 1, C.byref(res)) == 1 and b"NULL" in L.so_fusion_last_error()
    assert L.so_fusion_cols(0, 0, *none, 0, None, 0, 0, 7, 10, 1, C.byref(res)) == 0 and res.n_links == 0 and res.waits == 0
    L.so_fusion_free(C.byref(res))
    assert L.so_fusion_records(0, None, 3, None, 0, None, 0, 0, None, 0, 0, 7, 10, 1, C.byref(res)) == 1 and b"record pointer is NULL" in L.so_fusion_last_error()


def test_refusal_by_size(fu):
    """2^31 links: one run of 65 537 pairwise disjoint components is 65 537 x 65 536 / 2 = 2^31 + 32 768 links -- the count pass finds
    them, nothing is emitted.  (The other size limit, links beyond half of the free device memory, lies behind this one on a device of
    this size: 2^31 links take 120 GB.)  With every interval the same there is no link and the counters still say what was walked.
    The one table beyond a few thousand rows: nothing smaller reaches the refusal.  Both calls together take 0.84 s on the MI355X (2^31
    pairs tested and looked up in the first, 2 * 10^9 steps of the representatives' walk in each)."""
    n = 65537
    k = np.arange(n, dtype=np.int64)
    one = np.ones(n, dtype=np.int64)
    names = np.asarray([b"0|q"] + [b"1|g%05d" % i for i in range(n)])
    t = fu.Table(names, 0 * k, 1 + k, 10 * k + 1, 10 * k + 10, one, 100 * one, 100 * one, 1000000 * one)
    tax = np.concatenate([[0], one])
    with pytest.raises(RuntimeError) as e:
        fu.device_fusion_links(t, tax)
    assert str(n * (n - 1) // 2) in str(e.value) and "2^31" in str(e.value)
    t.qst, t.qed = one, 10 * one
    got = fu.device_fusion_links(t, tax)
    assert len(got) == 0 and got.counters() == dict(n_runs=1, n_eligible=n, n_reps=n, n_pairs=n * (n - 1) // 2, n_disjoint=0)


# ---------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------
def test_script_G_T_equals_G_F(fu, tmp_path):
    text = fi.sc_text(fi.run_sizes_case().table)
    out = {}
    for g in "FT":
        d = tmp_path / g
        d.mkdir()
        open(str(d / "in.sc"), "w").write(text)
        r = subprocess.run([sys.executable, SCRIPT, "-i", str(d / "in.sc"), "-o", "3", "-x", str(d / "o.xyz"), "-G", g], capture_output=True, cwd=str(d))
        assert r.returncode == 0, r.stderr[-2000:]
        out[g] = (r.stdout, open(str(d / "o.xyz"), "rb").read())
    assert out["T"] == out["F"] and out["F"][0].count(b"\n") > 100 and 0 < out["F"][1].count(b"\n") < out["F"][0].count(b"\n")
    # a refusal of the device call: exit code 2, one line, nothing written (with -G F the same row is refused by the definition)
    bad = text.split("\n")
    f = bad[5].split("\t")
    bad[5] = "\t".join(f[:6] + ["0"] + f[7:])
    for g in "FT":
        d = tmp_path / ("bad" + g)
        d.mkdir()
        open(str(d / "in.sc"), "w").write("\n".join(bad))
        r = subprocess.run([sys.executable, SCRIPT, "-i", str(d / "in.sc"), "-x", str(d / "o.xyz"), "-G", g], capture_output=True, cwd=str(d))
        # (the one line of the script: a driver may have written a line of its own to the process's stderr when the device was opened)
        own = [l for l in r.stderr.split(b"\n") if l.startswith(b"fusion_links: ")]
        assert r.returncode == 2 and r.stdout == b"" and not os.path.exists(str(d / "o.xyz")) and len(own) == 1 and b"qst < 1" in own[0] and b"Traceback" not in r.stderr
    assert own[0].startswith(b"fusion_links: so_fusion_cols: ") and r.stderr.endswith(own[0] + b"\n")


def run_all_fast(d, extra, fasta=None):
    d.mkdir()
    fas = str(d / "p.fsa")
    if fasta is None:
        shutil.copy(os.path.join(ROOT, "tests", "golden", "nr_dups.fsa"), fas)
    else:
        open(fas, "wb").write(fasta)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_all_fast.py"), "-i", fas, "-s", "111111", "-a", "1", "-v", "500", "-y", "0"] + list(extra),
                       capture_output=True, text=True, env=dict(os.environ, PYTHONHASHSEED="0"))
    assert p.returncode == 0, p.stderr[-3000:]
    res = fas + "_results"
    return {f: open(os.path.join(res, f), "rb").read() for f in sorted(os.listdir(res))}


def test_run_all_fast_F_T(fu, tmp_path):
    """-F T leaves <name>.fusion.tsv, <name>.fusion.xyz and <name>.fusion.clsr, with and without the device the same bytes; without -F
    every file is what it was and no other exists"""
    fasta = open(os.path.join(ROOT, "tests", "golden", "nr_dups.fsa"), "rb").read() + fi.fusion_fasta()
    plain = run_all_fast(tmp_path / "plain", ("-G", "T"), fasta)
    dev = run_all_fast(tmp_path / "dev", ("-F", "T", "-G", "T"), fasta)
    host = run_all_fast(tmp_path / "host", ("-F", "T"), fasta)
    new = {"p.fsa.fusion.tsv", "p.fsa.fusion.xyz", "p.fsa.fusion.clsr"}
    assert set(dev) == set(plain) | new and not new & set(plain)
    for f in plain:
        assert dev[f] == plain[f], f
    for f in new:
        assert dev[f] == host[f], f
    tsv = dev["p.fsa.fusion.tsv"].decode().split("\n")
    assert tsv[0] == fu.HEADER and tsv[-1] == "" and len(tsv) >= 4
    assert {tuple(l.split("\t")[:3]) for l in tsv[1:-1]} >= {(fi.COMPOSITE.decode(), a.decode(), b.decode()) for a, b in fi.COMPONENT_PAIRS}
    assert b"X|A\tX|B\t1\n" in dev["p.fsa.fusion.xyz"] and b"Z|A\tZ|B\t1\n" in dev["p.fsa.fusion.xyz"]
    # the modules are what find_cluster makes of the .xyz file (its own tests say which): members of it, each once, a line at least
    members = dev["p.fsa.fusion.clsr"].decode().split()
    assert len(members) == len(set(members)) >= 2 and set(members) <= {g for l in dev["p.fsa.fusion.xyz"].decode().split("\n") if l for g in l.split("\t")[:2]}
    assert dev["p.fsa.fusion.clsr"].count(b"\n") >= 1


def test_pipeline_end_to_end(fu, tmp_path):
    """a proteome with one fusion, from the FASTA file to the links in one process: C with (X|A, X|B) and with (Z|A, Z|B) and no composite
    other than C; the same text from the script on the .sc file of the same search, with and without the device, collapsed or not"""
    from swiftortho_amd import pipeline
    p, sc = str(tmp_path / "f.fsa"), str(tmp_path / "f.sc")
    open(p, "wb").write(fi.fusion_fasta())
    names, links, t = pipeline.fusion_links_from_search(p, sc_path=sc, **SEARCH_KW)
    nm = names.tolist()
    assert {nm[c] for c in links.link[:, 0].tolist()} == {fi.COMPOSITE}
    assert {(nm[a], nm[b]) for a, b in links.link[:, 1:3].tolist()} == fi.COMPONENT_PAIRS and len(links) == 2 == t["links"] and t["rows"] > 10 and "fusion" in t
    text = fu.links_text(names, links)
    for g in "FT":
        r = subprocess.run([sys.executable, SCRIPT, "-i", sc, "-G", g], capture_output=True)
        assert r.returncode == 0 and r.stdout.decode() == text, r.stderr[-2000:]
    for kw in (dict(device_stage=False), dict(collapse=True)):
        names2, links2, _ = pipeline.fusion_links_from_search(p, **dict(SEARCH_KW, **kw))
        assert fu.links_text(names2, links2) == text, kw
    # every test but homology switched off: still no composite other than C
    names, links, _ = pipeline.fusion_links_from_search(p, coverage="0", max_overlap=1000, same_taxon=False, **SEARCH_KW)
    assert {names.tolist()[c] for c in links.link[:, 0].tolist()} == {fi.COMPOSITE}
