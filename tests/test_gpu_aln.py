"""GPU tests of the alignment strings behind every row (Searcher.search(..., alignments=True), so_search_loaded_aln).

The strings are the REAL reference's kswat_st al0 / al1 for every row of the aln_<name>.json fixtures
(tools/refharness/make_aln_goldens.py); elsewhere they must agree with the rows they belong to, follow a path in the band,
be the same under every switch that picks another path through the aligners and walks, and asking for them must change no row.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLD

pytestmark = pytest.mark.gpu

AA9 = "AST,CFILMVY,DN,EQ,G,H,KR,P,W"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def aln_golden_names():
    return sorted(f[4:-5] for f in os.listdir(GOLD) if f.startswith("aln_") and f.endswith(".json"))


def flags_to_kwargs(flags):
    d = dict(zip(flags[0::2], flags[1::2]))
    return dict(ssd=d.get("-s", "111111"), nr=d.get("-r", AA9), ht=int(d.get("-M", -1)), chk=int(d.get("-c", 50000)), step=int(d.get("-j", 4)),
                v=int(d.get("-v", 500)), thr=int(d.get("-t", -1)), expect=float(d.get("-e", 1e-3)), max_miss=float(d.get("-m", 1e-3)),
                flt=d.get("-F", "T"))


@pytest.fixture(scope="module")
def fs():
    from swiftortho_amd import fsearch
    return fsearch


def search(fs, ref, qry, kw, ranges=None, alignments=True):
    """-> (row text, records, [(query string, subject string)] or None, counters)"""
    s = fs.Searcher(**kw)
    try:
        s.load_ref_bytes(ref)
        s.load_queries_bytes(qry)
        rows, recs, alns = [], [], []
        for lo, hi in ranges or [(-1, -1)]:
            h = s.search(lo, hi, alignments=alignments)
            rows += h.rows()
            recs.append(h.raw_bytes())
            if alignments:
                alns += [h.alignment(k) for k in range(len(h))]
            h.close()
        return b"".join(rows), b"".join(recs), (alns if alignments else None), s.counters()
    finally:
        s.close()


@pytest.mark.parametrize("name", aln_golden_names())
def test_strings_equal_the_real_reference(fs, oracle, name):
    from test_aln_fixtures import fixture
    _, gold, want = fixture(name, oracle)
    meta = json.load(open(os.path.join(GOLD, name + ".json")))
    ref = open(os.path.join(GOLD, name + ".ref.fsa"), "rb").read()
    qry = open(os.path.join(GOLD, name + ".qry.fsa"), "rb").read() if meta.get("separate_query") else ref
    rows, _, alns, _ = search(fs, ref, qry, flags_to_kwargs(meta["flags"]), ranges=meta.get("ranges"))
    assert rows == open(os.path.join(GOLD, name + ".sc"), "rb").read()
    assert len(want) > 0 and gold["left_out"] + gold["unmatched"] <= len(want) // 20
    for k, w in want.items():
        assert alns[k] == w, "row %d: %r" % (k, alns[k])


def het_fasta(n, seed):
    from swiftortho_amd import synthprot
    return synthprot.synthprot(n, seed=seed, lengths="lognormal")


def long_fasta():
    """the 40 000-residue set of test_gpu_parity.py (ten 4096-tiles per alignment)"""
    from swiftortho_amd import synthprot
    rng = np.random.default_rng(3)
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)

    def rnd(n):
        return aa[rng.integers(0, 20, n)].tobytes().decode()

    def mut(s, d):
        b = np.frombuffer(s.encode(), dtype=np.uint8).copy()
        m = rng.random(len(b)) < d
        b[m] = aa[rng.integers(0, 20, int(m.sum()))]
        return b.tobytes().decode()

    A = rnd(40000)
    recs = [("T0", A), ("T1", mut(A[1000:39000], 0.2)), ("T2", mut(A[20000:33000], 0.1)), ("S0", mut(A[35000:35400], 0.1)),
            ("R", "MKV" * 700)]
    return "".join(">%s\n%s\n" % r for r in recs).encode() + synthprot.synthprot(300, 250, 9)


HET_KW = dict(ssd="111111", nr=AA9, ht=120000000, chk=50000, step=1, v=500, expect=1e-5, flt="T")


@pytest.fixture(scope="module")
def het_default(fs):
    fa = het_fasta(3000, 11)
    return fa, search(fs, fa, fa, HET_KW)


@pytest.mark.parametrize("env", [{"SOHIT_ALIGN_PK": "0"}, {"SOHIT_SPEC": "1"}, {"SOHIT_SPEC": "0"}, {"SOHIT_TRACE_WAVE_ROWS": "0"},
                                 {"SOHIT_TRACE_WAVE_ROWS": "16", "SOHIT_TRACE_WAVE_MAX": "100000000"}, {"SOHIT_EMIT_PARTS": "1"},
                                 {"SOHIT_BATCH": "700"}, {"SOHIT_POISON": "0xFF"}],
                         ids=["no_packed", "kept_traces", "no_kept_traces", "every_walk_by_a_thread", "every_walk_by_a_wave", "one_range",
                              "small_batches", "poison"])
def test_path_switches_give_the_same_strings(fs, het_default, monkeypatch, env):
    fa, (rows0, recs0, alns0, _) = het_default
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rows, recs, alns, _ = search(fs, fa, fa, HET_KW)
    assert recs == recs0
    assert alns == alns0


def masked_queries(fs, fa, kw):
    """the queries as the aligner sees them (SEG under flt='T'): so_masked_query"""
    os.environ["SOHIT_KEEP_MASKED"] = "1"
    try:
        s = fs.Searcher(**kw)
        s.load_ref_bytes(fa)
        s.load_queries_bytes(fa)
        h = s.search()
        h.close()
        out = [s.masked_query(q) for q in range(s.num_queries)]
        s.close()
    finally:
        del os.environ["SOHIT_KEEP_MASKED"]
    return out


def check_consistent(fs, fa, kw, recs, alns):
    from swiftortho_amd import fsearch
    dt = np.dtype([(n, t) for n, t in (("qidx", "<i8"), ("sidx", "<i8"), ("identity", "<f8"), ("evalue", "<f8"), ("aln", "<i4"), ("mis", "<i4"),
                                      ("gap", "<i4"), ("qst", "<i4"), ("qed", "<i4"), ("sst", "<i4"), ("sed", "<i4"), ("bit", "<i4"),
                                      ("qlen", "<i4"), ("slen", "<i4"), ("matches", "<i4"), ("ungapped", "<i4"))])
    r = np.frombuffer(recs, dtype=dt)
    assert len(r) == len(alns) > 0
    subj = [l for l in fa.split(b"\n")[1::2]]
    qm = masked_queries(fs, fa, kw)
    qm = [q if isinstance(q, bytes) else q.encode("latin-1") for q in qm]
    for k in range(len(r)):
        a0, a1 = alns[k]
        h = r[k]
        assert len(a0) == len(a1) == h["aln"]
        matches, mis, gap, idy = fsearch.aln_stats(a0, a1)
        assert (matches, mis, gap) == (h["matches"], h["mis"], h["gap"]), k
        assert np.float64(idy).tobytes() == np.float64(h["identity"]).tobytes(), k
        assert a0.replace(b"-", b"") == qm[h["qidx"]][h["qst"] - 1:h["qed"]], k
        assert a1.replace(b"-", b"") == subj[h["sidx"]][h["sst"] - 1:h["sed"]], k
        # a path in the band of its tile: i (query side) and j (subject side) step by at most one each, never both stay;
        # |i - j| - the start's offset stays within the band (kbound 16, plus the boundary walk through row/column 0)
        g0 = np.frombuffer(a0, dtype=np.uint8) == 45
        g1 = np.frombuffer(a1, dtype=np.uint8) == 45
        assert not np.any(g0 & g1), k
        drift = np.cumsum(g1.astype(np.int64) - g0.astype(np.int64))
        span = int(drift.max(initial=0) - drift.min(initial=0))
        assert span <= 2 * 17 + abs((h["qed"] - h["qst"]) - (h["sed"] - h["sst"])), k


def test_every_row_consistent_synthetic(fs):
    from swiftortho_amd import synthprot
    fa = synthprot.synthprot(2000, 250, 7)
    kw = dict(ssd="111111", nr=AA9, ht=120000000, chk=50000, step=1, v=500, expect=1e-5, flt="T")
    _, recs, alns, _ = search(fs, fa, fa, kw)
    check_consistent(fs, fa, kw, recs, alns)


def test_every_row_consistent_het(fs, het_default):
    fa, (_, recs, alns, _) = het_default
    check_consistent(fs, fa, HET_KW, recs, alns)


def test_every_row_consistent_long(fs):
    fa = long_fasta()
    kw = dict(ssd="111111", nr=AA9, ht=1000003, chk=50000, step=1, v=500, expect=1e-5, flt="T")
    _, recs, alns, _ = search(fs, fa, fa, kw)
    check_consistent(fs, fa, kw, recs, alns)


def test_asking_changes_no_row(fs, het_default):
    fa, (rows1, recs1, _, c1) = het_default
    rows0, recs0, none, c0 = search(fs, fa, fa, HET_KW, alignments=False)
    assert none is None
    assert recs0 == recs1 and rows0 == rows1
    for k in ("rows", "seed_hits", "candidates", "alignments", "n_queries", "cells"):
        assert c0[k] == c1[k], k


def test_sub_range_strings_equal_the_full_run(fs, het_default):
    fa, (_, recs, alns, _) = het_default
    r = np.frombuffer(recs, dtype=np.uint8).reshape(-1, 80)
    qidx = r[:, :8].copy().view("<i8").ravel()
    lo, hi = 700, 1900
    _, recs2, alns2, _ = search(fs, fa, fa, HET_KW, ranges=[(lo, hi)])
    sel = np.nonzero((qidx >= lo) & (qidx < hi))[0]
    assert recs2 == r[sel].tobytes()
    assert alns2 == [alns[k] for k in sel]


def test_halves_rerun_keeps_the_strings(fs):
    code = r'''
import os, sys
sys.path.insert(0, %r)
from swiftortho_amd import fsearch, synthprot
fa = synthprot.synthprot(900, seed=3, lengths="lognormal")
kw = dict(ssd="111111", nr="AST,CFILMVY,DN,EQ,G,H,KR,P,W", ht=120000000, chk=400, step=1, v=500, expect=1e-5, flt="T")
def run():
    s = fsearch.Searcher(**kw)
    s.load_ref_bytes(fa); s.load_queries_bytes(fa)
    h = s.search(alignments=True)
    raw, al = h.raw_bytes(), [h.alignment(k) for k in range(len(h))]
    h.close(); s.close()
    return raw, al
want = run()
os.environ["SOHIT_TEST_OOM_PHASE2"] = "1"
got = run()
assert got[0] == want[0] and len(want[1]) > 500, (len(got[0]), len(want[0]))
assert got[1] == want[1]
print("OOM_ALN_OK")
''' % ROOT
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "OOM_ALN_OK" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
