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


_ORACLE = {}


def oracle_strings(oracle, ref, qry, kw, tmp_path, ranges=None):
    """-> (the oracle's rows as text, every row's (query string, subject string)); cached per input and flags"""
    import hashlib
    key = (hashlib.sha1(ref).hexdigest(), hashlib.sha1(qry).hexdigest(), tuple(sorted(kw.items())), tuple(map(tuple, ranges or [])))
    if key not in _ORACLE:
        rp, qp = tmp_path / "oracle_r.fsa", tmp_path / "oracle_q.fsa"
        rp.write_bytes(ref), qp.write_bytes(qry)
        text, alns = b"", []
        for k, (lo, hi) in enumerate(ranges or [(-1, -1)]):
            out = str(tmp_path / ("oracle%d.sc" % k))
            r = oracle.blastp_parallel(str(qp), str(rp), out, threads=16, st=lo, ed=hi, alignments=True, **kw)
            text += open(out, "rb").read()
            assert r.alignments is not None and len(r.alignments) == len(r.ints)
            alns += r.alignments
        _ORACLE[key] = (text, alns)
    return _ORACLE[key]


def assert_same_strings(got_rows, got_alns, want_rows, want_alns, what=""):
    """the rows, then every row's strings byte for byte (the first difference shown)"""
    assert got_rows == want_rows, what
    assert len(got_alns) == len(want_alns) > 0, what
    for k, (g, w) in enumerate(zip(got_alns, want_alns)):
        if g != w:
            row = want_rows.split(b"\n")[k]
            pytest.fail("%s: row %d (%d rows) differs: %r\n gpu    %r\n        %r\n oracle %r\n        %r"
                        % (what, k, len(want_alns), row[:120], g[0][:200], g[1][:200], w[0][:200], w[1][:200]))


@pytest.fixture(scope="module")
def het_oracle(oracle, het_default, tmp_path_factory):
    fa, _ = het_default
    return oracle_strings(oracle, fa, fa, HET_KW, tmp_path_factory.mktemp("het"))


@pytest.mark.parametrize("env", [{"SOHIT_ALIGN_PK": "0"}, {"SOHIT_SPEC": "1"}, {"SOHIT_SPEC": "0"}, {"SOHIT_TRACE_WAVE_ROWS": "0"},
                                 {"SOHIT_TRACE_WAVE_ROWS": "16", "SOHIT_TRACE_WAVE_MAX": "100000000"}, {"SOHIT_EMIT_PARTS": "1"},
                                 {"SOHIT_BATCH": "700"}, {"SOHIT_POISON": "0xFF"}],
                         ids=["no_packed", "kept_traces", "no_kept_traces", "every_walk_by_a_thread", "every_walk_by_a_wave", "one_range",
                              "small_batches", "poison"])
def test_path_switches_give_the_same_strings(fs, het_default, het_oracle, monkeypatch, env):
    fa, (rows0, recs0, alns0, _) = het_default
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rows, recs, alns, _ = search(fs, fa, fa, HET_KW)
    assert recs == recs0
    assert alns == alns0
    assert_same_strings(rows, alns, *het_oracle, what=str(env))


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


# ---- every row's strings against the oracle's (oracle.blastp(alignments=True): kswat_st's al0 / al1 of the row's own alignment or tile)

def test_strings_equal_the_oracle_synthetic(fs, oracle, tmp_path):
    from swiftortho_amd import synthprot
    fa = synthprot.synthprot(2000, 250, 7)
    kw = dict(ssd="111111", nr=AA9, ht=120000000, chk=50000, step=1, v=500, expect=1e-5, flt="T")
    rows, _, alns, _ = search(fs, fa, fa, kw)
    assert_same_strings(rows, alns, *oracle_strings(oracle, fa, fa, kw, tmp_path), what="synthetic")


def test_strings_equal_the_oracle_het(fs, het_default, het_oracle):
    fa, (rows, _, alns, _) = het_default
    assert_same_strings(rows, alns, *het_oracle, what="het")


def test_strings_equal_the_oracle_long_tiles(fs, oracle, tmp_path):
    """the 40 000-residue set: rows of kswat_st_long tiles, each with its own tile's strings"""
    fa = long_fasta()
    kw = dict(ssd="111111", nr=AA9, ht=1000003, chk=50000, step=1, v=500, expect=1e-5, flt="T")
    rows, recs, alns, _ = search(fs, fa, fa, kw)
    r = np.frombuffer(recs, dtype=np.uint8).reshape(-1, 80)
    qlen = r[:, 64:68].copy().view("<i4").ravel()
    slen = r[:, 68:72].copy().view("<i4").ravel()
    assert ((qlen > 4096) & (slen > 4096)).sum() >= 10   # tile rows
    assert_same_strings(rows, alns, *oracle_strings(oracle, fa, fa, kw, tmp_path), what="long")


def tandem_fasta():
    """homopolymers and tandem repeats of period 1 .. 11 with a few point changes (test_gpu_parity.py's set)"""
    from swiftortho_amd import synthprot
    rng = np.random.default_rng(23)
    aa = "ACDEFGHIKLMNPQRSTVWY"
    recs = []
    for k, period in enumerate((1, 1, 2, 3, 5, 7, 11, 4, 9)):
        unit = "".join(aa[int(x)] for x in rng.integers(0, 20, period))
        for c in range(3):
            n = int(rng.integers(120, 420))
            s = (unit * (n // period + 1))[:n]
            b = list(s)
            for p in rng.integers(0, n, size=n // 25):
                b[int(p)] = aa[int(rng.integers(0, 20))]
            recs.append(("rep%d_%d_%d" % (period, k, c), "".join(b)))
    return "".join(">%s\n%s\n" % r for r in recs).encode() + synthprot.synthprot(60, 150, 8)


@pytest.mark.parametrize("flt", ["F", "T"])
def test_strings_equal_the_oracle_tandem_repeats(fs, oracle, tmp_path, flt):
    """co-optimal paths everywhere: which column of a run takes the gap is decided by the walk's tie order alone"""
    fa = tandem_fasta()
    kw = dict(ssd="111111,1101011", nr=AA9, ht=1000003, chk=20, step=1, v=500, expect=1e-3, flt=flt)
    rows, _, alns, _ = search(fs, fa, fa, kw)
    assert any(a.count(b"-") for a, _ in alns)
    assert_same_strings(rows, alns, *oracle_strings(oracle, fa, fa, kw, tmp_path), what="tandem " + flt)


def odd_byte_sets():
    """(reference, queries): homologs with literal '-' (runs too), '*', '.', digits, lower case and rare letters inside their aligned
    regions, plus test_gpu_parity.py's FASTA quirks (a '>' inside a line, blank lines, blanks inside lines, duplicate ids)"""
    from swiftortho_amd import synthprot
    rng = np.random.default_rng(78)
    base = synthprot.synthprot(80, 140, 6).decode().strip().split("\n")
    odd = ["-", "--", "---", "*", ".", "0", "7", "x", "a", "k", "U", "J", "B", "-*-"]
    recs = []
    for i in range(0, len(base), 2):
        sq = list(base[i + 1])
        for p in sorted(rng.integers(8, len(sq) - 8, size=int(rng.integers(1, 6))), reverse=True):
            sq[int(p):int(p) + 1] = list(odd[int(rng.integers(0, len(odd)))])
        recs.append(base[i] + "\n" + "".join(sq) + "\n")
    ref = "".join(recs).encode()
    s0, s1 = base[1], base[3]
    quirks = b"".join([b">gt_inside\n" + (s0[:40] + ">" + s0[40:]).encode() + b"\n",
                       b">blank_lines\n" + s1[:30].encode() + b"\n\n" + s1[30:].encode() + b"\n\n",
                       b">spaces in\theader\n" + (s0[:20] + "  " + s0[20:]).encode() + b"\n",
                       b">dup\n" + s1.encode() + b"\n", b">dup\n" + s1.encode() + b"\n"])
    qry = b"".join(recs[k].encode() for k in range(0, len(recs), 3)) + quirks
    return ref + quirks, qry


def test_strings_equal_the_oracle_odd_bytes(fs, oracle, tmp_path):
    ref, qry = odd_byte_sets()
    kw = dict(ssd="111111", nr=AA9, ht=1000003, chk=50000, step=1, v=500, expect=1e-3, flt="T")
    rows, _, alns, _ = search(fs, ref, qry, kw)
    assert sum(any(x == y == 45 for x, y in zip(a0, a1)) for a0, a1 in alns) >= 1   # a literal '-' opposite a gap
    assert_same_strings(rows, alns, *oracle_strings(oracle, ref, qry, kw, tmp_path), what="odd bytes")


def test_strings_equal_the_oracle_query_longer(fs, oracle, tmp_path):
    """a separate query file whose homologs are LONGER than their subjects (extended at both ends, with indels): the reference swaps
    the sequences, and its lists back"""
    from swiftortho_amd import synthprot
    rng = np.random.default_rng(79)
    aa = "ACDEFGHIKLMNPQRSTVWY"
    base = synthprot.synthprot(300, 160, 10).decode().strip().split("\n")
    qrecs = []
    for i in range(0, len(base), 2):
        sq = list(base[i + 1])
        for _ in range(int(rng.integers(0, 4))):
            p = int(rng.integers(5, len(sq) - 5))
            if rng.random() < 0.5:
                del sq[p:p + int(rng.integers(1, 3))]
            else:
                sq[p:p] = [aa[int(x)] for x in rng.integers(0, 20, int(rng.integers(1, 3)))]
        ext = lambda n: "".join(aa[int(x)] for x in rng.integers(0, 20, n))
        qrecs.append(">q%s\n%s%s%s\n" % (base[i][1:].split()[0], ext(int(rng.integers(5, 40))), "".join(sq), ext(int(rng.integers(5, 40)))))
    qry = "".join(qrecs[::2]).encode()
    ref = "\n".join(base).encode() + b"\n"
    kw = dict(ssd="111111", nr=AA9, ht=1000003, chk=50000, step=1, v=500, expect=1e-5, flt="T")
    rows, recs, alns, _ = search(fs, ref, qry, kw)
    r = np.frombuffer(recs, dtype=np.uint8).reshape(-1, 80)
    qlen = r[:, 64:68].copy().view("<i4").ravel()
    slen = r[:, 68:72].copy().view("<i4").ravel()
    assert (qlen > slen).sum() >= 50
    assert_same_strings(rows, alns, *oracle_strings(oracle, ref, qry, kw, tmp_path), what="query longer")


@pytest.mark.parametrize("alignments", [True, False])
def test_slab_route_and_kept_trace_fallback(fs, oracle, tmp_path, monkeypatch, capfd, alignments):
    """SOHIT_TRACE_VAR_MAX lowers the trace budgets: every emission range's traced rows go through the fixed-stride slabs (several per
    range) and the first round's kept traces do not fit (their tasks are scored only).  Rows -- and strings -- are the oracle's."""
    fa = het_fasta(1200, 13)
    for k, v in {"SOHIT_TRACE_VAR_MAX": "4096", "SOHIT_SPEC": "1", "SOHIT_SPEC_SLACK": "1e30", "SOHIT_EMIT_PARTS": "2",
                 "SOHIT_EMIT_MIN_ROWS": "1", "SOHIT_DEBUG": "1"}.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    rows, _, alns, _ = search(fs, fa, fa, HET_KW, alignments=alignments)
    err = capfd.readouterr().err
    assert "[sohit] kept traces do not fit" in err and "[sohit] trace slabs:" in err, err[-2000:]
    import re
    slabs = [tuple(map(int, m)) for m in re.findall(r"\[sohit\] trace slabs: (\d+) rows of (\d+) per range at most, (\d+) tasks per slab", err)]
    assert any(per_range > 2 * slab for _, per_range, slab in slabs), slabs   # a range spans several slabs
    want_rows, want_alns = oracle_strings(oracle, fa, fa, HET_KW, tmp_path)
    if alignments:
        assert_same_strings(rows, alns, want_rows, want_alns, what="slab route")
    else:
        assert rows == want_rows and alns is None
