"""GPU tests of the CIGAR behind every row (Searcher.search(..., cigar=True), so_search_loaded_cigar, find_hit.py -C T).

The runs are coded on the GPU from the columns the traceback walks write (k_cigar_count, scan, k_cigar_emit).  They must be the REAL
reference's for every row of the aln_<name>.json fixtures and every case of kswat_aln_edges.json, rebuild the oracle's strings for
every row of the synthetic sets, say what the strings of the same search say, stay the same under every switch that picks another
path through the aligners and walks -- and asking for them must change no row.

Where a sequence holds a literal '-' byte a CIGAR derived from strings (the goldens' were) is ambiguous: for such rows the two CIGARs
are compared through the strings they rebuild.  That is a condition on the row's sequences, not a tolerance.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLD

from test_gpu_aln import (HET_KW, ROOT, aln_golden_names, flags_to_kwargs, fs, het_default, het_fasta, het_oracle, long_fasta,  # noqa: F401
                          odd_byte_sets, oracle_strings, tandem_fasta)

pytestmark = pytest.mark.gpu

AA9 = "AST,CFILMVY,DN,EQ,G,H,KR,P,W"
DT = np.dtype([(n, t) for n, t in (("qidx", "<i8"), ("sidx", "<i8"), ("identity", "<f8"), ("evalue", "<f8"), ("aln", "<i4"), ("mis", "<i4"),
                                   ("gap", "<i4"), ("qst", "<i4"), ("qed", "<i4"), ("sst", "<i4"), ("sed", "<i4"), ("bit", "<i4"),
                                   ("qlen", "<i4"), ("slen", "<i4"), ("matches", "<i4"), ("ungapped", "<i4"))])
# the rows whose query or subject holds a literal '-' (counted over tests/golden/ on the CPU): every other row is compared CIGAR to CIGAR
DASH_ROWS = {"toy_ragged": 2, "toy_oddchars": 23}


def search_cigar(fs, ref, qry, kw, ranges=None, masked=False):
    """-> (row text, records, [uint32 runs per row], [CIGAR text per row], counters, the queries as the aligner saw them or None)"""
    s = fs.Searcher(**kw)
    try:
        if masked:
            s.set_option("SOHIT_KEEP_MASKED", "1")
        s.load_ref_bytes(ref)
        s.load_queries_bytes(qry)
        rows, recs, runs, text = [], [], [], []
        for lo, hi in ranges or [(-1, -1)]:
            h = s.search(lo, hi, cigar=True)
            rows += h.rows()
            recs.append(h.raw_bytes())
            ops, off = h.cigar_buffer()
            assert len(off) == len(h) + 1 and off[0] == 0 and off[len(h)] == len(ops)
            runs += [ops[int(off[k]):int(off[k + 1])].copy() for k in range(len(h))]
            text += [h.cigar(k) for k in range(len(h))]
            with pytest.raises(fs.SohitError):
                h.alignment(0)
            h.close()
        qm = [s.masked_query(q) for q in range(s.num_queries)] if masked else None
        return b"".join(rows), b"".join(recs), runs, text, s.counters(), qm
    finally:
        s.close()


def sequences(data):
    """the sequences of a FASTA text in file order, lines joined (test_aln_fixtures.records, by position instead of by id)"""
    out = []
    for rec in data.split(b"\n>"):
        rec = rec[1:] if rec.startswith(b">") else rec
        if rec.strip():
            out.append(b"".join(rec.split(b"\n")[1:]))
    return out


def check_canonical(runs, h, what=""):
    """no run of no columns, no unknown operation, neighbours differ; the three length sums of the row"""
    ln, op = (runs >> 4).astype(np.int64), (runs & 15).astype(np.int64)
    assert (ln > 0).all() and (op <= 2).all(), what
    assert (op[1:] != op[:-1]).all(), what
    assert ln.sum() == h["aln"], what
    assert ln[op != 2].sum() == h["qed"] - h["qst"] + 1 and ln[op != 1].sum() == h["sed"] - h["sst"] + 1, what


def check_against_strings(fs, recs, runs, text, qm, subj, want_alns, what):
    """every row: canonical runs, the sums, the text is the runs', and the CIGAR rebuilds the wanted strings from the sequences"""
    r = np.frombuffer(recs, dtype=DT)
    assert len(r) == len(runs) == len(text) == len(want_alns) > 0, what
    for k in range(len(r)):
        h = r[k]
        check_canonical(runs[k], h, (what, k))
        assert text[k] == "".join("%d%s" % (v >> 4, "MID"[v & 15]) for v in runs[k].tolist()), (what, k)
        got = fs.cigar_to_strings(runs[k], qm[h["qidx"]], subj[h["sidx"]], int(h["qst"]), int(h["sst"]))
        if got != want_alns[k]:
            pytest.fail("%s: row %d of %d: %s rebuilds\n gpu    %r\n        %r\n wanted %r\n        %r"
                        % (what, k, len(r), text[k], got[0][:200], got[1][:200], want_alns[k][0][:200], want_alns[k][1][:200]))


# ---- 1. the REAL reference ----------------------------------------------------------------------------------------------------------

def test_the_exempt_rows_are_the_counted_ones():
    from test_aln_fixtures import records
    seen = {}
    for name in aln_golden_names():
        meta = json.load(open(os.path.join(GOLD, name + ".json")))
        ref = open(os.path.join(GOLD, name + ".ref.fsa"), "rb").read()
        qry = open(os.path.join(GOLD, name + ".qry.fsa"), "rb").read() if meta.get("separate_query") else ref
        n = sum(b"-" in s for d in (records(ref), records(qry)) for v in d.values() for s in v)
        if n:
            seen[name] = n
    assert sorted(seen) == sorted(DASH_ROWS)   # none of the other eight goldens holds the byte: no row of theirs is exempt


@pytest.mark.parametrize("name", aln_golden_names())
def test_cigars_equal_the_real_reference(fs, oracle, name):
    from test_aln_fixtures import fixture, records
    rows_gold, gold, want = fixture(name, oracle)
    meta = json.load(open(os.path.join(GOLD, name + ".json")))
    ref = open(os.path.join(GOLD, name + ".ref.fsa"), "rb").read()
    qry = open(os.path.join(GOLD, name + ".qry.fsa"), "rb").read() if meta.get("separate_query") else ref
    seg = dict(zip(meta["flags"][0::2], meta["flags"][1::2])).get("-F", "T") == "T"
    rows, recs, runs, text, _, _ = search_cigar(fs, ref, qry, flags_to_kwargs(meta["flags"]), ranges=meta.get("ranges"))
    assert rows == open(os.path.join(GOLD, name + ".sc"), "rb").read()
    assert len(want) > 0 and gold["left_out"] + gold["unmatched"] <= len(want) // 20
    r = np.frombuffer(recs, dtype=DT)
    qs, ss = records(qry), records(ref)
    exempt = 0
    for k, cig in gold["rows"]:
        c = rows_gold[k].split(b"\t")
        q, s = qs[c[0]][0], ss[c[1]][0]
        check_canonical(runs[k], r[k], (name, k))
        if b"-" in q or b"-" in s:
            exempt += 1
            qa = oracle.seg(q) if seg else q
            qa = qa if isinstance(qa, bytes) else qa.encode("latin-1")
            assert fs.cigar_to_strings(text[k], qa, s, int(c[6]), int(c[8])) == fs.cigar_to_strings(cig, qa, s, int(c[6]), int(c[8])) == want[k], (name, k)
        else:
            assert text[k] == cig, "row %d: %s, the reference has %s" % (k, text[k], cig)
    assert exempt == DASH_ROWS.get(name, 0)


# ---- 2. task by task at the edges ---------------------------------------------------------------------------------------------------

def test_edge_fixture_cigars(fs, oracle):
    from test_aln_fixtures import aln_edge_cases
    from test_gpu_align import TRACED, Set, check
    cases = aln_edge_cases()
    rowmax = np.maximum(0, oracle.b62_matrix().max(axis=1))
    seqs = [x.decode("latin-1") for x in cases[0]["seqs"]]
    st = Set(fs, seqs, seqs)
    tasks = [(c["q"], c["s"], c["qlo"] + min(c["qst"], c["qhi"] - c["qlo"]), c["slo"] + min(c["sst"], c["shi"] - c["slo"]), c["qhi"], c["shi"])
             for c in cases]
    assert any(c["out"] is None for c in cases) and any(b"-" in c["qw"] + c["sw"] for c in cases)
    for mode in TRACED:
        take = [k for k, t in enumerate(tasks) if not (mode == 4 and st.wide(t, rowmax))]
        sub = [tasks[k] for k in take]
        got, runs = st.s.align_pairs(sub, mode, cigar=True)
        check(oracle, st, sub, got, mode, "edge fixture, CIGARs")
        assert np.array_equal(got, st.s.align_pairs(sub, mode)), "asking for the CIGARs changed the records"
        # (a permuted launch list: the runs land per task)
        got_r, runs_r = st.s.align_pairs(sub, mode, order=np.arange(len(sub))[::-1].copy(), cigar=True)
        assert np.array_equal(got_r, got) and all(np.array_equal(a, b) for a, b in zip(runs, runs_r))
        for j, k in enumerate(take):
            c = cases[k]
            what = "mode %d case %d" % (mode, k)
            if c["out"] is None:
                assert len(runs[j]) == 0, what
                continue
            text = fs.format_cigar(runs[j])
            ln, op = runs[j] >> 4, runs[j] & 15
            assert (ln > 0).all() and (op <= 2).all() and (op[1:] != op[:-1]).all() and ln.sum() == got["aln"][j], what
            if b"-" in c["qw"] or b"-" in c["sw"]:
                q, s = c["seqs"][c["q"]], c["seqs"][c["s"]]
                assert fs.cigar_to_strings(runs[j], q, s, int(got["qst"][j]) + 1, int(got["sst"][j]) + 1) == c["strings"], (what, text, c["cigar"])
            else:
                assert text == c["cigar"], what
        assert len(take) > 0.9 * len(tasks)
    with pytest.raises(Exception, match="traced kernels"):
        st.s.align_pairs([tasks[0]], 0, cigar=True)
    st.close()


# ---- 3. the oracle, every row -------------------------------------------------------------------------------------------------------

def against_the_oracle(fs, oracle, ref, qry, kw, tmp_path, what):
    rows, recs, runs, text, _, qm = search_cigar(fs, ref, qry, kw, masked=True)
    want_rows, want_alns = oracle_strings(oracle, ref, qry, kw, tmp_path)
    assert rows == want_rows, what
    check_against_strings(fs, recs, runs, text, qm, sequences(ref), want_alns, what)
    return np.frombuffer(recs, dtype=DT), runs


def test_cigars_rebuild_the_oracle_strings_synthetic(fs, oracle, tmp_path):
    from swiftortho_amd import synthprot
    fa = synthprot.synthprot(2000, 250, 7)
    kw = dict(ssd="111111", nr=AA9, ht=120000000, chk=50000, step=1, v=500, expect=1e-5, flt="T")
    against_the_oracle(fs, oracle, fa, fa, kw, tmp_path, "synthetic")


@pytest.fixture(scope="module")
def het_cigar(fs, het_default):
    fa, _ = het_default
    return search_cigar(fs, fa, fa, HET_KW, masked=True)


def test_cigars_rebuild_the_oracle_strings_het(fs, het_default, het_oracle, het_cigar):
    """log-normal lengths with the 30 000-residue giant"""
    fa, _ = het_default
    rows, recs, runs, text, _, qm = het_cigar
    assert rows == het_oracle[0]
    check_against_strings(fs, recs, runs, text, qm, sequences(fa), het_oracle[1], "het")
    assert max(len(s) for s in sequences(fa)) >= 30000


def test_cigars_rebuild_the_oracle_strings_long_tiles(fs, oracle, tmp_path):
    fa = long_fasta()
    kw = dict(ssd="111111", nr=AA9, ht=1000003, chk=50000, step=1, v=500, expect=1e-5, flt="T")
    r, runs = against_the_oracle(fs, oracle, fa, fa, kw, tmp_path, "long")
    assert ((r["qlen"] > 4096) & (r["slen"] > 4096)).sum() >= 10   # tile rows, each with its own tile's CIGAR
    assert max(int((x >> 4).sum()) for x in runs) >= 4096


@pytest.mark.parametrize("flt", ["F", "T"])
def test_cigars_rebuild_the_oracle_strings_tandem_repeats(fs, oracle, tmp_path, flt):
    fa = tandem_fasta()
    kw = dict(ssd="111111,1101011", nr=AA9, ht=1000003, chk=20, step=1, v=500, expect=1e-3, flt=flt)
    _, runs = against_the_oracle(fs, oracle, fa, fa, kw, tmp_path, "tandem " + flt)
    assert any(len(x) > 1 for x in runs)


def test_cigars_rebuild_the_oracle_strings_odd_bytes(fs, oracle, tmp_path):
    ref, qry = odd_byte_sets()
    kw = dict(ssd="111111", nr=AA9, ht=1000003, chk=50000, step=1, v=500, expect=1e-3, flt="T")
    against_the_oracle(fs, oracle, ref, qry, kw, tmp_path, "odd bytes")


def test_cigars_rebuild_the_oracle_strings_query_longer(fs, oracle, tmp_path):
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
    r, _ = against_the_oracle(fs, oracle, ref, qry, kw, tmp_path, "query longer")
    assert (r["qlen"] > r["slen"]).sum() >= 50


# ---- 4. the same answer as the strings ----------------------------------------------------------------------------------------------

def test_cigars_say_what_the_strings_say(fs, het_default, het_cigar):
    fa, (rows1, recs1, alns1, _) = het_default
    rows, recs, runs, text, _, qm = het_cigar
    assert recs == recs1 and rows == rows1
    check_against_strings(fs, recs, runs, text, qm, sequences(fa), alns1, "strings of the same search")


# ---- 5. asking changes nothing; ranges, the halves rerun, the path switches ---------------------------------------------------------

def test_asking_for_cigars_changes_no_row(fs, het_default, het_cigar):
    from test_gpu_aln import search
    fa, _ = het_default
    rows0, recs0, none, c0 = search(fs, fa, fa, HET_KW, alignments=False)
    rows, recs, _, _, c1, _ = het_cigar
    assert none is None and recs0 == recs and rows0 == rows
    for k in ("rows", "seed_hits", "candidates", "alignments", "n_queries", "cells"):
        assert c0[k] == c1[k], k
    s = fs.Searcher(**HET_KW)
    try:
        s.load_ref_bytes(fa), s.load_queries_bytes(fa)
        with pytest.raises(ValueError):
            s.search(alignments=True, cigar=True)
        h = s.search(0, 50)   # a plain search carries none
        with pytest.raises(fs.SohitError):
            h.cigar(0)
        h.close()
    finally:
        s.close()


def test_sub_range_cigars_equal_the_full_run(fs, het_default, het_cigar):
    fa, _ = het_default
    _, recs, runs, text, _, _ = het_cigar
    qidx = np.frombuffer(recs, dtype=DT)["qidx"]
    lo, hi = 700, 1900
    _, recs2, runs2, text2, _, _ = search_cigar(fs, fa, fa, HET_KW, ranges=[(lo, hi)])
    sel = np.nonzero((qidx >= lo) & (qidx < hi))[0]
    assert recs2 == np.frombuffer(recs, dtype=np.uint8).reshape(-1, 80)[sel].tobytes()
    assert text2 == [text[k] for k in sel]
    # two ranges in one context, appended
    _, recs3, _, text3, _, _ = search_cigar(fs, fa, fa, HET_KW, ranges=[(0, 1000), (1000, -1)])
    assert recs3 == recs and text3 == text


def test_halves_rerun_keeps_the_cigars(fs):
    code = r'''
import os, sys
sys.path.insert(0, %r)
from swiftortho_amd import fsearch, synthprot
fa = synthprot.synthprot(900, seed=3, lengths="lognormal")
kw = dict(ssd="111111", nr="AST,CFILMVY,DN,EQ,G,H,KR,P,W", ht=120000000, chk=400, step=1, v=500, expect=1e-5, flt="T")
def run():
    s = fsearch.Searcher(**kw)
    s.load_ref_bytes(fa); s.load_queries_bytes(fa)
    h = s.search(cigar=True)
    raw, cg, cnt = h.raw_bytes(), [h.cigar(k) for k in range(len(h))], s.counters()
    h.close(); s.close()
    return raw, cg, cnt
want = run()
os.environ["SOHIT_TEST_OOM_PHASE2"] = "1"
got = run()
assert got[0] == want[0] and len(want[1]) > 500, (len(got[0]), len(want[0]))
assert got[1] == want[1]
assert all(got[2][k] == want[2][k] for k in ("rows", "n_queries", "candidates")), (got[2], want[2])
print("OOM_CIGAR_OK")
''' % ROOT
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "OOM_CIGAR_OK" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])


@pytest.mark.parametrize("env", [{"SOHIT_ALIGN_PK": "0"}, {"SOHIT_SPEC": "1"}, {"SOHIT_SPEC": "0"}, {"SOHIT_TRACE_WAVE_ROWS": "0"},
                                 {"SOHIT_TRACE_WAVE_ROWS": "16", "SOHIT_TRACE_WAVE_MAX": "100000000"}, {"SOHIT_EMIT_PARTS": "1"},
                                 {"SOHIT_BATCH": "700"}, {"SOHIT_POISON": "0xFF"}],
                         ids=["no_packed", "kept_traces", "no_kept_traces", "every_walk_by_a_thread", "every_walk_by_a_wave", "one_range",
                              "small_batches", "poison"])
def test_path_switches_give_the_same_cigars(fs, het_default, het_cigar, monkeypatch, env):
    fa, _ = het_default
    _, recs0, _, text0, _, _ = het_cigar
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _, recs, _, text, _, _ = search_cigar(fs, fa, fa, HET_KW)
    assert recs == recs0
    assert text == text0


# ---- 6. the command line ------------------------------------------------------------------------------------------------------------

def _cli(args, **kw):
    return subprocess.run([sys.executable] + args, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, **kw)


def test_find_hit_cli_writes_the_cigar_column(tmp_path):
    name = "toy_default"
    meta = json.load(open(os.path.join(GOLD, name + ".json")))
    gold = json.load(open(os.path.join(GOLD, "aln_%s.json" % name)))
    ref = os.path.join(GOLD, name + ".ref.fsa")
    want = open(os.path.join(GOLD, name + ".sc"), "rb").read()
    base = [os.path.join("bin", "find_hit.py"), "-p", "blastp", "-i", ref, "-d", ref, "-a", "1"] + list(meta["flags"])
    out = tmp_path / "c.sc"
    p = _cli(base + ["-o", str(out), "-C", "T"])
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-2000:])
    lines = out.read_bytes().split(b"\n")
    assert lines[-1] == b"" and all(l.count(b"\t") == 16 for l in lines[:-1])
    assert b"".join(l.rsplit(b"\t", 1)[0] + b"\n" for l in lines[:-1]) == want
    cig = dict((k, c) for k, c in gold["rows"])
    assert len(cig) == len(lines) - 1 > 100
    assert [l.rsplit(b"\t", 1)[1].decode() for l in lines[:-1]] == [cig[k] for k in range(len(lines) - 1)]
    for extra in ([], ["-C", "F"]):
        plain = tmp_path / "p.sc"
        p = _cli(base + ["-o", str(plain)] + extra)
        assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-2000:])
        assert plain.read_bytes() == want


def test_two_rank_cli_writes_the_one_rank_cigar_file(tmp_path):
    """find_hit.py -a 2 -C T (two ranks over gloo, both on GPU 0; every rank writes its own 17-column part) = -a 1 -C T"""
    from swiftortho_amd import synthprot
    from test_gpu_parity import ONE_GPU_GLOO
    fa = tmp_path / "w.fsa"
    fa.write_bytes(synthprot.synthprot(3000, 300, 77))
    outs = []
    for a in (1, 2):
        out = tmp_path / ("a%d.sc" % a)
        p = _cli([os.path.join("bin", "find_hit.py"), "-p", "blastp", "-i", str(fa), "-d", str(fa), "-o", str(out), "-e", "1e-5", "-s", "111111",
                  "-a", str(a), "-C", "T"], env=dict(os.environ, **ONE_GPU_GLOO))
        assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
        outs.append(out.read_bytes())
    assert outs[0].count(b"\n") > 5000 and all(l.count(b"\t") == 16 for l in outs[0].split(b"\n")[:-1])
    assert outs[0] == outs[1]
