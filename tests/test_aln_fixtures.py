"""CPU test: the alignment fixtures (aln_<name>.json, the REAL reference's kswat_st strings per golden row, kept as CIGARs that
rebuild them) and the product's string rules (fsearch.aln_stats, fsearch.py:1454-1471) check each other: every row's two strings
reproduce the aln, mis, gap and identity columns of the golden .sc row they belong to."""
import json
import os

import pytest

from conftest import GOLD

from swiftortho_amd.fsearch import aln_stats

NAMES = sorted(f[4:-5] for f in os.listdir(GOLD) if f.startswith("aln_") and f.endswith(".json"))


def records(data):
    out = {}
    for rec in data.split(b"\n>"):
        rec = rec[1:] if rec.startswith(b">") else rec
        if rec.strip():
            lines = rec.split(b"\n")
            out.setdefault(lines[0].split(b" ")[0], []).append(b"".join(lines[1:]))
    return out


def aln_strings(cigar, q, s, qst, sst):
    """(query string, subject string) from a CIGAR (M both advance, I query alone, D subject alone) and the row's 1-based starts"""
    a0, a1, qp, sp, n = [], [], qst - 1, sst - 1, 0
    for ch in cigar:
        if ch.isdigit():
            n = 10 * n + int(ch)
            continue
        for _ in range(n):
            a0.append(q[qp:qp + 1] if ch != "D" else b"-")
            a1.append(s[sp:sp + 1] if ch != "I" else b"-")
            qp += ch != "D"
            sp += ch != "I"
        n = 0
    return b"".join(a0), b"".join(a1)


def fixture(name, oracle):
    """-> (golden .sc rows, fixture dict, {row index: (query string, subject string)}); the query as the aligner saw it (SEG under -F T)"""
    gold = json.load(open(os.path.join(GOLD, "aln_%s.json" % name)))
    meta = json.load(open(os.path.join(GOLD, name + ".json")))
    ref = open(os.path.join(GOLD, name + ".ref.fsa"), "rb").read()
    qry = open(os.path.join(GOLD, name + ".qry.fsa"), "rb").read() if meta.get("separate_query") else ref
    seg = dict(zip(meta["flags"][0::2], meta["flags"][1::2])).get("-F", "T") == "T"
    qs, ss = records(qry), records(ref)
    rows = [r for r in open(os.path.join(GOLD, name + ".sc"), "rb").read().split(b"\n") if r]
    strings = {}
    for k, cig in gold["rows"]:
        c = rows[k].split(b"\t")
        q = qs[c[0]][0]
        strings[k] = aln_strings(cig, oracle.seg(q) if seg else q, ss[c[1]][0], int(c[6]), int(c[8]))
    return rows, gold, strings


def test_fixtures_cover_the_goldens():
    assert set(NAMES) >= {"toy_default", "toy_w10", "toy_messy", "toy_oddchars", "toy_ragged", "toy_chunks", "toy_long_subject",
                          "toy_long_both", "het_w6", "het_w10"}


@pytest.mark.parametrize("name", NAMES)
def test_fixture_strings_reproduce_the_golden_rows(oracle, name):
    rows, gold, strings = fixture(name, oracle)
    assert len(gold["rows"]) + gold["left_out"] + gold["unmatched"] == len(rows)
    assert len(gold["rows"]) >= 0.95 * len(rows)
    for k, (a0, a1) in strings.items():
        c = rows[k].split(b"\t")
        assert len(a0) == len(a1) == int(c[3]), (name, k)
        assert a0.replace(b"-", b"") or a1.replace(b"-", b""), (name, k)
        matches, mis, gap, idy = aln_stats(a0, a1)
        if any(x == y == 45 for x, y in zip(a0, a1)):
            # a literal '-' residue opposite a gap: the reference ran the machine in its own order, which is the swapped one when
            # the subject was on its columns -- the two orders differ only in such columns
            gap = (gap, aln_stats(a1, a0)[2])[aln_stats(a1, a0)[2] == int(c[5])]
        assert (mis, gap) == (int(c[4]), int(c[5])), (name, k)
        assert -1e-9 <= idy - float(c[2]) < 0.01 + 1e-9, (name, k)   # (the row prints it cut to two decimals)


def test_aln_stats_rules():
    # a literal '-' residue counts like a gap character; a run of L gap columns opens ceil(L / 2) times
    assert aln_stats(b"AC--D", b"ACGTD") == (3, 2, 1, 60.0)
    assert aln_stats(b"A---", b"AGGG")[2] == 2
    assert aln_stats(b"A-C", b"A-C") == (3, 0, 1, 100.0)
    with pytest.raises(ValueError):
        aln_stats(b"A", b"AC")


def oracle_kwargs(flags):
    """oracle.blastp's arguments for a golden's fsearch-c flags"""
    d = dict(zip(flags[0::2], flags[1::2]))
    return dict(ssd=d.get("-s", "111111"), nr=d.get("-r", "AST,CFILMVY,DN,EQ,G,H,KR,P,W"), expect=float(d.get("-e", 1e-3)), v=int(d.get("-v", 500)),
                max_miss=float(d.get("-m", 1e-3)), thr=int(d.get("-t", -1)), step=int(d.get("-j", 4)), flt=d.get("-F", "T"), ht=int(d.get("-M", -1)),
                chk=int(d.get("-c", 50000)))


def oracle_run(oracle, name, tmp_path):
    """-> (the oracle's .sc text, its rows' (query string, subject string)) for golden `name`, with the golden's flags and query ranges"""
    meta = json.load(open(os.path.join(GOLD, name + ".json")))
    ref = os.path.join(GOLD, name + ".ref.fsa")
    qry = os.path.join(GOLD, name + ".qry.fsa") if meta.get("separate_query") else ref
    text, alns = b"", []
    for k, rng in enumerate(meta.get("ranges") or [(-1, -1)]):
        out = str(tmp_path / ("o%d.sc" % k))
        r = oracle.blastp(qry, ref, out, st=rng[0], ed=rng[1], alignments=True, **oracle_kwargs(meta["flags"]))
        text += open(out, "rb").read()
        assert r.alignments is not None and len(r.alignments) == len(r.ints)
        alns += r.alignments
    return text, alns


def check_row_strings(row, a0, a1):
    """one .sc row's aln, mis, gap and identity columns from its strings (aln_stats, with the reference's literal-'-' rule)"""
    c = row.split(b"\t")
    assert len(a0) == len(a1) == int(c[3])
    matches, mis, gap, idy = aln_stats(a0, a1)
    if any(x == y == 45 for x, y in zip(a0, a1)):
        gap = (gap, aln_stats(a1, a0)[2])[aln_stats(a1, a0)[2] == int(c[5])]
    assert (mis, gap) == (int(c[4]), int(c[5]))
    assert -1e-9 <= idy - float(c[2]) < 0.01 + 1e-9


@pytest.mark.parametrize("name", NAMES)
def test_oracle_strings_equal_the_real_reference(oracle, name, tmp_path):
    """the oracle's rows are the golden's, and its strings are the REAL reference's for every fixture row"""
    rows, gold, want = fixture(name, oracle)
    text, alns = oracle_run(oracle, name, tmp_path)
    assert text == open(os.path.join(GOLD, name + ".sc"), "rb").read()
    assert len(alns) == len(rows) and len(want) > 0
    for k, w in want.items():
        assert alns[k] == w, (name, k)
    # every oracle row (the fixture's left-out and unmatched ones too) agrees with its own columns
    for k, (a0, a1) in enumerate(alns):
        check_row_strings(rows[k], a0, a1)


def aln_edge_cases():
    """tests/golden/kswat_aln_edges.json (make_goldens.py, the REAL reference's kswat_st strings at the edges): per case the query and
    subject windows (bytes), the starts, the reference's tuple (None: no answer) and its strings (b"" both when there is none)"""
    e = json.load(open(os.path.join(GOLD, "kswat_aln_edges.json")))
    seqs = [x.encode("latin-1") for x in e["seqs"]]
    out = []
    for c in e["cases"]:
        c = dict(zip(e["fields"], c))
        q, s = seqs[c["q"]][c["qlo"]:c["qhi"]], seqs[c["s"]][c["slo"]:c["shi"]]
        r = c["out"]
        strings = aln_strings(c["cigar"], q, s, r[4] + 1, r[6] + 1) if r is not None else (b"", b"")
        out.append(dict(c, qw=q, sw=s, strings=strings, seqs=seqs))
    return out


def test_oracle_strings_at_the_edges(oracle):
    """every case of kswat_aln_edges.json: the oracle's tuple and strings are the real reference's"""
    cases = aln_edge_cases()
    assert len(cases) >= 200
    lens = {(len(c["qw"]) - min(c["qst"], len(c["qw"]))) - (len(c["sw"]) - min(c["sst"], len(c["sw"]))) for c in cases}
    assert {-1, 0, 1} <= lens   # query shorter, equal (the swap branch), longer
    assert {4096} <= {len(c["qw"]) for c in cases} and any(c["out"] is None for c in cases)
    assert any(b"-" in c["qw"] and b"-" in c["strings"][0] + c["strings"][1] for c in cases)
    for c in cases:
        r, (a0, a1) = oracle.kswat_st(c["qw"], c["sw"], c["qst"], c["sst"], strings=True)
        if c["out"] is None:
            assert r[1] == 0 and (a0, a1) == (b"", b""), c["cigar"]
            continue
        assert r[0] == c["out"][0] and list(r[1:]) == c["out"][1:], (c["qw"][:40], c["sw"][:40], r, c["out"])
        assert (a0, a1) == c["strings"], (c["qw"][:40], c["sw"][:40], c["cigar"])
        # and the tuple's statistics follow from the strings (in the reference's own order when a literal '-' faces a gap)
        _, mis, gap, idy = aln_stats(a0, a1)
        if gap != r[3]:
            gap = aln_stats(a1, a0)[2]
        assert (len(a0), mis, gap) == (r[1], r[2], r[3]) and abs(idy - r[0]) < 1e-9
