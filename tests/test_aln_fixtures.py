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
