"""Aligned strings of every golden row from the REAL reference (container only).

    python tools/refharness/make_aln_goldens.py [--force] [name ...]

kswat_st fills two lists with the query-side and subject-side aligned strings of every alignment it makes (fsearch.py:1417-1444,
'-' in gap columns; it swaps the lists when it swaps the sequences, so al0 is always the query side) and derives the row's
statistics from them (1454-1471); entry_point passes fresh lists per call (3066-3070) and throws them away.  This script wraps
the module's kswat_st and kswat_st_long so that every call's strings are recorded, runs entry_point with each golden's own
flags (and query ranges, for the het_* goldens), and pairs each row of the golden's .sc with the call that produced it: same
query sequence (as the aligner saw it: SEG-masked under -F T), same subject, same coordinates and statistics.  A row that two
matching calls would explain with different strings is left out, and counted.

Writes only data: tests/golden/aln_<name>.json = {"name", "rows": [[row index in the .sc, CIGAR], ...], "left_out", "unmatched"}.
The CIGAR holds the columns of the pair of strings in order, run-length coded: M both sides advance, I the query alone ('-' in the
subject string), D the subject alone ('-' in the query string).  With the row's qst / sst, the query as the aligner saw it and the
subject it rebuilds both strings byte for byte (aln_strings); a row whose strings it would not rebuild exactly is left out too.
"""
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import refload  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
FORCE = "--force" in sys.argv
NAMES = ["toy_default", "toy_w10", "toy_messy", "toy_oddchars", "toy_ragged", "toy_chunks", "toy_long_subject", "toy_long_both",
         "het_w6", "het_w10"]


def _b(x):
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    if isinstance(x, str):
        return x.encode("latin-1")
    return b"".join(_b(c) for c in x)


def fasta_records(data):
    """(header's first word, residues) per record, as the reference splits them (header line, then sequence lines joined)"""
    out = []
    for rec in data.split(b"\n>"):
        rec = rec[1:] if rec.startswith(b">") else rec
        if not rec.strip():
            continue
        lines = rec.split(b"\n")
        out.append((lines[0].split(b" ")[0], b"".join(lines[1:])))
    return out


def aln_strings(cigar, q, s, qst, sst):
    """(query string, subject string) from a CIGAR, the query as the aligner saw it, the subject and the row's 1-based starts"""
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


def to_cigar(a0, a1, q, s, qst, qed, sst, sed):
    """the columns of two aligned strings as M / I / D runs, or None.  A '-' in a string is a gap column or a literal '-' residue:
    the columns are matched against the sequences, every reading that fits kept (they are few), and a path that ends at
    (qed, sed) taken"""
    states = {(qst - 1, sst - 1): None}   # (query position, subject position) -> (previous state, op)
    back = []
    for x, y in zip(a0, a1):
        nxt = {}
        for qp, sp in states:
            qc, sc = q[qp:qp + 1], s[sp:sp + 1]
            for op, ok, st in (("M", qc == bytes([x]) and sc == bytes([y]), (qp + 1, sp + 1)),
                               ("I", qc == bytes([x]) and y == 45, (qp + 1, sp)), ("D", x == 45 and sc == bytes([y]), (qp, sp + 1))):
                if ok and st not in nxt:
                    nxt[st] = ((qp, sp), op)
        if not nxt:
            return None
        back.append(nxt)
        states = nxt
    st = (qed, sed)
    if st not in states:
        return None
    ops = []
    for nxt in reversed(back):
        st, op = nxt[st]
        if ops and ops[-1][0] == op:
            ops[-1][1] += 1
        else:
            ops.append([op, 1])
    return "".join("%d%s" % (n, op) for op, n in reversed(ops))


class Recorder:
    """wraps m.kswat_st / m.kswat_st_long: calls[key] = set of (al0, al1)"""

    def __init__(self, m):
        self.m = m
        self.calls = {}
        self.orig_st, self.orig_long = m.kswat_st, m.kswat_st_long
        rec = self

        def kswat_st(S0, S1, *a, **kw):
            r = rec.orig_st(S0, S1, *a, **kw)
            al0, al1 = kw.get("al0"), kw.get("al1")
            if al0 is not None and al1 is not None:
                idy, aln, mis, gap, qst, qed, sst, sed, bit = r
                rec.add(S0, S1, (qst + 1, qed, sst + 1, sed, aln, mis, gap), al0, al1)
            return r

        def kswat_st_long(sqi, sqj, qi, qj, *a, **kw):
            al0, al1 = kw.get("al0"), kw.get("al1")
            for r in rec.orig_long(sqi, sqj, qi, qj, *a, **kw):
                idy, aln, mis, gap, qst, qed, sst, sed, bit = r
                rec.add(sqi, sqj, (qst + 1, qed, sst + 1, sed, aln, mis, gap), al0, al1)   # (the tile's lists, emptied after the yield)
                yield r

        m.kswat_st, m.kswat_st_long = kswat_st, kswat_st_long

    def add(self, S0, S1, stats, al0, al1):
        key = (_b(S0), _b(S1)) + tuple(int(x) for x in stats)
        self.calls.setdefault(key, set()).add((_b(al0), _b(al1)))

    def restore(self):
        self.m.kswat_st, self.m.kswat_st_long = self.orig_st, self.orig_long


def make(m, name):
    dst = os.path.join(GOLD, "aln_%s.json" % name)
    if os.path.isfile(dst) and not FORCE:
        print(name, "exists, skipped")
        return
    meta = json.load(open(os.path.join(GOLD, name + ".json")))
    ref = open(os.path.join(GOLD, name + ".ref.fsa"), "rb").read()
    qry = open(os.path.join(GOLD, name + ".qry.fsa"), "rb").read() if meta.get("separate_query") else ref
    flags = meta["flags"]
    seg_on = dict(zip(flags[0::2], flags[1::2])).get("-F", "T") == "T"
    tmp = tempfile.mkdtemp(prefix="gold_aln_")
    fa, qa = os.path.join(tmp, "ref.fsa"), os.path.join(tmp, "qry.fsa")
    open(fa, "wb").write(ref)
    open(qa, "wb").write(qry)
    rec = Recorder(m)
    t0 = time.time()
    try:
        for r in meta.get("ranges") or [None]:
            out = os.path.join(tmp, "out.sc")
            rng = ["-l", str(r[0]), "-u", str(r[1])] if r else []
            m.entry_point(["fsearch", "-p", "blastp", "-i", qa, "-d", fa, "-o", out, "-T", tmp] + rng + flags)
    finally:
        rec.restore()
    want = open(os.path.join(GOLD, name + ".sc"), "rb").read().split(b"\n")
    want = [r for r in want if r]
    qseqs, sseqs = {}, {}
    for nm, sq in fasta_records(qry):
        qseqs.setdefault(nm, []).append(sq)
    for nm, sq in fasta_records(ref):
        sseqs.setdefault(nm, []).append(sq)

    def masked(sq):   # the query as kswat_st sees it (fsearch.py:2963)
        if not seg_on:
            return sq
        try:
            r, _ = m.seg(sq.decode("latin-1"))
        except TypeError:
            r, _ = m.seg(sq)
        return _b(r)

    rows, left_out, unmatched = [], 0, 0
    for k, line in enumerate(want):
        c = line.split(b"\t")
        stats = tuple(int(c[i]) for i in (6, 7, 8, 9, 3, 4, 5))
        found = set()
        for q in qseqs.get(c[0], []):
            for s in sseqs.get(c[1], []):
                found |= rec.calls.get((masked(q), s) + stats, set())
        if not found:
            unmatched += 1
        elif len(found) > 1:
            left_out += 1
        else:
            a0, a1 = next(iter(found))
            q = masked(qseqs[c[0]][0]) if len(qseqs[c[0]]) == 1 else None
            sq = sseqs[c[1]][0] if len(sseqs[c[1]]) == 1 else None
            cig = to_cigar(a0, a1, q, sq, int(c[6]), int(c[7]), int(c[8]), int(c[9])) if q is not None and sq is not None else None
            if cig is None or aln_strings(cig, q, sq, int(c[6]), int(c[8])) != (a0, a1):
                left_out += 1
            else:
                rows.append([k, cig])
    with open(dst, "w") as f:
        json.dump({"name": name, "left_out": left_out, "unmatched": unmatched, "rows": rows}, f, separators=(",", ":"))
        f.write("\n")
    print(name, "rows", len(want), "kept", len(rows), "left out", left_out, "unmatched", unmatched, "%.0fs" % (time.time() - t0),
          "%d bytes" % os.path.getsize(dst), flush=True)


def main():
    m = refload.load()
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or NAMES
    for name in names:
        make(m, name)


if __name__ == "__main__":
    main()
