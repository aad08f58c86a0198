"""Generate tests/golden/ fixtures by running the REAL reference source (container only).

    python tools/refharness/make_goldens.py

Writes only data: inputs (FASTA), expected outputs (.sc rows, stage values) and the
flags used.  No reference source text is stored.  Re-running must reproduce the
committed files byte for byte (the reference path is deterministic).
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import refload  # noqa: E402
from swiftortho_amd import synthprot  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
AA9 = "AST,CFILMVY,DN,EQ,G,H,KR,P,W"
AA20 = "A,S,T,C,F,I,L,M,V,Y,D,N,E,Q,G,H,K,R,P,W"
AA10B = "A,KR,EDNQ,C,G,H,ILVM,FYW,P,ST"


def messy_fasta(rng):
    """Hand-shaped inputs: low-complexity runs, X/B/Z/U letters, lower case, multi-line
    records, descriptions with spaces, a short record, an offset-0 seed situation."""
    base = synthprot.synthprot(24, 90, 99).decode().split("\n")
    recs = [(base[i][1:], base[i + 1]) for i in range(0, len(base) - 1, 2)]
    out = []
    for k, (hd, sq) in enumerate(recs):
        if k % 4 == 0:
            sq = sq[:30] + "SSSSSSSSSSSSSSGAAAAAAPAPAPAPAPAPQQQQQQQQQQQ" + sq[30:]
        if k % 5 == 1:
            sq = sq[:20] + "XXBZU" + sq[25:]
        if k % 7 == 2:
            sq = sq[:40] + sq[40:60].lower() + sq[60:]
        if k % 6 == 3:
            sq = "\n".join(sq[i:i + 25] for i in range(0, len(sq), 25))
        out.append(">%s some description %d\n%s\n" % (hd, k, sq))
    # (a record shorter than the shortest seed crashes the reference: fsearch.py:2649-2651 indexes past the string)
    out.append(">dup|p2\n%s\n" % recs[0][1])
    return "".join(out).encode()


def oddchar_fasta():
    """Residues outside the alphabet inside homologous regions: literal '-' (the reference's statistics read aligned
    STRINGS, so a '-' residue counts like a gap character, fsearch.py:1454-1471), '*', '.', U / J / O / B / Z, x / X and lower
    case -- a few per record, so that the alignments run across them."""
    rng = np.random.default_rng(77)
    base = synthprot.synthprot(60, 120, 5).decode().strip().split("\n")
    odd = "-*.UJOBZxXak-"
    out = []
    for i in range(0, len(base), 2):
        sq = list(base[i + 1])
        if (i // 2) % 3 != 2:
            for p in rng.integers(8, len(sq) - 8, size=int(rng.integers(1, 5))):
                sq[int(p)] = odd[int(rng.integers(0, len(odd)))]
        out.append(base[i] + "\n" + "".join(sq) + "\n")
    return "".join(out).encode()


def fasta_quirks():
    """Record parsing (fsearch.py:1543-1553, 2182-2205): '>' inside a line, blank lines, blanks inside sequence lines, tabs in
    a header, duplicate ids, a 300-character id.  Returns (reference, queries)."""
    base = synthprot.synthprot(60, 120, 5)
    recs, cur = {}, None
    for l in base.decode().strip().split("\n"):
        if l.startswith(">"):
            cur = l
            recs[cur] = ""
        else:
            recs[cur] += l
    names = list(recs)
    s0, s1, s2 = recs[names[0]], recs[names[1]], recs[names[2]]
    rag = b"".join([
        b">gt_inside\n" + (s0[:40] + ">" + s0[40:]).encode() + b"\n",
        b">blank_lines\n" + s1[:30].encode() + b"\n\n" + s1[30:].encode() + b"\n\n",
        b">spaces in\theader\twith tabs\n" + (s2[:20] + "  " + s2[20:70] + " " + s2[70:]).encode() + b"\n",
        b">dup\n" + s0.encode() + b"\n", b">dup\n" + s0.encode() + b"\n",
        b">" + b"L" * 300 + b" longheader\n" + s1.encode() + b"\n",
    ])
    return base + rag, rag


def ragged_queries():
    """Query records the reference still defines: wrapped lines + description, all-X, lower case, CRLF line ends (the '\\r'
    stays in the id and in the residues), bytes outside the alphabet, last record without a newline.  (Records shorter
    than the seed or empty crash the reference and are our own definition: tests/test_gpu_parity.py.)"""
    base = synthprot.synthprot(60, 120, 5)
    recs, cur = {}, None
    for l in base.decode().strip().split("\n"):
        if l.startswith(">"):
            cur = l
            recs[cur] = ""
        else:
            recs[cur] += l
    names = list(recs)
    s0, s1 = recs[names[0]], recs[names[1]]
    qry = b"".join([
        (names[0] + " some description here\n").encode(), (s0[:50] + "\n" + s0[50:] + "\n").encode(),
        b">allx\n" + b"X" * 40 + b"\n",
        b">lower\n" + s1.lower().encode() + b"\n",
        b">crlf\r\n" + s1[:60].encode() + b"\r\n" + s1[60:].encode() + b"\r\n",
        b">weird\n" + (s0[:30] + "*U-J" + s0[30:]).encode() + b"\n",
        b">last_no_newline\n" + s0.encode(),
    ])
    return base, qry


FORCE = "--force" in sys.argv


def long_sets():
    """Sequences >= 4096 aa (kswat_st_long tiles, fsearch.py:1480-1498, 3083-3101).

    The reference is only defined when every tile of a candidate still starts inside the subject:
    a long query whose later tiles run past a shorter subject indexes an empty string
    (IndexError under CPython, out-of-bounds read in the RPython build).  So:
      set A: queries < 4096 aa against long subjects (one 4096-wide tile per candidate);
      set B: long queries against equally long subjects only (three tiles each, all in range)."""
    rng = np.random.default_rng(44)
    aa = "ACDEFGHIKLMNPQRSTVWY"

    def rnd(n):
        return "".join(aa[i] for i in rng.integers(0, 20, n))

    def mut(s, d, indels=True):
        s = list(s)
        for p in range(len(s)):
            if rng.random() < d:
                s[p] = aa[int(rng.integers(0, 20))]
        if indels:
            for _ in range(max(1, len(s) // 400)):
                p = int(rng.integers(10, len(s) - 10))
                if rng.random() < 0.5:
                    del s[p:p + int(rng.integers(1, 6))]
                else:
                    s[p:p] = list(rnd(int(rng.integers(1, 6))))
        return "".join(s)

    A = rnd(9000)
    L3 = rnd(4100)
    base = synthprot.synthprot(12, 250, 45).decode().split("\n")
    normal = [(base[i][1:], base[i + 1]) for i in range(0, len(base) - 1, 2)]
    refA = [("L0|giant", A), ("L1|first6000", mut(A[:6000], 0.15)), ("L2|mid4600", mut(A[2000:6600], 0.25)), ("L3|other4100", L3)] + normal
    qryA = [("S0|frag_a", mut(A[100:420], 0.1)), ("S1|frag_b", mut(A[5000:5350], 0.2)), ("S2|frag_c", mut(A[8600:8990], 0.1)),
            ("S3|frag_of_L3", mut(L3[3700:4090], 0.1)), ("S4|frag_d", mut(A[4000:4300], 0.05))] + normal[:4]
    refB = [("L0|giant", A), ("L0m|giant_mut", mut(A, 0.2)), ("L0n|giant_mut2", mut(A, 0.35))]
    qryB = [("L0|giant", A), ("L0q|giant_mut3", mut(A, 0.1))]
    f = lambda recs: "".join(">%s\n%s\n" % r for r in recs).encode()
    return f(refA), f(qryA), f(refB), f(qryB)


def run_e2e(m, name, fasta, flags, qry=None):
    if os.path.isfile(os.path.join(GOLD, name + ".sc")) and not FORCE:
        print(name, "exists, skipped")
        return
    tmp = tempfile.mkdtemp(prefix="gold_")
    fa = os.path.join(tmp, "ref.fsa")
    open(fa, "wb").write(fasta)
    qa = fa
    if qry is not None:
        qa = os.path.join(tmp, "qry.fsa")
        open(qa, "wb").write(qry)
    out = os.path.join(tmp, "out.sc")
    m.entry_point(["fsearch", "-p", "blastp", "-i", qa, "-d", fa, "-o", out, "-T", tmp] + flags)
    open(os.path.join(GOLD, name + ".ref.fsa"), "wb").write(fasta)
    if qry is not None:
        open(os.path.join(GOLD, name + ".qry.fsa"), "wb").write(qry)
    open(os.path.join(GOLD, name + ".sc"), "wb").write(open(out, "rb").read())
    json.dump({"flags": flags, "separate_query": qry is not None}, open(os.path.join(GOLD, name + ".json"), "w"), indent=1)
    print(name, "rows:", open(out, "rb").read().count(b"\n"))


def run_find_hit(name, ref, qry, flags, max_chr=None):
    """End-to-end through the REAL launcher bin/find_hit.py (query blocks, cat; with max_chr the reference split + merge)."""
    import ref_find_hit
    if os.path.isfile(os.path.join(GOLD, name + ".sc")) and not FORCE:
        print(name, "exists, skipped")
        return
    tmp = tempfile.mkdtemp(prefix="gold_")
    fa, qa, out = os.path.join(tmp, "ref.fsa"), os.path.join(tmp, "qry.fsa"), os.path.join(tmp, "out.sc")
    open(fa, "wb").write(ref)
    open(qa, "wb").write(qry)
    ref_find_hit.run(["-p", "blastp", "-i", qa, "-d", fa, "-o", out, "-T", os.path.join(tmp, "t")] + flags, max_chr=max_chr)
    open(os.path.join(GOLD, name + ".ref.fsa"), "wb").write(ref)
    open(os.path.join(GOLD, name + ".qry.fsa"), "wb").write(qry)
    open(os.path.join(GOLD, name + ".sc"), "wb").write(open(out, "rb").read())
    json.dump({"find_hit_flags": flags, "max_chr": max_chr, "separate_query": True}, open(os.path.join(GOLD, name + ".json"), "w"), indent=1)
    print(name, "rows:", open(out, "rb").read().count(b"\n"))


def first_records(fasta, n):
    recs = fasta.split(b">")[1:]
    return b"".join(b">" + r for r in recs[:n])


def stage_dump(m, name, fasta, ssd, nr, NC, step=1, nq=12):
    """find_msav_m internals for a few queries: threshold, index digest, candidates."""
    tmp = tempfile.mkdtemp(prefix="gold_")
    fa = os.path.join(tmp, "ref.fsa")
    open(fa, "wb").write(fasta)
    DB = m.Fasta(open(fa, "rb"))
    DB.build_msav(space=ssd, nr=nr, step=step, start=0, end=len(DB), ht=NC)
    start = np.array(DB.start, dtype=np.uint32)
    locus = np.array(DB.locus, dtype=np.uint32)
    soas = np.array(DB.soas, dtype=np.uint32)
    nz = np.nonzero(np.diff(np.concatenate([start, [len(locus)]])))[0]
    d = {"ssd": ssd, "nr": nr, "NC": NC, "step": step, "threshold": int(DB.threshold), "n_locus": int(len(locus)),
         "soas": soas.tolist(), "nonempty_buckets": nz[:2000].tolist(), "start_at_nonempty": start[nz[:2000]].tolist(),
         "locus_head": locus[:4000].tolist(), "locus_sum": int(locus.astype(np.int64).sum()),
         "start_sum": int(start.astype(np.int64).sum()), "queries": []}
    for i in range(min(nq, len(DB))):
        hd, sq = DB[i]
        sqi = m.seg(sq)[0]
        cands = DB.find_msav_m(sqi, sort=False)
        d["queries"].append({"i": i, "masked": sqi, "cands": [[int(x) for x in c] for c in cands]})
    open(os.path.join(GOLD, name + ".ref.fsa"), "wb").write(fasta)
    json.dump(d, open(os.path.join(GOLD, name + ".stage.json"), "w"))
    print(name, "threshold", d["threshold"], "locus", d["n_locus"])


def kats(m):
    rng = np.random.default_rng(5)
    k = {}
    # BLOSUM62 over raw bytes: full 256x256 as a nested list of the 46 interesting rows/cols + default
    letters = "ABCDEFGHIKLMNPQRSTVWXYZ"
    k["b62_letters"] = letters
    k["b62_23x23"] = [[m.b62[ord(a)][ord(b)] for b in letters] for a in letters]
    k["b62_default"] = m.b62[ord("U")][ord("U")]
    k["b62_probe"] = [[a, b, m.b62[a][b]] for a, b in
                      [(ord("a"), ord("A")), (ord("x"), ord("x")), (ord("x"), ord("A")), (ord("J"), ord("L")), (42, 42),
                       (ord("w"), ord("W")), (ord("b"), ord("n")), (13, 65), (ord("-"), ord("-"))]]
    k["b62_sum"] = int(sum(sum(r) for r in m.b62))
    k["nr_tbl"] = {g: list(m.generate_nr_tbl(g)) for g in (AA9, AA20, AA10B, "KREDQN,C,G,H,ILV,M,F,Y,W,P,STA")}
    seqs = ["MENIHDLWERAL", "MENIHDLWERALAE", "MENIHDLWE", "MKVxxxxxxxxxxxxLLLAAAGGGHHWWPPKKRR", "AXAAAAAAAAAAAAAAAAAAB",
            "".join("ACDEFGHIKLMNPQRSTVWY"[i] for i in rng.integers(0, 20, 200))]
    sp = []
    for s in seqs:
        for ssd, nr, mod, step in [("111111", AA9, 120000000, 1), ("11111011111", AA9, 120000000, 1), ("1111111", AA20, 120000000, 1),
                                   ("111111,1101011", AA9, 1000003, 1), ("1111,1011", AA9 + "/" + AA10B, 97, 1),
                                   ("111111", AA9, 120000000, 3), ("11,11", AA9, 5, 1)]:
            codes = [m.generate_nr_tbl(e) for e in nr.split("/")]
            sp.append({"seq": s, "ssd": ssd, "nr": nr, "mod": mod, "step": step,
                       "out": [[int(a), int(b)] for a, b in m.spseeds(s, step=step, codes=codes, ssps=ssd, mod=mod)]})
    k["spseeds"] = sp
    segs = ["MSSSSSSSSSSSSGAAAAAAPAPAPAPAPAPQQQQQQQQQQQKLMNDERTWYHGFCVIKLMNPQRSTDE", "MKV", "AAAAAAAAAAAA", "ACDEFGHIKLMN",
            "ACDEFGHIKLMNACDEFGHIKLMNAAAAAAAAAAAAAAAAAAAAAAAACDEFGHIKLMNPQRSTVWY", "mkvllaAAAaaaAAAaaaAAAKLMNDERTWYHGFCVIK",
            "A", "AC", "QQQQQQQQQQQQQWERTYIPASDFGHKLCVNM", "WERTYIPASDFGHKLCVNMQQQQQQQQQQQQQ"]
    for _ in range(30):
        n = int(rng.integers(5, 150))
        alpha = "ACDEFGHIKLMNPQRSTVWY"[:int(rng.integers(2, 20))]
        segs.append("".join(alpha[i] for i in rng.integers(0, len(alpha), n)))
    k["seg"] = [{"in": s, "out": m.seg(s)[0]} for s in segs]
    qs = []
    for _ in range(40):
        n = int(rng.integers(0, 400))
        v = [int(x) for x in rng.integers(-5, 6 if n % 2 else 60, n)]
        idx = list(range(n))
        m.qsort(idx, key=lambda i: v[i])
        qs.append({"keys": v, "perm": idx})
    k["qsort"] = qs
    S0 = "MENIHDLWERALAEMEKKVSKPSYETWLKSTKANDIQNDVITITAPNEFARDWLEEHYAG"
    S1 = "MENLHDLWDRALAEMEKVSKPSYETWLRSTKANDIANDQVITITAPNEFARDWLEEHWAG"
    f = m.Fasta.__new__(m.Fasta)
    ug = []
    for q, s, a, b, qlo, slo in [(S0, S1, 10, 10, -1, -1), (S0, S1, 0, 0, -1, -1), (S0, S1, 1, 1, -1, -1), (S0, S1, 30, 30, 20, 20),
                                 (S0, S1, 5, 8, -1, -1), (S0, S1, 59, 59, -1, -1), (S0, S1, 20, 60, -1, -1), (S0, S1, 25, 25, 40, 40),
                                 (S0, S1, 10, -61, -1, -1)]:
        ug.append({"q": q, "s": s, "Qst": a, "Sst": b, "qlo": qlo, "slo": slo, "out": list(f.ungap(q, s, a, b, qlo=qlo, slo=slo))})
    k["ungap"] = ug
    ch = []
    for locs in [[[10, 10], [30, 30], [50, 50]], [[10, 10]], [[1, 1], [2, 2], [3, 3], [40, 40]], [[5, 8], [20, 23]]]:
        ch.append({"q": S0, "s": S1, "locs": locs, "out": list(f.get_ungap_scores(S0, S1, locs))})
    k["ungap_chain"] = ch
    ks = []
    pairs = [(S0, S1, 0, 0), (S0, S1[3:], 3, 0), (S0[10:], S1, 0, 10), (S0[5:40], S1, 0, 2), (S0, S0, 0, 0), (S1, S0, 7, 0),
             (S0, "WWWWWWWWWW", 0, 0), (S0[:20], S1, 0, 0), (S0, S1[:20], 0, 0), (S0, S1, 0, 30), (S0, S1, 30, 0),
             (S0.replace("ETWLK", "xxxxx"), S1, 0, 0)]
    for _ in range(40):
        n = int(rng.integers(20, 260))
        a = "".join("ACDEFGHIKLMNPQRSTVWY"[i] for i in rng.integers(0, 20, n))
        b = list(a)
        for _i in range(int(rng.integers(0, n // 3 + 1))):
            p = int(rng.integers(0, len(b)))
            r = rng.random()
            if r < 0.6:
                b[p] = "ACDEFGHIKLMNPQRSTVWY"[int(rng.integers(0, 20))]
            elif r < 0.8 and len(b) > 5:
                del b[p:p + int(rng.integers(1, 4))]
            else:
                b[p:p] = list("ACDEFGHIKLMNPQRSTVWY"[int(rng.integers(0, 20))] * int(rng.integers(1, 4)))
        b = "".join(b)
        qi, qj = (0, int(rng.integers(0, 6))) if rng.random() < 0.5 else (int(rng.integers(0, 6)), 0)
        pairs.append((a, b, qi, qj))
    sm = [[0] * 4100 for _ in range(4100)]
    tm = [["*"] * 4100 for _ in range(4100)]
    for q, s, a, b in pairs:
        r = m.kswat_st(q, s, qst=a, sst=b, score=sm, trace=tm, al0=[], al1=[])
        ks.append({"q": q, "s": s, "qst": a, "sst": b, "out": [r[0]] + [int(x) for x in r[1:]]})
    k["kswat_st"] = ks
    k["score2bit"] = [[s, int(m.score2bit(s))] for s in (0, 1, 24, 25, 50, 100, 111, 500, 2000, 30000)]
    k["bit2e"] = [[D, a, b, bit, m.bit2e(D, "x" * a, "x" * b, bit)] for D, a, b, bit in
                  [(99, 147, 143, 104), (10000, 300, 300, 30), (1000000, 300, 310, 1000), (5, 3, 3, 1075), (7, 450, 450, 897)]]
    k["f2s"] = [[repr(e), m.f2s(e)] for e in (2.88e-261, 9.9999e-4, 1e-5, 0.5, 0.0, 1.0260511648602738e-25, 1e-3, 9.995e-10,
                                             1e-300, 123.456, 1e-10, 9.99e-7)]
    k["fmt_idy"] = [[repr(x), ("%f" % x)[:("%f" % x).find(".") + 3]] for x in (88.52459016393443, 100.0, 99.99999999, 7.0 * (100. / 9), 0.0)]
    json.dump(k, open(os.path.join(GOLD, "kat.json"), "w"))
    print("kat.json written")


# every residue byte a FASTA line can carry besides the 20 amino acids: lower case, stop, gap, dot, digits, ambiguity and rare letters
ODD_BYTES = "acdwy*-.0123456789BZJUOXx"


def kswat_edges(m):
    """kswat_st at the edges of the GPU aligners (band, tiles, 16-bit packed range): the reference's tuple, the maximum of the score
    matrix over THIS call's band cells (the matrices are reused between calls) and the number of those cells."""
    rng = np.random.default_rng(11)
    aa = "ACDEFGHIKLMNPQRSTVWY"

    def rnd(n, alpha=aa):
        return "".join(alpha[i] for i in rng.integers(0, len(alpha), n))

    def mut(a, rate=0.15, alpha=aa):
        b = list(a)
        for _ in range(int(rng.binomial(len(a), rate))):
            p = int(rng.integers(0, len(b) + 1))
            r = rng.random()
            if r < 0.6 and p < len(b):
                b[p] = alpha[int(rng.integers(0, len(alpha)))]
            elif r < 0.8 and len(b) > 1:
                del b[p:p + int(rng.integers(1, 4))]
            else:
                b[p:p] = list(rnd(int(rng.integers(1, 4)), alpha))
        return "".join(b) or a[:1]

    def sized(a, n):   # a related sequence of exactly n residues
        b = mut(a)
        return (b + rnd(n))[:n]

    pairs = []
    for la in (1, 2, 15, 16, 17, 31, 32, 33):
        a = rnd(la)
        for lb in (la, la + 1, la - 1, la + 16, la + 17, 3 * la + 40):
            if lb < 1:
                continue
            pairs.append((a, sized(a, lb), 0, 0))
            pairs.append((sized(a, lb), a, 0, 0))
        pairs.append((a, rnd(la + 5), 0, 0))
    # starts 0, len - 1, len (the reference is undefined on an empty alignment: such pairs are dropped below), equal windows, far longer
    for la, lb in ((40, 40), (40, 35), (33, 50), (60, 200), (200, 60), (17, 17)):
        a = rnd(la)
        b = sized(a, lb)
        for qst, sst in ((0, 0), (la - 1, 0), (0, lb - 1), (la - 1, lb - 1), (la, 0), (0, lb), (5, 0), (0, 5), (la - lb, 0) if la > lb else (0, lb - la)):
            pairs.append((a, b, qst, sst))
    # ties: homopolymers, period-2 and period-3 repeats (trace priority against the gap-extend cost)
    for a, b in (("A" * 20, "A" * 20), ("A" * 20, "A" * 27), ("W" * 9, "W" * 40), ("AG" * 15, "GA" * 15), ("AG" * 15, "AG" * 12 + "A"),
                 ("ACD" * 12, "CDA" * 12), ("ACD" * 12, "ACD" * 5 + "AC" + "ACD" * 6), ("AAAAGAAAA" * 3, "AAAAAAAA" * 3), ("KR" * 30, "KKRR" * 15),
                 ("LLLLLLLLLLILLLLLLLLL", "LLLLLLLLLLLLLLLLLLLL"), ("P" * 5 + "A" * 30 + "P" * 5, "A" * 33), ("GGGGG", "G" * 60)):
        pairs.append((a, b, 0, 0))
        pairs.append((b, a, 0, 0))
    # raw bytes of FASTA lines
    for _ in range(6):
        a = rnd(int(rng.integers(20, 80)), aa + ODD_BYTES)
        pairs.append((a, mut(a, 0.2, aa + ODD_BYTES), 0, 0))
    pairs.append((ODD_BYTES * 3, ODD_BYTES * 3, 0, 0))
    pairs.append((aa + ODD_BYTES, ODD_BYTES + aa, 0, 0))
    # W-rich pairs at the packed aligners' length limit (11 * min(rows, columns) <= 8179 <=> min <= 740): prefixes of one pair
    w = "".join("W" if rng.random() < 0.8 else aa[int(rng.integers(0, 20))] for _ in range(742))
    w2 = sized(w, 743)
    for n in (739, 740, 741, 742):
        pairs.append((w[:n], w[:n], 0, 0))
        pairs.append((w[:n], w2[:n + 1], 0, 0))
    pairs.append(("W" * 742 + "P", "W" * 742 + "P", 0, 0))
    pairs.append(("W" * 742 + "C", "W" * 742 + "C", 0, 0))
    # windows of 4095 and 4096 residues (a kswat_st_long tile)
    a = rnd(4096)
    b = sized(a, 4096)
    pairs.append((a[:4095], b[:4095], 0, 0))
    pairs.append((a, b, 0, 0))
    pairs.append((a, a, 0, 0))

    sm = [[0] * 4100 for _ in range(4100)]
    tm = [["*"] * 4100 for _ in range(4100)]
    out = []
    for q, s, qst, sst in pairs:
        try:
            r = m.kswat_st(q, s, qst=qst, sst=sst, score=sm, trace=tm, al0=[], al1=[])
        except ZeroDivisionError:   # empty alignment: idy *= 100. / 0 (no answer)
            continue
        # this call's band (kswat_st's swap and loops)
        a0, b0 = min(max(qst, 0), len(q)), min(max(sst, 0), len(s))
        la, lb = len(q) - a0, len(s) - b0
        l0, l1 = (la + 1, lb + 1) if la < lb else (lb + 1, la + 1)
        best, cells = 0, 0
        for i in range(1, l1):
            row = sm[i][max(1, i - 16):min(i + 16, l0)]
            cells += len(row)
            best = max([best] + row)
        out.append((q, s, qst, sst, [r[0]] + [int(x) for x in r[1:]], best, cells))
    # the sequences once (a window is a prefix of one of them): [sequence, length] per side
    seqs = []
    for x in sorted({x for p in out for x in p[:2]}, key=len, reverse=True):
        if not any(y.startswith(x) for y in seqs):
            seqs.append(x)

    def ref(x):
        return [next(i for i, y in enumerate(seqs) if y.startswith(x)), len(x)]

    fields = ["q", "qlen", "s", "slen", "qst", "sst", "idy", "aln", "mis", "gap", "out_qst", "out_qed", "out_sst", "out_sed", "bit", "maxscore",
              "cells"]
    return {"fields": fields, "seqs": seqs, "pairs": [ref(q) + ref(s) + [qst, sst] + o + [best, cells] for q, s, qst, sst, o, best, cells in out]}


def write_kswat_edges(m):
    """kswat_edges.json: kswat_st at the aligners' edges (kept apart from kat.json, whose bytes stay as they are)"""
    path = os.path.join(GOLD, "kswat_edges.json")
    if FORCE or not os.path.isfile(path):
        json.dump(kswat_edges(m), open(path, "w"), separators=(",", ":"))
        print("kswat_edges.json written")


def kswat_aln_edges(m):
    """kswat_st's strings (al0 / al1, query side first) where a co-optimal path or the byte under a column could go wrong: indels in
    homopolymer runs and tandem repeats, literal '-' '*' lower-case and digit bytes (opposite gaps too), either side the longer one and
    equal lengths (the swap), maxima on the band edge, one-residue and empty windows, 4096-residue kswat_st_long tiles.  Every case is
    windows [lo, hi) of two stored sequences aligned from (qst, sst); its strings are kept as a CIGAR over those windows from the
    reported starts (aln_strings in make_aln_goldens.py), verified to rebuild them; an empty alignment (the reference has no answer:
    idy *= 100. / 0) is kept with out = null."""
    from make_aln_goldens import aln_strings, to_cigar
    rng = np.random.default_rng(12)
    aa = "ACDEFGHIKLMNPQRSTVWY"

    def rnd(n, alpha=aa):
        return "".join(alpha[i] for i in rng.integers(0, len(alpha), n))

    def mut(a, rate, alpha=aa):
        b = list(a)
        for _ in range(int(rng.binomial(len(a), rate))):
            p = int(rng.integers(0, len(b) + 1))
            r = rng.random()
            if r < 0.6 and p < len(b):
                b[p] = alpha[int(rng.integers(0, len(alpha)))]
            elif r < 0.8 and len(b) > 1:
                del b[p:p + int(rng.integers(1, 4))]
            else:
                b[p:p] = list(rnd(int(rng.integers(1, 4)), alpha))
        return "".join(b) or a[:1]

    pairs = []   # (q, s, qst, sst) on whole strings, or (q, qlo, qhi, s, slo, shi, qst, sst) for tiles

    def both(a, b):
        pairs.append((a, b, 0, 0))
        pairs.append((b, a, 0, 0))

    L, R = "MKWHDECY", "PRTNYCWF"
    # homopolymer runs with an indel (and a mismatch) inside
    for c in "AGWLK":
        for run in (3, 6, 11):
            for d in (-2, -1, 1, 3):
                both(L + c * run + R, L + c * (run + d) + R)
            x = c * run
            both(L + x + R, L + x[:run // 2] + "P" + x[run // 2 + 1:] + c + R)
    core = rnd(30)
    both(core + "A" * 20 + core[::-1], core + "A" * 17 + core[::-1])
    # tandem repeats with one unit deleted or inserted
    for unit in ("AG", "ACD", "KRWE", "PLNYT", "WC"):
        for k in (3, 6):
            both(L + unit * k + R, L + unit * (k - 1) + R)
            both(L + unit * k + R, L + unit * (k + 1) + R)
            f1, f2 = rnd(25), rnd(25)
            both(f1 + unit * (k + 2) + f2, f1 + unit * (k + 1) + f2)
    # literal '-', '*', lower case and digits, opposite gaps too
    for a, b in (("WCH-DE-FGWC", "WCH-DEFGWC"), ("WCHAB*C*DWCH", "WCHAB*DWCH"), ("WCmkvLLwWC", "WCmkvLwWC"), ("WC0123456789WC", "WC012356789WC"),
                 ("WC---WC", "WC-WC"), ("WCH--**--HCW", "WCH-*-HCW"), ("WWacdwyWW", "WWacdyWW"), ("CW-W-C", "CWWC"), ("W*W*W*W", "W*W*W"),
                 ("HW.x.xWH", "HW.xWH"), ("WCWC" + "-" * 6 + "WCWC", "WCWC--WCWC")):
        both(a, b)
    for _ in range(6):
        a = rnd(int(rng.integers(20, 70)), aa + ODD_BYTES)
        both(a, mut(a, 0.2, aa + ODD_BYTES))
    # query longer, shorter, equal (equal lengths take the swap branch)
    for la, lb in ((50, 60), (60, 50), (55, 55), (120, 121), (121, 120), (200, 200), (1, 1), (2, 2)):
        a = rnd(la)
        b = (mut(a, 0.1) + rnd(lb))[:lb]
        pairs.append((a, b, 0, 0))
    # maxima on the band edge |i - j| = 16 (and one in, one out)
    for off in (15, 16, 17):
        cpart = rnd(40, "WCHYM")
        both(cpart, rnd(off) + cpart)
        both(cpart + rnd(5), rnd(off) + cpart)
    # one-residue windows; starts at len - 1 and len (empty: no answer)
    a, b = rnd(30), rnd(30)
    b = a[:10] + b[10:]
    for qst, sst in ((29, 0), (0, 29), (29, 29), (30, 0), (0, 30), (30, 30), (29, 5)):
        pairs.append((a, b, qst, sst))
    for a, b in (("W", "W"), ("W", "MKWV"), ("MKWV", "W"), ("A", "C")):
        pairs.append((a, b, 0, 0))
    # 4096-residue tiles as kswat_st_long frames them: [i, i + 4096) of the query against [j, j + 4096) of the subject, j = i
    A = rnd(6000)
    B = mut(A[:3000], 0.03) + "L" * 20 + mut(A[3000:], 0.05)
    for i in (0, 4096):
        pairs.append((A, i, min(len(A), i + 4096), B, i, min(len(B), i + 4096), 0, 0))
    C_ = "AG" * 2048
    pairs.append((C_, 0, 4096, C_[:2000] + C_[2002:] + "AG", 0, 4096, 0, 0))

    sm = [[0] * 4100 for _ in range(4100)]
    tm = [["*"] * 4100 for _ in range(4100)]
    out = []
    for p in pairs:
        q, qlo, qhi, s, slo, shi, qst, sst = p if len(p) == 8 else (p[0], 0, len(p[0]), p[1], 0, len(p[1]), p[2], p[3])
        qw, sw = q[qlo:qhi], s[slo:shi]
        al0, al1 = [], []
        try:
            r = m.kswat_st(qw, sw, qst=qst, sst=sst, score=sm, trace=tm, al0=al0, al1=al1)
        except ZeroDivisionError:   # empty alignment: no answer
            out.append((q, qlo, qhi, s, slo, shi, qst, sst, None, None))
            continue
        a0, a1 = _b(al0), _b(al1)
        qb, sb = qw.encode("latin-1"), sw.encode("latin-1")
        cig = to_cigar(a0, a1, qb, sb, r[4] + 1, r[5], r[6] + 1, r[7])
        assert cig is not None and aln_strings(cig, qb, sb, r[4] + 1, r[6] + 1) == (a0, a1), (qw[:40], sw[:40])
        out.append((q, qlo, qhi, s, slo, shi, qst, sst, [r[0]] + [int(x) for x in r[1:]], cig))
    seqs = []
    for x in sorted({x for c in out for x in (c[0], c[3])}, key=lambda x: (-len(x), x)):   # (not set order: string hashes vary per process)
        if not any(y.startswith(x) for y in seqs):
            seqs.append(x)

    def ref(x):
        return next(i for i, y in enumerate(seqs) if y.startswith(x))

    fields = ["q", "qlo", "qhi", "s", "slo", "shi", "qst", "sst", "out", "cigar"]
    return {"fields": fields, "out_fields": ["idy", "aln", "mis", "gap", "qst", "qed", "sst", "sed", "bit"], "seqs": seqs,
            "cases": [[ref(c[0]), c[1], c[2], ref(c[3])] + list(c[4:]) for c in out]}


def _b(x):
    return "".join(x).encode("latin-1") if not isinstance(x, (bytes, bytearray)) else bytes(x)


def write_kswat_aln_edges(m):
    """kswat_aln_edges.json: kswat_st's strings at the edges (kept apart from kswat_edges.json, whose bytes stay as they are)"""
    path = os.path.join(GOLD, "kswat_aln_edges.json")
    if FORCE or not os.path.isfile(path):
        with open(path, "w") as f:
            json.dump(kswat_aln_edges(m), f, separators=(",", ":"))
            f.write("\n")
        print("kswat_aln_edges.json written")


def main():
    os.makedirs(GOLD, exist_ok=True)
    m = refload.load()
    if FORCE or not os.path.isfile(os.path.join(GOLD, "kat.json")):
        kats(m)
    write_kswat_edges(m)
    write_kswat_aln_edges(m)
    rng = np.random.default_rng(1)
    base = ["-e", "1e-5", "-v", "500", "-j", "1", "-F", "T"]
    run_e2e(m, "toy_default", synthprot.synthprot(99, 150, 21), base + ["-s", "111111", "-r", AA9, "-M", "1000003", "-c", "50000"])
    run_e2e(m, "toy_chunks", synthprot.synthprot(90, 120, 6), base + ["-s", "111111", "-r", AA9, "-M", "1000003", "-c", "40"])
    run_e2e(m, "toy_multiseed", synthprot.synthprot(80, 100, 3), base + ["-s", "111111,1101011", "-r", AA9, "-M", "1000003", "-c", "50000"])
    run_e2e(m, "toy_twoalpha", synthprot.synthprot(80, 100, 5),
            base + ["-s", "11111", "-r", AA9 + "/" + AA10B, "-M", "300007", "-c", "25000"])
    run_e2e(m, "toy_uniform", synthprot.uniform_proteins(60, 150, 8), base + ["-s", "111111", "-r", AA9, "-M", "5003", "-c", "50000"])
    run_e2e(m, "toy_messy", messy_fasta(rng), ["-e", "1e-3", "-v", "5", "-j", "1", "-F", "T", "-s", "111111", "-r", AA9, "-M", "1000003", "-c", "10"])
    run_e2e(m, "toy_oddchars", oddchar_fasta(), ["-e", "1e-3", "-v", "500", "-j", "1", "-F", "T", "-s", "111111", "-r", AA9, "-M", "1000003", "-c", "50000"])
    qref, qqry = fasta_quirks()
    run_e2e(m, "toy_fastaquirks", qref, ["-e", "1e-3", "-v", "500", "-j", "1", "-F", "T", "-s", "111111", "-r", AA9, "-M", "1000003", "-c", "50000"], qry=qqry)
    rref, rqry = ragged_queries()
    run_e2e(m, "toy_ragged", rref, ["-e", "1e-3", "-v", "500", "-j", "1", "-F", "T", "-s", "111111", "-r", AA9, "-M", "1000003", "-c", "50000"], qry=rqry)
    run_e2e(m, "toy_w10", synthprot.synthprot(70, 200, 12), base + ["-s", "11111011111", "-r", AA9, "-M", "120000000", "-c", "50000"])
    refA, qryA, refB, qryB = long_sets()
    lf = ["-e", "1e-5", "-v", "500", "-j", "1", "-F", "T", "-s", "111111", "-r", AA9, "-M", "1000003", "-c", "50000"]
    run_e2e(m, "toy_long_subject", refA, lf, qry=qryA)
    run_e2e(m, "toy_long_both", refB, lf, qry=qryB)
    run_e2e(m, "toy_aa20", synthprot.synthprot(80, 100, 4), base + ["-s", "1111111", "-r", AA20, "-M", "50021", "-c", "50000"])
    qry = open(os.path.join(refload.REFERENCE, "example", "qry.fsa"), "rb").read()
    # config 1 (example/run.sh plumbing): the shipped ref.fsa is absent -> stand-in reference with the
    # query and three mutated copies planted among synthetic proteins
    ref = synthprot.synthprot(40, 300, 31)
    q = qry.split(b"\n")[1].decode()
    rr = np.random.default_rng(3)
    planted = []
    for t, d in enumerate((0.0, 0.1, 0.3, 0.5)):
        s = list(q)
        for p in range(len(s)):
            if rr.random() < d:
                s[p] = "ACDEFGHIKLMNPQRSTVWY"[int(rr.integers(0, 20))]
        planted.append(">t%04d|planted%d copy d=%.1f\n%s\n" % (t, t, d, "".join(s)))
    ref = ref + "".join(planted).encode()
    run_e2e(m, "example_cfg1", ref, ["-e", "1e-5", "-s", "111111", "-r", AA9, "-M", "120000000", "-c", "50000", "-j", "1"], qry=qry)
    # the launcher itself (find_hit.py:95-146, 303-351): more queries than references (End < 0 -> N, the QUERY count), the block
    # scheme with -a 3 (the last block runs past -u), and the reference split + `sort -m | awk` merge with max_chr forced low
    whole = synthprot.synthprot(70, 120, 9)
    fh = ["-e", "1e-5", "-s", "111111", "-M", "1000003", "-c", "50000"]
    run_find_hit("fh_more_queries", first_records(whole, 30), whole, fh)
    run_find_hit("fh_blocks", first_records(whole, 30), whole, fh + ["-a", "3", "-l", "5", "-u", "48"])
    run_find_hit("fh_split", whole, first_records(whole, 40), fh + ["-v", "1"], max_chr=3000)
    # on-disk index files (Fasta.makedb / Fasta.write, fsearch.py:2283-2352) as the reference writes them
    if FORCE or not os.path.isfile(os.path.join(GOLD, "idx_toy.json")):
        tmp = tempfile.mkdtemp(prefix="gold_")
        fa = synthprot.synthprot(60, 100, 3)
        p = os.path.join(tmp, "ref.fsa")
        open(p, "wb").write(fa)
        args = dict(space="111111,1101011", nr=AA9, step=1, ht=5003, chk=25)
        m.makedb(p, **args)
        open(os.path.join(GOLD, "idx_toy.ref.fsa"), "wb").write(fa)
        files = sorted(f for f in os.listdir(tmp) if f.startswith("ref.fsa."))
        for f in files:
            open(os.path.join(GOLD, "idx_toy" + f[len("ref.fsa"):]), "wb").write(open(os.path.join(tmp, f), "rb").read())
        json.dump({"args": args, "files": [f[len("ref.fsa"):] for f in files]}, open(os.path.join(GOLD, "idx_toy.json"), "w"), indent=1)
        print("idx_toy", files)
    stage_dump(m, "stage_default", synthprot.synthprot(99, 150, 21), "111111", AA9, 1000003)
    stage_dump(m, "stage_multi", synthprot.synthprot(60, 100, 3), "111111,1101011", AA9 + "/" + AA10B, 200003)


if __name__ == "__main__":
    main()
