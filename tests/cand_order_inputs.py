"""Inputs for tests/test_gpu_cand_order.py: protein sets whose PASSING diagonals are planted on the edges of the candidate stage -- best
diagonal per (query, subject), then a query's candidates in first-touch order -- and a plain model of that stage.

Parameters of every set: seed 111111 over the 9-class alphabet, step 1, -F F, the frequency cap out of reach (thr), queries in a file of
their own.  The hits are bucket_ungap_inputs.BucketModel's (a hit = query window x index entry of its bucket, the offset-0 entry of a
sequence kept under the sequence in front of it at the position behind its last residue, that of a chunk's first sequence dropped).

The model of the stage (expected_cands): the reference visits a query's windows by position and the entries of a window's bucket by
DESCENDING entry value -- owner sequence, then position, so the offset-0 entry of sequence j + 1 (filed under subject j) comes behind every
real entry of j + 1 and in front of every entry of j.  A hit's visiting key is (query position, -owner, -position in the owner), a
diagonal's FIRST-TOUCH key the smallest one of its hits.  A diagonal is a pass record when its chained ungapped score (oracle.ungap_chain
over its hits) is >= 25.  A subject with records is a candidate: its record is the one of maximum score (strict >: of equal scores the
smaller first-touch key wins), qi / qj the diagonal sst - qst (> 0: qj), its place among the query's candidates the MINIMUM first-touch
key of all its records -- which may belong to a diagonal that is not the best one.  Candidates of a query leave chunk-major.

Planting.  A PIECE is a 6-mer over the 18 letters without G and P, no two pieces of a set of one class string, each scoring >= 25 against
itself (bucket_ungap_inputs._strong_pieces).  Queries are pieces with a P behind each, subjects pieces with a G behind each: a window that
holds a separator meets nothing (no subject holds a P, no query a G), a window that is a piece meets exactly the copies of that piece.
Every hit is therefore planned, every diagonal a singleton, and its score is at least the piece's own (the X-drop pass may add a few
points from the neighbours: the model takes the score from oracle.ungap_chain on the one pair involved).  Where a score has to be EXACT (the
tie set) the pieces of a subject stand between runs of 40 G: G scores at most 0 against every residue of a query (which holds no G), so
nothing outside the piece adds to a pass and 40 pairs end it; the score is the sum of oracle.b62 over the piece's own six pairs, asserted
against oracle.ungap_chain.  (Not flanks of -4 pairs from bucket_ungap_inputs._Cross: BLOSUM62 has so few pairs of -4 that thirty
flanks of them meet each other's windows in every draw.)  Pieces of a wanted score: residues that score 4 (A I L S V), 5 (E
K M Q R T), 6 (D F N), 7 (Y), 8 (H), 9 (C), 11 (W) against themselves; 24 = 6 x 4, 25 = 5 x 4 + 5.

tier_set: k_q_best's instances (128, 512, 2048 records of a query) and its overflow.  Query R of TIERS has exactly R records, spread over
subjects that carry 65, 63, 64 ... and the remainder (1 for 65, 129, 513, 2049; 2 for the query of 2 records) -- a subject with c records holds c
of the query's pieces in REVERSE order, so that query positions rise while subject positions fall: c different diagonals.  Runs of 63, 64
and 65 records of one subject: the run loop of a head lane ends in front of, on and behind a 64-lane stride.  Three more queries have 2049 records
(the overflow: the pass is redone by the sorted flow) on 256, 257 and 2049 subjects: maxseg = 256 (k_cand_order_lds<256>), 257 (<2048>)
and 2049 (the device-wide sort).  All queries have fewer than 512 residues (65 pieces: 456): one length class, one pass.  Some 80 000
residues.  Query ranges: `where["ranges"]`.

tie_set: one query (`ties`) against fifteen subjects, 259 filler queries of one piece (so that the pass has >= 256 queries:
k_cand_order_seg), and a last query of 4100 residues P W P W ... that meets nothing: with SOHIT_BUCKET=0 all length classes are one pass, its
pmaxq >= 4096 keeps the per-query flow away and the SORTED flow runs without an overflow.  The cases, in the order of the query:
  two, three      two / three diagonals of equal score (30 / 31) on one subject, the earliest one NOT the first in the subject: it wins
  early           a diagonal of 26 in front of one of 40 on subject C, and subject M's only diagonal between them in the query: C's record is
                  the 40, its place in front of M
  same            one piece, one query position, subjects E1 and E2: E2 (the higher number) comes first
  quirk           subject J1 BEGINS with piece X and holds it again; subject J in front of it ends with eleven residues that score 78
                  against the eleven in front of X in the query without a window of one class (five identical residues, D against E, five
                  more): the offset-0 entry of J1 is filed under J behind its last residue and its left pass makes J a candidate whose
                  first-touch key is an offset-0 entry.  X is also in I (in front of J) and in J2 (behind J1): the order at that query
                  position is J2, J1, J, I -- J1's real entry in front of its offset-0 entry (the bit (ft & pm) == pm), which a sort that
                  dropped the bit would leave in subject order: J, J1
  exact           diagonals of 24 and of 25 on subject F, the 24 first, and subject N's only diagonal between them: F is a candidate of score
                  25 BEHIND N (a 24 that counted would put it in front)
  dist            diagonals sst - qst of +37, of -(the query position - 9) and of 0: qj, qi, neither
The tie subjects stand in the middle of the reference: chk = `where["chk"]` cuts them into two chunks (7 and 8), the candidates are chunk-major.

seg_set: k_cand_order_seg (bucketed best, >= 256 queries in the pass; CO_CAP = 16384 candidates per sub-pass, digit = the top CO_DBITS =
11 bits of the first-touch word).  The first-touch word is (query position: bp bits)(owner + 1: bs + 1 bits)(offset-0 bit).  The set has
32 785 + 256 subjects (bs = 16) and its longest query has 511 residues (bp = 9): the digit is (query position, owner >> 15) -- every query position
has digits of its own, and inside a position the subjects below and from 32 768 on are two digits.
  b    one piece X, in subjects 0 .. 16 399: 16 400 candidates of ONE query position and one digit (> CO_CAP): the fall-back to the
       segmented library sort.  k_bkt_group does not refuse the pass: it refuses a subject sub-range of more than BG_CAP = 4096 hits and
       divides a bucket down to single subjects; here every subject brings one hit.
  a1   sixteen pieces, each in 1024 subjects (16 400 .. 32 783): 16 384 candidates, 17 digits (the last sixteen subjects lie beyond
       32 768: both sides of a digit edge inside one query position): ONE sub-pass
  a2   the same and piece Z (subject 32 784) in its middle: 16 385 candidates, TWO sub-passes
  c    511 residues, a piece at position 1 and one at position 505 (the last window), G P G P ... between them: the first and the last
       digit a candidate of this pass can have (a hit at query position 0 scores nothing in the reference: oracle.ungap returns 0 for it)
  and 256 queries of one piece, one candidate each (the one whose piece has the chunk's highest bucket may lose it: the slot the
  reference never reads).  Some 230 000 residues; with SOHIT_BATCH below 256 the passes have fewer than 256 queries: the device-wide sort.

sort2_set: the device-wide order in TWO sorts (ftbits + bq > 64; one sort on (query, first-touch) otherwise).  With one alphabet and one
pattern ftbits = bp + (bs + 1) + bsp, and the sort key of the hits has to fit as well: bq + bs + bd + bp <= 64 with bd = the bits of
pmaxq + maxslen + 1 (sequences numbered, no bands).  So bsp + 1 > bd: the subject decides both, the query stays a quarter of it.  A
subject of 2^20 + 1 residues (G only: bsp = bd = 21), a query of 2^18 + 1 (P W P W ...: bp = 19; neither meets anything), 2055 subjects
(bs = 12) and 2052 queries in the batch (bq = 12): key 64 bits, ftbits 53, ftbits + bq 65.  The long query puts pmaxq above 4096 (with
SOHIT_BUCKET=0 all length classes are one pass: no per-query flow), a query with a piece in each of 2052 subjects puts maxseg above 2048
(no LDS order), two small queries stand on either side of it, and 2048 queries P W P W P W P W fill the batch.  Some 1.3 M residues.

What is NOT here, with the arithmetic:
  * a digit of all ones (2047): the query position field of a pass whose longest query has 511 residues ends at 505, the owner field at
    33 041 of 131 072.
  * the seed 11111011111: a piece of eleven residues makes a query of 65 pieces 781 residues long, above k_ungapq's 512; the stage under
    test starts at the pass records, which do not depend on the seed.  The per-query flow is reached with 111111 through SOHIT_BUCKET=0 (the
    sorted grouping, k_ungapq included when the pass has 256 queries) and through SOHIT_BUCKET_BEST=0 (the bucketed grouping)."""
import numpy as np

from bucket_ungap_inputs import AA18, CLS, K, SEED, BucketModel, _join, _strong_pieces, b62  # noqa: F401
from uqchain_inputs import HT, to_fasta  # noqa: F401

MIN_UNGAP = 25
Q_BEST_TIERS = (128, 512, 2048)   # k_group.hip: the instances of k_q_best
CO_CAP = 16384                    # k_bucket.hip
TIERS = (1, 2, 64, 65, 128, 129, 512, 513, 2047, 2048)
_G = np.frombuffer(b"G", dtype=np.uint8)
_P = np.frombuffer(b"P", dtype=np.uint8)


def expected_cands(oracle, m, q, chk=None):
    """(candidates [[subject, score, qi, qj], ...] of query q in spill order, records per chunk, candidates per chunk): the model in the
    head of the file"""
    sid, pos, qp, drop = m.hits(q)
    lens = np.array([len(x) for x in m.refs], dtype=np.int64)
    quirk = pos == lens[sid]          # (a real entry lies K and more in front of the end)
    owner, raw = sid + quirk, np.where(quirk, 0, pos)
    keep = np.flatnonzero(~drop)
    keep = keep[np.lexsort((-raw[keep], -owner[keep], qp[keep]))]   # visiting order
    chunk = sid // chk if chk else sid * 0
    qs = m.qrys[q].tobytes()
    out, nrec, ncand = [], [], []
    for c in np.unique(chunk[keep]):
        groups = {}
        for i in keep[chunk[keep] == c]:
            groups.setdefault((int(sid[i]), int(pos[i] - qp[i])), []).append((int(qp[i]), int(pos[i])))
        best, n = {}, 0
        for (s, d), locs in groups.items():   # (in first-touch order: dicts keep the order of insertion)
            sc = oracle.ungap_chain(qs, m.refs[s].tobytes(), sorted(locs))[0]
            if sc < MIN_UNGAP:
                continue
            n += 1
            if s not in best:
                best[s] = [s, sc, d]
            elif sc > best[s][1]:
                best[s][1:] = [sc, d]
        out += [[s, sc, 0 if d > 0 else -d, d if d > 0 else 0] for s, sc, d in best.values()]
        nrec.append(n), ncand.append(len(best))
    return out, nrec, ncand


def _subject(pieces):
    return _join(pieces, b"G")


def _query(pieces):
    return _join(pieces, b"P")


# ================================================================================================================
# tiers of k_q_best, its overflow, maxseg of the sorted flow
# ================================================================================================================
def spread(R):
    """records per subject of the query of R records: 65, 63, then 64s, then the remainder"""
    out = []
    if R >= 128:
        out, R = [65, 63], R - 128
    while R >= 64:
        out.append(64)
        R -= 64
    return out + ([R] if R else [])


OVER = {"over256": [9] + [8] * 255, "over257": [8] * 250 + [7] * 7, "over2049": [1] * 2049}


def tier_set(oracle, seed=50511):
    """(reference fasta, query fasta, model, where).  where: "tier" {R: query}, "over" {name: query}, "spread" {query: records per
    subject}, "subjects" {query: (first, behind the last)}, "ranges" {name: (first query, behind the last)} -- "tiers" (the ten, no
    overflow), "tiers_over256" (the ten and a query of 2049 records on 256 subjects), "over257" and "over2049" (the query between two small
    ones)"""
    rng = np.random.default_rng(seed)
    plan = [("tier", R, spread(R)) for R in TIERS] + [("over", "over256", OVER["over256"])] + [("small", 0, [2, 1])] + \
           [("over", "over257", OVER["over257"])] + [("small", 1, [3])] + [("over", "over2049", OVER["over2049"])] + [("small", 2, [1, 1])]
    npc = [max(16, max(sp)) if kind != "over" or name != "over2049" else 64 for kind, name, sp in plan]
    pool = _strong_pieces(oracle, rng, sum(npc))
    refs, qrys, where = [], [], {"tier": {}, "over": {}, "small": {}, "spread": {}, "subjects": {}}
    for (kind, name, sp), n in zip(plan, npc):
        pc, pool = pool[:n], pool[n:]
        q = len(qrys)
        qrys.append(_query(pc))
        where[kind][name] = q
        where["spread"][q] = sp
        first = len(refs)
        for t, c in enumerate(sp):
            pick = sorted(int(i) for i in rng.choice(n, size=c, replace=False)) if c > 1 else [t % n]
            refs.append(_subject([pc[i] for i in pick[::-1]]))
        where["subjects"][q] = (first, len(refs))
    t, o = where["tier"], where["over"]
    where["ranges"] = {"tiers": (0, len(TIERS)), "tiers_over256": (0, o["over256"] + 1), "over257": (o["over256"] + 1, o["over257"] + 2),
                       "over2049": (o["over257"] + 1, o["over2049"] + 2)}
    assert t[1] == 0 and where["ranges"]["over2049"][1] == len(qrys) and max(len(x) for x in qrys) < 512
    return to_fasta(refs), to_fasta(qrys), BucketModel(oracle, refs, qrys), where


# ================================================================================================================
# ties, the minimum key, equal query positions, the offset-0 bit, 24 / 25, the sign of the diagonal
# ================================================================================================================
_BY_SCORE = {4: b"AILSV", 5: b"EKMQRT", 6: b"DFN", 7: b"Y", 8: b"H", 9: b"C", 11: b"W"}


def _scored_piece(oracle, rng, score, seen):
    """a 6-mer that scores exactly `score` against itself, of a class string not in `seen`"""
    for _ in range(100000):
        v, left = [], score
        for k in range(K - 1, -1, -1):   # (each residue drawn from the scores that leave the rest in reach: 4 .. 11 per residue)
            ok = [x for x in _BY_SCORE if 4 * k <= left - x <= 11 * k and (k or left - x == 0)]
            if not ok:
                break
            v.append(int(rng.choice(ok)))
            left -= v[-1]
        if len(v) != K or left:
            continue
        v = np.array(v)[rng.permutation(K)]
        p = np.array([_BY_SCORE[int(x)][int(rng.integers(len(_BY_SCORE[int(x)])))] for x in v], dtype=np.uint8)
        key = CLS[p].tobytes()
        if key not in seen and len(set(CLS[p].tolist())) >= 2:
            assert sum(b62(oracle, a, a) for a in p) == score
            seen.add(key)
            return p
    raise AssertionError("no piece of score %d" % score)


class _Seq:
    def __init__(self):
        self.parts, self.n, self.at = [], 0, {}

    def add(self, arr, name=None, core=0):
        if name is not None:
            self.at[name] = self.n + core
        self.parts.append(np.asarray(arr, dtype=np.uint8))
        self.n += len(arr)
        return self

    def seq(self):
        return np.concatenate(self.parts)


TAIL_Q, TAIL_S = b"WHKDYDCWHKD", b"WHKDYECWHKD"   # 11 + 8 + 5 + 6 + 7 + 2 + 9 + 11 + 8 + 5 + 6 = 78, runs of one class: 5 and 5
TIE_SCORES = {"a1": 30, "a2": 30, "b1": 31, "b2": 31, "b3": 31, "c1": 26, "m": 30, "c2": 40, "e": 30, "f24": 24, "n": 30, "f25": 25, "gp": 30, "gn": 30,
              "g0": 30}
TIE_QUERY = ("a1", "a2", "b1", "b2", "b3", "c1", "m", "c2", "e", "quirk", "f24", "n", "f25", "gp", "gn", "g0")
N_FILL = 259
TIE_RUN = 40   # G between two pieces of a tie subject


def tie_set(oracle, seed=50512):
    """(reference fasta, query fasta, model, where).  where: "ties" (the query), "subj" {name: subject}, "qpos" / "score" {segment: query
    position of its piece / its score}, "spos" {(subject name, segment): subject position}, "chk", "ranges" {"small": without the last query, "all": with it}, "order" / "order2" (the
    candidates of `ties` as [subject, score, qi, qj] in one chunk / at chk)"""
    rng = np.random.default_rng(seed)
    bad = None
    for _ in range(64):
        seen = set()
        seg = {name: _scored_piece(oracle, rng, sc, seen) for name, sc in TIE_SCORES.items()}
        px = _scored_piece(oracle, rng, 33, seen)
        fill = [p for p in _strong_pieces(oracle, rng, N_FILL + 40) if CLS[p].tobytes() not in seen][:N_FILL]
        q = _Seq().add(_P)
        for name in TIE_QUERY:
            if name == "quirk":
                q.add(np.frombuffer(TAIL_Q, dtype=np.uint8)).add(px, "quirk").add(_P)
            else:
                q.add(seg[name], name).add(_P)
        qpos = q.at

        def run(n):
            return np.full(n, ord("G"), dtype=np.uint8)

        def subj(names, lead=TIE_RUN):
            s = _Seq().add(run(lead))
            for name in names:
                s.add(seg[name], name).add(run(TIE_RUN))
            return s

        tie = [("A", subj(["a2", "a1"])), ("B", subj(["b3", "b1", "b2"])), ("C", subj(["c2", "c1"])), ("M", subj(["m"])), ("E1", subj(["e"])),
               ("E2", subj(["e"], TIE_RUN + 5)), ("I", _Seq().add(_G).add(px).add(_G)), ("J", _Seq().add(run(5)).add(np.frombuffer(TAIL_S, dtype=np.uint8))),
               ("J1", _Seq().add(px).add(run(9)).add(px).add(_G)), ("J2", _Seq().add(_G).add(px)),
               ("F", subj(["f25", "f24"])), ("N", subj(["n"])), ("Gp", subj(["gp"], qpos["gp"] + 37)), ("Gn", subj(["gn"])), ("G0", subj(["g0"], qpos["g0"]))]
        front = 130
        refs = [_subject([p]) for p in fill[:front]] + [s.seq() for _, s in tie] + [_subject([p]) for p in fill[front:]]
        qrys = [q.seq()] + [_query([p]) for p in fill] + [np.frombuffer(b"PW" * 2050, dtype=np.uint8)]
        where = {"ties": 0, "subj": {name: front + i for i, (name, _) in enumerate(tie)}, "qpos": dict(qpos), "score": dict(TIE_SCORES, quirk=33),
                 "spos": {(name, k): v for name, sq in tie for k, v in sq.at.items()}, "chk": front + 7, "ranges": {"small": (0, 1 + N_FILL), "all": (0, 2 + N_FILL)}}
        S = where["subj"]
        d = {name: s.at for name, s in tie}

        def cand(sname, segname, score=None):
            dist = d[sname][segname] - qpos[segname]
            return [S[sname], TIE_SCORES[segname] if score is None else score, 0 if dist > 0 else -dist, dist if dist > 0 else 0]

        lj = len(tie[7][1].seq())
        dq = lj - qpos["quirk"]   # the offset-0 entry of J1 under J: subject position = J's length
        dj1 = (K + 9) - qpos["quirk"]
        order = [cand("A", "a1"), cand("B", "b1"), cand("C", "c2"), cand("M", "m"), cand("E2", "e"), cand("E1", "e"),
                 [S["J2"], None, qpos["quirk"] - 1, 0], [S["J1"], None, -dj1, 0], [S["J"], None, 0 if dq > 0 else -dq, dq if dq > 0 else 0],
                 [S["I"], None, qpos["quirk"] - 1, 0], cand("N", "n"), cand("F", "f25"), cand("Gp", "gp"), cand("Gn", "gn"), cand("G0", "g0")]
        m = BucketModel(oracle, refs, qrys)
        m2 = BucketModel(oracle, refs, qrys, chk=where["chk"])
        where["order"], where["order2"] = order, [c for c in order if c[0] < where["chk"]] + [c for c in order if c[0] >= where["chk"]]
        bad = tie_problems(oracle, m, m2, where)
        if not bad:
            return to_fasta(refs), to_fasta(qrys), m, where
    raise AssertionError("the planted cases keep meeting chance matches: %r" % (bad[:4],))


def _same(exp, got):
    """`exp` with None for a score the design leaves to the neighbours"""
    return len(exp) == len(got) and all(e[0] == g[0] and e[2:] == g[2:] and (e[1] is None or e[1] == g[1]) for e, g in zip(exp, got))


def tie_problems(oracle, m, m2, where):
    """what keeps the set from being the one the head describes ([]: nothing)"""
    bad = []
    q = where["ties"]
    if len(m.qrys[q]) >= 512:
        bad.append("length")
    got, nrec, ncand = expected_cands(oracle, m, q)
    if not _same(where["order"], got):
        bad.append(("order", got))
    # records: two, three, two (26 and 40), one (the 24 is none) ... : every planted diagonal but f24, and nothing else
    if nrec != [len(TIE_SCORES) - 1 + 1 + 4]:   # the segments but f24, e twice; X in I, J1, J2 and, through J1's offset-0 entry, in J
        bad.append(("records", nrec))
    got2, nrec2, ncand2 = expected_cands(oracle, m2, q, where["chk"])
    if not _same(where["order2"], got2) or ncand2 != [7, 8]:
        bad.append(("order2", got2, ncand2))
    # the designed scores are exact: the piece's own pairs
    qs = m.qrys[q].tobytes()
    for sname, segname in (("A", "a1"), ("A", "a2"), ("B", "b1"), ("B", "b2"), ("B", "b3"), ("C", "c1"), ("C", "c2"), ("F", "f24"), ("F", "f25")):
        s, p, sp = where["subj"][sname], where["qpos"][segname], where["spos"][(sname, segname)]
        if m.hits_on(q, s).get(sp - p) != 1 or oracle.ungap_chain(qs, m.refs[s].tobytes(), [(p, sp)])[0] != where["score"][segname]:
            bad.append(("score", sname, segname))
    # the fillers: a candidate each (but the one the reference's unread slot takes away)
    if sum(len(m.hits(f)[0]) for f in range(1, 1 + N_FILL)) < N_FILL - 1 or len(m.hits(1 + N_FILL)[0]):
        bad.append("fillers")
    return bad


# ================================================================================================================
# k_cand_order_seg: one and two sub-passes, a digit group above CO_CAP, the first and the last digit
# ================================================================================================================
SEG_B, SEG_PER, SEG_NY, SEG_FILL = 16400, 1024, 16, 256


def seg_set(oracle, seed=50513):
    """(reference fasta, query fasta, model, where).  where: "a1", "a2", "c" (queries 0 .. 2), "b" (the LAST query, behind the 256 of one
    piece), "ncand" {query: candidates}, "ranges" {"sub_passes": all queries but b (259), "resort": all 260}"""
    bad = None
    for k in range(16):
        rng = np.random.default_rng(seed + k)
        pool = _strong_pieces(oracle, rng, 2 + SEG_NY + SEG_FILL)
        x, z, ys, fl = pool[0], pool[1], pool[2:2 + SEG_NY], pool[2 + SEG_NY:]
        refs = [_subject([x])] * SEG_B + [_subject([ys[i // SEG_PER]]) for i in range(SEG_NY * SEG_PER)] + [_subject([z])] + [_subject([p]) for p in fl]
        gp = np.frombuffer(b"PP" + b"GP" * 248, dtype=np.uint8)
        qrys = [_query(ys), _query(ys[:8] + [z] + ys[8:]), np.concatenate([_P, ys[0], gp, ys[-1]])] + [_query([p]) for p in fl] + [_query([x])]
        m = BucketModel(oracle, refs, qrys)
        nq = len(qrys)
        where = {"a1": 0, "a2": 1, "c": 2, "b": nq - 1, "ncand": {0: SEG_NY * SEG_PER, 1: SEG_NY * SEG_PER + 1, 2: 2 * SEG_PER, nq - 1: SEG_B},
                 "ranges": {"sub_passes": (0, nq - 1), "resort": (0, nq)}}
        bad = seg_problems(m, where)
        if not bad:
            return to_fasta(refs), to_fasta(qrys), m, where
    raise AssertionError("the planted counts are not met: %r" % (bad[:4],))


def seg_problems(m, where):
    """the HITS (each a diagonal of its own and a record: tests/test_cand_order_inputs.py) are the planted numbers"""
    bad = []
    if not 32768 < len(m.refs) <= 65536 or max(len(q) for q in m.qrys) != 511 or len(m.qrys) - 1 < 256:
        bad.append("sizes")
    for q, n in where["ncand"].items():
        sid, pos, qp, drop = m.hits(q)
        if len(sid) != n or drop.any() or len(set(sid.tolist())) != n:
            bad.append(("hits", q, len(sid)))
    sid, pos, qp, drop = m.hits(where["b"])
    if len(set(qp.tolist())) != 1 or sid.max() >= 32767:
        bad.append("b")
    sid, pos, qp, drop = m.hits(where["a2"])
    if len(set(qp.tolist())) != SEG_NY + 1 or not (sid.min() < 32767 < sid.max()):
        bad.append("a2")
    sid, pos, qp, drop = m.hits(where["c"])
    if sorted(set(qp.tolist())) != [1, 511 - K]:
        bad.append("c")
    return bad


# ================================================================================================================
# the device-wide order in two sorts: ftbits + bq > 64
# ================================================================================================================
S2_SUBJECT, S2_QUERY, S2_FILL = (1 << 20) + 1, (1 << 18) + 1, 2048
S2_CANDS = 2052   # subjects of the big query (the slot the reference never reads may take one candidate away)


def sort2_bits(refs, qrys):
    """(bp, bs, bd, bsp, bq) of a pass that holds all of `qrys` against one chunk of `refs`, sequences numbered (no bands): host_seed.hip"""
    def clog2(x):
        return max(1, int(x - 1).bit_length())
    pmaxq, maxslen = max(len(q) for q in qrys), max(len(s) for s in refs)
    return clog2(max(pmaxq, 2)), clog2(len(refs)), clog2(pmaxq + maxslen + 1), clog2(maxslen + 1), clog2(len(qrys) + 1)


def sort2_set(oracle, seed=50514):
    """(reference fasta, query fasta, model, where).  where: "big" (the query of S2_CANDS - 1 candidates and more), "long" (the query of
    2^18 + 1 residues), "ncand" {query: candidates} of the two small queries, "range" (all queries)"""
    rng = np.random.default_rng(seed)
    pool = _strong_pieces(oracle, rng, 64 + 16 + 16)
    pc, pa, pb = pool[:64], pool[64:80], pool[80:]
    refs = [_subject([pc[t % 64]]) for t in range(S2_CANDS)] + [_subject([pa[3], pa[0]]), _subject([pb[5]])] + [np.full(S2_SUBJECT, ord("G"), dtype=np.uint8)]
    fill = np.frombuffer(b"PWPWPWPW", dtype=np.uint8)
    qrys = [_query(pa), _query(pc), _query(pb), np.frombuffer(b"PW" * (S2_QUERY // 2) + b"P", dtype=np.uint8)] + [fill] * S2_FILL
    where = {"small": (0, 2), "big": 1, "long": 3, "range": (0, len(qrys)), "ncand": {0: 1, 2: 1}}
    return to_fasta(refs), to_fasta(qrys), BucketModel(oracle, refs, qrys), where
