"""Inputs for tests/test_gpu_bucket_ungap.py: small protein sets whose diagonals are PLANTED on the edges of the bucketed seed pass
(k_bkt_group, then k_ungap1 for the singleton groups and the non-QSEG instance of k_ungap2 for the chains), and a plain numpy model of them.

Parameters of every set: seed 111111 over the 9-class alphabet, step 1, the frequency cap out of reach (thr); -F F wherever a designed
stretch is of low complexity.  The model is uqchain_inputs.ChainModel with the seed, the SEG switch and the chunk size as parameters
(BucketModel adds the counts the bucketed flow reports): a hit of query q is a pair (query window, index entry of the window's bucket), its
diagonal (subject, subject position - query position).  The offset-0 entry of a sequence is kept under the sequence in front of it at the
position behind its last residue (a hit that is never scored: the sentinel); that of a chunk's first sequence is dropped, as the library
drops it.  n_single() / n_chain() count the diagonals with one / with two and more KEPT hits: the groups k_ungap1 extends itself and the
heads it lists for k_ungap2.

Order inside a bucket.  A bucket is (query, 2^wb diagonal bands); its words are sorted by (band, diagonal id, query position), bands ascend
with the subjects, and the diagonal id of a hit is gbase - (sst - qpos) (k_encode_band32): it FALLS as sst - qpos rises.  No set relies on
that: every set reads the same in both directions or reaches its edge by a sweep, and the coverage is asserted for both.

Planting.  A pair of aligned residues is `same` (one class: part of a hit) or `cross` (two classes: never part of a hit); a 6-mer of `same`
pairs flanked by `cross` pairs is a diagonal of exactly one hit.  Cross pairs of every score -4 .. 0 are looked up in BLOSUM62
(_Cross), the positive ones are D/E, H/Y, W/Y (2) and K/E, Q/R, N/S (1); same-class pairs that score below zero are uqchain_inputs._NEG.
A stretch that must stay a singleton never holds six `same` pairs in a row.

What is NOT here, with the arithmetic:
  * X-drop offsets below 10 (right pass) and 7 (left pass): a pass loses at most 4 per pair (2 inside the seed, whose pairs are of one
    class), so 30 points are lost after 6 seed pairs + 5 more at the earliest going right (12 + 4 * 4 + 2) and after 8 pairs going left
    (7 * 4 + 2).  Every element k = 0 .. 15 of a step, the lone 16th included, is reached in the second and third step (offsets 16 .. 47).
  * The three query-slot instances of k_ungap1 cannot be told apart by a counter: groups_single / groups_chain exist only with
    SOHIT_UG_COUNT=1, and the counting instance is always the U1_QCAP one (launch_ungap1).  The slot set is therefore searched twice: with
    the counters (the flow and the extents) and without them (the 512 / 1024 / U1_QCAP instances by pmaxq: rows and candidates).
    seed_stage puts the lengths < 512, 512 .. 1023, 1024 .. 2047, 2048 .. 4095 into passes of their own (query_class), and the slot is
    chosen by the pass's LONGEST query: 512 and 513 (1024 and 1025, 2048 and 2049) have to be searched in different query ranges.
  * Bucket totals of 64 n and 64 n + 1 cannot both come from the sweep (its totals all have one parity: k singletons at either end):
    two more queries of the scan set bring them.
And what IS here although it looked doubtful -- list pieces: reachable under BG_CAP = 4096 hits with a 2048-residue query.  250 pieces of
7 residues (8 with the separator: 2000 residues) found in each of five subjects are some 1250 chain heads in 2500 hits (> U1_LCHUNK - 64
= 960), 290 pieces of 6 residues in three subjects some 870 passing singletons (> U1_CHUNK = 512): list_set.

One more rule of the index that the model needed for exact counts: the reference never reads the last slot of a chunk's index, so the
smallest entry of the chunk's highest bucket is no hit for anybody (uqchain_inputs.ChainModel drops it, as the library does)."""
import numpy as np

import uqchain_inputs as ci
from uqchain_inputs import AA, HT, DSH, ChainModel, _NEG, _host, _iid, _plant, to_fasta  # noqa: F401

SEED = "111111"
K = 6
BG_CAP = 4096      # k_bucket.hip: #define BG_CAP (no accessor in the library)
BG_BINS = 1024     # k_bucket.hip: #define BG_BINS
U1_QCAP = 2048     # kernels.h
CLASSES = "AST,CFILMVY,DN,EQ,G,H,KR,P,W"
CLS = np.zeros(256, dtype=np.int64)
for _i, _g in enumerate(CLASSES.split(",")):
    for _c in _g:
        CLS[ord(_c)] = _i
XP = {ord(a): ord(b) for a, b in zip("DEHYWKQRNS", "EDYHYERQSN")}   # residue -> a residue of ANOTHER class that scores above zero against it
AA18 = np.frombuffer(b"ACDEFHIKLMNQRSTVWY", dtype=np.uint8)     # no G, no P: the separators of the piece queries
AA10 = np.frombuffer(b"DEHYWKQRNS", dtype=np.uint8)             # the residues that have a partner in XP
_B62 = {}


def b62(oracle, a, b):
    if not _B62:
        assert oracle.AA9 == CLASSES
        for x in AA:
            for y in AA:
                _B62[(int(x), int(y))] = oracle.b62(int(x), int(y))
    return _B62[(int(a), int(b))]


class _Cross:
    """X(v): a (query residue, subject residue) of two classes that scores v, drawn so that neither side repeats the class of the pair
    drawn before: a stretch of such pairs holds no run of one class on either side (runs meet each other all over a set)"""

    def __init__(self, oracle, rng):
        b62(oracle, AA[0], AA[0])
        self.rng, self.last = rng, (-1, -1)

    def __call__(self, v):
        c = [xy for xy, s in sorted(_B62.items()) if s == v and CLS[xy[0]] != CLS[xy[1]] and CLS[xy[0]] != self.last[0] and CLS[xy[1]] != self.last[1]]
        x, y = c[int(self.rng.integers(0, len(c)))]
        self.last = (CLS[x], CLS[y])
        return x, y


class BucketModel(ChainModel):
    """ChainModel for the seed 111111, with what the bucketed flow counts"""

    def __init__(self, oracle, refs, qrys=None, flt=False, chk=None):
        ChainModel.__init__(self, oracle, refs, qrys, ssd=SEED, flt=flt, chk=chk)
        self._k = {}

    def kept(self, q):
        """(keys, sizes) of query q's diagonals without the dropped entries"""
        if q not in self._k:
            sid, pos, qp, drop = self.hits(q)
            key = ((sid << DSH) | (pos - qp + (1 << (DSH - 1))))[~drop]
            self._k[q] = np.unique(key, return_counts=True)
        return self._k[q]

    def _range(self, qs):
        return range(len(self.qrys)) if qs is None else qs

    def n_single(self, qs=None):
        return int(sum(int((self.kept(q)[1] == 1).sum()) for q in self._range(qs)))

    def n_chain(self, qs=None):
        return int(sum(int((self.kept(q)[1] >= 2).sum()) for q in self._range(qs)))

    def n_hits(self, qs=None):
        """all hits, the dropped ones included (so_counters.seed_hits)"""
        return int(sum(len(self.hits(q)[0]) for q in self._range(qs)))

    def hits_on(self, q, s):
        """{diagonal: kept hits} of query q on subject s"""
        u, c = self.kept(q)
        m = (u >> DSH) == s
        return {int(k & ((1 << DSH) - 1)) - (1 << (DSH - 1)): int(n) for k, n in zip(u[m], c[m])}

    def qpos_on(self, q, s, d):
        """query positions of the hits of query q on diagonal d of subject s, ascending"""
        sid, pos, qp, drop = self.hits(q)
        return sorted(int(x) for x in qp[(sid == s) & (pos - qp == d) & ~drop])

    def sizes_along(self, q, subjects, reverse=False):
        """group sizes in bucket order: the subjects in the order given (reverse: the whole sequence backwards), the diagonals of one
        subject by sst - qpos"""
        out = []
        for s in subjects:
            h = self.hits_on(q, s)
            out += [h[d] for d in sorted(h)]
        return out[::-1] if reverse else out


def word_offsets(sizes):
    """(singletons, heads, lasts, total): the word positions inside the bucket of the groups of one hit, of the first and of the last word
    of the longer groups"""
    at = np.cumsum([0] + list(sizes))
    n = np.asarray(sizes)
    return at[:-1][n == 1], at[:-1][n >= 2], (at[1:] - 1)[n >= 2], int(at[-1])


def _assemble(rng, pairs, pre_q, pre_s, tail=20):
    q = np.concatenate([_iid(rng, pre_q), np.array([p[0] for p in pairs], dtype=np.uint8), _iid(rng, tail)])
    s = np.concatenate([_iid(rng, pre_s), np.array([p[1] for p in pairs], dtype=np.uint8), _iid(rng, tail)])
    return q, s


def _ident(rng, n):
    return [(int(a), int(a)) for a in _iid(rng, n)]


def _neg(rng, n):
    return [(int(a), _NEG[int(a)]) for a in np.frombuffer(b"CFIYLMV", dtype=np.uint8)[rng.integers(0, 7, size=n)]]


def _neg2(rng, n):
    """pairs of one class that score -2 each"""
    return [(ord(a), ord(b)) for a, b in (("CF", "FC", "YC")[int(i)] for i in rng.integers(0, 3, size=n))]


def _score(oracle, pairs):
    return sum(b62(oracle, a, b) for a, b in pairs)


# ================================================================================================================
# X-drop: 30 / 31 below the maximum at every reachable element offset, both directions
# ================================================================================================================
def _drop_run(n, d):
    """n scores of -4 .. 0 that sum to -d; the zeros first, the remainder LAST: the running sum reaches -d at the n-th element and not before"""
    v = [-4] * (d // 4) + ([-(d % 4)] if d % 4 else [])
    assert len(v) <= n, (n, d)
    return [0] * (n - len(v)) + v


XDROP_RIGHT_MIN, XDROP_LEFT_MIN = 10, 7


def _xdrop_pairs(oracle, rng, o, d, left):
    """(pairs, seed's index, group score, b62 lookups): the running score of the pass falls d below its maximum at element o, then W/W W/W
    D/E W/W W/W W/W (+57); eight pairs of -4 end every pass"""
    X = _Cross(oracle, rng)
    stop = [X(-4) for _ in range(8)]
    w = (ord("W"), ord("W"))
    rec = [w, w, (ord("D"), ord("E")), w, w, w]
    goes_on = d <= 30
    if left:
        seed = _ident(rng, K)
        ext = [X(v) for v in _drop_run(o + 1, d)] + rec + stop   # (going left from the seed)
        pairs = ext[::-1] + seed + stop
        base = _score(oracle, seed)
        return pairs, len(ext), base + (27 if goes_on else 0), (K + 8) + (o + 1 + (len(rec) + 8 if goes_on else 0))
    positive = o >= 14
    seed = _ident(rng, K) if positive else _neg2(rng, K)
    run = [X(v) for v in _drop_run(o - 5, d + (0 if positive else _score(oracle, seed)))]
    pairs = stop + seed + run + rec + stop
    base = _score(oracle, seed) if positive else 0
    return pairs, 8, base + (27 if goes_on else 0), 8 + (o + 1 + (len(rec) + 8 if goes_on else 0))


def xdrop_set(oracle, seed=40411):
    """(fasta, model, cases): all-vs-all, -F F; cases = (query, subject, Qst, Sst, left, o, d, score, lookups), a 30-drop and its
    31-twin per direction and offset; the twin of a case is the next one"""
    rng = np.random.default_rng(seed)
    for _ in range(32):
        seqs, cases = [], []
        for left in (False, True):
            for o in range(XDROP_LEFT_MIN if left else XDROP_RIGHT_MIN, 48):
                sd = int(rng.integers(1 << 30))   # (the twin has the same seed residues)
                for d in (30, 31):
                    pairs, at, score, flag = _xdrop_pairs(oracle, np.random.default_rng(sd), o, d, left)
                    pq, ps = int(rng.integers(10, 30)), int(rng.integers(10, 30))
                    q, s = _assemble(rng, pairs, pq, ps)
                    seqs += [q, s]
                    cases.append((len(seqs) - 2, len(seqs) - 1, pq + at, ps + at, left, o, d, score, flag))
        m = BucketModel(oracle, seqs)
        bad = xdrop_problems(oracle, m, cases)
        if not bad:
            return to_fasta(seqs), m, cases
    raise AssertionError("the planted cases keep meeting chance matches: %r" % (bad[:4],))


def xdrop_problems(oracle, m, cases):
    bad = []
    for q, s, qst, sst, left, o, d, score, flag in cases:
        if m.hits_on(q, s).get(sst - qst) != 1:
            bad.append(("singleton", left, o, d))
        u = oracle.ungap(m.refs[q].tobytes(), m.refs[s].tobytes(), qst, sst)
        if (u[0], u[5]) != (score, flag):
            bad.append(("oracle", left, o, d, u, score, flag))
    for a, b in zip(cases[0::2], cases[1::2]):   # the pair differs as designed: 27 points and the 14 lookups behind the drop
        if (a[6], b[6]) != (30, 31) or a[7] - b[7] != 27 or a[8] - b[8] != 14:
            bad.append(("pair", a[4], a[5]))
    return bad


# ================================================================================================================
# slot instances, query ends, long singleton passes, ends of the subject array
# ================================================================================================================
SLOT_LENGTHS = (512, 513, 1024, 1025, 2048, 2049)


def _partner(sub, L, left):
    """a query of L residues whose ONLY hit with `sub` (L residues of a subject over AA10) is one window -- its last one (left) or the one at
    position 1 -- and whose every other residue up to the far end scores above zero: five pairs of one residue, then one XP pair"""
    q = sub.copy()
    for i in range(L):
        e = (L - 1 - i) if left else (i - 1)   # distance from the seed's near end
        if e >= K and (e - K) % 6 == 0:
            q[i] = XP[int(sub[i])]
    q[0] = ord("G")   # (position 0 is never scored; AA10 has no G)
    return q


def slot_set(oracle, seed=40412, n_back=150, c0=100):
    """(reference fasta, query fasta, model, where), -F F.  where:
      ranges     {name: (first query, behind the last)}: the query ranges to search on their own -- "even" (a 6-, a 7-residue query, short ones
                 and the queries of 512, 1024 and 2048 residues; the batch's last query is of 2048), "odd" (513, 1025), "over" (2049: k_ungap)
      long       {(L, left): (query, subject, Qst, Sst, score)}: a singleton whose extension spans the whole query -- left: the seed is the query's
                 last window and the last window of the reference's LAST sequence, the pass runs down to position 1; else: the seed sits at
                 position 1 of the query and of the reference's FIRST sequence, the pass runs up to the last residue
      wrich      the same (left) for 2048 residues of W W W W W H against W W W W W Y
      q6, q7     queries of one and of two windows; q7 is the head of subject `mid`: its window 0 meets the offset-0 entry, kept under the
                 subject in front at the position behind its last residue
      qc         the same with subject c0: the first sequence of the second chunk at chk = c0 (dropped there)
      tiny       (query, subject, diagonal): a subject of 12 residues that holds a group of two hits"""
    rng = np.random.default_rng(seed)
    for _ in range(32):
        first, last = AA10[rng.integers(0, 10, size=2100)], AA10[rng.integers(0, 10, size=2100)]
        refs = [first] + [_iid(rng, int(rng.integers(60, 161))) for _ in range(n_back)]
        mid = 40
        body = np.full(2048, ord("W"), dtype=np.uint8)
        qw = body.copy()
        for i in range(2048):
            e = 2047 - i
            if e >= K and (e - K) % 6 == 0:
                body[i], qw[i] = ord("H"), ord("Y")
        qw[0] = ord("G")
        refs.append(np.concatenate([_iid(rng, 30), body]))
        sw = len(refs) - 1
        qt = _iid(rng, 60)
        refs.append(_host(rng, qt, 20, K + 1, 12, 3))
        tiny = len(refs) - 1
        refs.append(last)
        qrys, where = [], {"ranges": {}, "long": {}, "mid": mid, "c0": c0}

        def add(s):
            qrys.append(s)
            return len(qrys) - 1

        def longs(lengths):
            for L in lengths:
                where["long"][(L, False)] = (add(_partner(first[:L], L, False)), 0, 1, 1)
                where["long"][(L, True)] = (add(_partner(last[2100 - L:], L, True)), len(refs) - 1, L - K, 2100 - K)

        longs((513, 1025))
        where["ranges"]["odd"] = (0, len(qrys))
        longs((2049,))
        where["ranges"]["over"] = (where["ranges"]["odd"][1], len(qrys))
        where["q6"] = add(refs[5][20:20 + K].copy())
        where["q7"] = add(refs[mid][:K + 1].copy())
        where["qc"] = add(refs[c0][:K + 1].copy())
        where["tiny"] = (add(qt), tiny, 3 - 20)
        longs((512, 1024))
        where["wrich"] = (add(qw), sw, 2048 - K, 30 + 2048 - K)
        longs((2048,))
        where["ranges"]["even"] = (where["ranges"]["over"][1], len(qrys))
        m = BucketModel(oracle, refs, qrys)
        bad = slot_problems(oracle, m, where)
        if not bad:
            return to_fasta(refs), to_fasta(qrys), m, where
    raise AssertionError("the planted cases keep meeting chance matches: %r" % (bad[:4],))


def _long_cases(where):
    return list(where["long"].items()) + [((2048, "w"), where["wrich"])]


def slot_problems(oracle, m, where):
    bad = []
    for (L, left), (q, s, qst, sst) in _long_cases(where):
        qs, ss = m.qrys[q].tobytes(), m.refs[s].tobytes()
        if len(qs) != L or m.hits_on(q, s).get(sst - qst) != 1:
            bad.append(("singleton", L, left))
        u = oracle.ungap(qs, ss, qst, sst)
        want = sum(b62(oracle, qs[i], ss[i + sst - qst]) for i in range(1, L))
        # every residue but position 0 is scored once, all of them above zero: the maximum is the pass's last residue
        if u[0] != want or u[5] != L - 1 or (u[1] if left else u[2]) != (1 if left else L - 1):
            bad.append(("oracle", L, left, u, want))
    q, s, qst, sst = where["wrich"]
    sc = oracle.ungap(m.qrys[q].tobytes(), m.refs[s].tobytes(), qst, sst)[0]
    if not 19000 <= sc < (1 << 15) - 8192:   # (kernels.h at U1_QCAP: the packed score and the pin's 8192 stay below 2^15)
        bad.append(("wrich", sc))
    if len(m.hits(where["q6"])[0]) < 1 or len(m.qrys[where["q6"]]) != K or len(m.qrys[where["q7"]]) != K + 1:
        bad.append("q6")
    for name, j in (("q7", where["mid"]), ("qc", where["c0"])):   # window 0: behind the last residue of the subject in front; window 1: position 1
        h = m.hits_on(where[name], j - 1)
        if h.get(len(m.refs[j - 1])) != 1 or m.hits_on(where[name], j).get(0) != 1:
            bad.append(name)
    q, s, d = where["tiny"]
    if len(m.refs[s]) >= 16 or m.hits_on(q, s) != {d: 2}:
        bad.append("tiny")
    lo, hi = where["ranges"]["even"]
    if hi != len(m.qrys) or len(m.qrys[hi - 1]) != 2048 or sorted(set(len(m.qrys[q]) for q in range(lo, hi)) & set(SLOT_LENGTHS)) != [512, 1024, 2048]:
        bad.append("ranges")
    return bad


# ================================================================================================================
# scan edges: every group on every word offset of the 64-word scan
# ================================================================================================================
def _scan_query(S, khi, klo):
    """'G' + pieces of S, a 'G' behind each: khi singletons on the highest diagonals, the base (singletons next to groups of 2, 3 and 65
    hits), klo singletons on the lowest diagonals"""
    out, pos = [np.frombuffer(b"G", dtype=np.uint8)], 1
    for j in range(khi):   # (the first one: the subject's last window at the query's first -- no diagonal lies above it)
        out += [S[len(S) - K - 9 * j:len(S) - 9 * j], out[0]]
        pos += K + 1
    for i, n in enumerate((1, 2, 1, 3, 1, 65, 1)):
        sst = pos + 500 + 10 * i
        out += [S[sst:sst + n + K - 1], out[0]]
        pos += n + K
    for j in range(klo - 1, -1, -1):   # (the last one: the subject's position 1 at the query's last window -- none lies below)
        out += [S[1 + 5 * j:1 + 5 * j + K], out[0]]
        pos += K + 1
    return np.concatenate(out)


def scan_set(oracle, seed=40413):
    """(reference fasta, query fasta, model): -F F.  The reference is ONE subject of 1600 residues (no G, no P) and a second one of the same
    length, G P G P ..., that no query window meets: alone in its chunk the subject would be cut into two diagonal bands (band_plan takes the
    narrower diagonal field whenever that saves a key bit; with two subjects of one length it saves none), and two bands may be two
    buckets.  Queries 0 .. 63: query k = the base and k more singleton diagonals at BOTH extremes; queries 64, 65: bucket totals of 64 n and
    64 n + 1 with a singleton as the first and as the last word."""
    rng = np.random.default_rng(seed)
    for _ in range(32):
        S = AA18[rng.integers(0, 18, size=1600)]
        refs = [S, np.frombuffer(b"GP" * 800, dtype=np.uint8)]
        qrys = [_scan_query(S, k, k) for k in range(64)]
        cand = [_scan_query(S, 1, a) for a in range(1, 66)]   # (the extra pieces bring chance hits of their own: take the totals from the model)
        mc = BucketModel(oracle, refs, cand)
        tot = [sum(mc.hits_on(a, 0).values()) % 64 for a in range(65)]
        if 0 not in tot or 1 not in tot:
            continue
        qrys += [cand[tot.index(0)], cand[tot.index(1)]]
        m = BucketModel(oracle, refs, qrys)
        bad = scan_problems(m)
        if not bad:
            return to_fasta(refs), to_fasta(qrys), m
    raise AssertionError("the planted cases keep meeting chance matches: %r" % (bad[:4],))


def scan_problems(m):
    bad = []
    if len(m.qrys) != 66 or any(m.hits_on(q, 1) for q in range(66)):
        bad.append("second subject")
    for rev in (False, True):
        seen = {"single": set(), "head": set(), "last": set()}
        for q in range(64):
            sizes = m.sizes_along(q, [0], rev)
            h = m.hits_on(q, 0)
            # the base: diagonals 500, 510 ... 560 (chance groups are swept like the planted ones)
            if [h.get(d) for d in range(500, 561, 10)] != [1, 2, 1, 3, 1, 65, 1] or (q and (sizes[0] != 1 or sizes[-1] != 1)):
                bad.append(("base", q))
            s1, hd, la, tot = word_offsets(sizes)
            seen["single"] |= set(int(x) % 64 for x in s1)
            seen["head"] |= set(int(x) % 64 for x in hd)
            seen["last"] |= set(int(x) % 64 for x in la)
        for k, v in seen.items():
            if not {0, 63} <= v:   # the first and the last word of a scan
                bad.append((k, rev))
        for q, r in ((64, 0), (65, 1)):
            sizes = m.sizes_along(q, [0], rev)
            if sum(sizes) % 64 != r or sizes[0] != 1 or sizes[-1] != 1:
                bad.append(("total", q, sum(sizes)))
    return bad


# ================================================================================================================
# chains (k_ungap2): where the first segment's maximum lies, ties, covered and bounded seeds, group sizes
# ================================================================================================================
def _cover_pairs(oracle, rng, m, gap=0, tie=False, zero=False):
    """(pairs, seed's index, r1 = offset of the first segment's maximum): eight pairs of -4, the first segment (zero: six pairs of one class
    that score below zero -- nothing positive, the maximum stays at the seed; else m + 1 identical residues, filled up to the seed's six
    with pairs of one class that score below zero), tie: a pair of -1 and one of +1 (the maximum again, two residues on), `gap` pairs
    of 0, six pairs of one class that score below zero (a seed hit that adds nothing), eight pairs of -4"""
    X = _Cross(oracle, rng)
    stop = [X(-4) for _ in range(8)]
    first = _neg(rng, K) if zero else _ident(rng, m + 1) + _neg(rng, max(0, K - m - 1))
    mid = ([X(-1), (ord("K"), ord("E"))] if tie else []) + [X(0) for _ in range(gap)]
    return stop + first + mid + _neg(rng, K) + stop, 8, 0 if zero else m


def chain_set(oracle, seed=40414, n_back=120):
    """(fasta, model, where): all-vs-all, -F F.  where:
      pair, triple, g64, g65   (query, host, diagonal): groups of exactly 2, 3, 64 and 65 hits
      copies                   four copies of one 250-residue protein: groups of 244 and 245 hits, four per query
      neighbours, repeat       neighbouring diagonals; two groups on one subject
      cover                    {name: (query, host, Qst, Sst, r1, next, tie)}: the first segment's maximum r1 residues behind its seed, the next
                               seed that runs at `next` -- names ("max", m) for m = 0 .. 47, "zero", ("tie", m) for m = 19 (both in one group of
                               three elements), 20 (two groups), 30 and 15 (two steps), ("gap", g) for g = 0 .. 16 and 20 with m = 20,
                               and ("len", L): the ("gap", 5) shape in a query of L = 512, 1024, 2048 residues"""
    rng = np.random.default_rng(seed)
    for _ in range(32):
        seqs = [_iid(rng, int(rng.integers(40, 121))) for _ in range(n_back)]
        where = {"cover": {}}

        def add(s):
            seqs.append(s)
            return len(seqs) - 1

        for name, n in (("pair", 2), ("triple", 3), ("g64", 64), ("g65", 65)):
            ln = n + K - 1
            q = _iid(rng, ln + 60)
            qi = add(q)
            where[name] = (qi, add(_host(rng, q, 25, ln, ln + 50, 10)), 10 - 25)
        big = _iid(rng, 250)
        where["copies"] = [add(big.copy()) for _ in range(4)]
        q, h = _iid(rng, 120), _iid(rng, 140)
        _plant(h, 40, q, 20, K + 1)   # diagonal 20
        _plant(h, 71, q, 50, K + 1)   # diagonal 21
        where["neighbours"] = (add(q), add(h), 20)
        q, h = _iid(rng, 100), _iid(rng, 150)
        _plant(h, 15, q, 30, K + 1)
        _plant(h, 90, q, 30, K + 1)
        where["repeat"] = (add(q), add(h), -15, 60)
        shapes = [(("max", m), dict(m=m)) for m in range(48)] + [("zero", dict(m=0, zero=True))] + \
                 [(("tie", m), dict(m=m, tie=True)) for m in (19, 20, 30, 15)] + [(("gap", g), dict(m=20, gap=g)) for g in list(range(17)) + [20]] + \
                 [(("len", L), dict(m=20, gap=5)) for L in (512, 1024, 2048)]
        for name, kw in shapes:
            pairs, at, r1 = _cover_pairs(oracle, rng, **kw)
            pq, ps = int(rng.integers(10, 40)), int(rng.integers(10, 40))
            q, s = _assemble(rng, pairs, pq, ps, tail=(name[1] - pq - len(pairs)) if name[0] == "len" else 20)
            s = s[:ps + len(pairs) + 20]
            nxt = pq + at + max(kw["m"] + 1, K) + (2 if kw.get("tie") else 0) + kw.get("gap", 0)
            if kw.get("zero") or kw["m"] < K - 1:
                nxt = pq + at + r1 + 1   # (the residues behind the maximum are of one class: the next window starts at once)
            where["cover"][name] = (add(q), add(s), pq + at, ps + at, r1, nxt, bool(kw.get("tie")))
        m = BucketModel(oracle, seqs)
        bad = chain_problems(oracle, m, where)
        if not bad:
            return to_fasta(seqs), m, where
    raise AssertionError("the planted cases keep meeting chance matches: %r" % (bad[:4],))


def chain_problems(oracle, m, where):
    bad = []
    for name, n in (("pair", 2), ("triple", 3), ("g64", 64), ("g65", 65)):
        q, h, d = where[name]
        if m.hits_on(q, h).get(d) != n:
            bad.append(name)
    for q in where["copies"]:
        if any(m.hits_on(q, s).get(0) not in (244, 245) for s in where["copies"]):   # (a copy's offset-0 entry sits under the sequence in front)
            bad.append("copies")
    q, h, d = where["neighbours"]
    if (m.hits_on(q, h).get(d), m.hits_on(q, h).get(d + 1)) != (2, 2):
        bad.append("neighbours")
    q, h, d0, d1 = where["repeat"]
    if (m.hits_on(q, h).get(d0), m.hits_on(q, h).get(d1)) != (2, 2):
        bad.append("repeat")
    ninv = set()
    for name, (q, h, qst, sst, r1, nxt, tie) in where["cover"].items():
        qs, hs = m.refs[q].tobytes(), m.refs[h].tobytes()
        d = sst - qst
        locs = m.qpos_on(q, h, d)
        if len(locs) < 2 or locs[0] != qst or nxt not in locs or any(qst + r1 < p < nxt for p in locs):
            bad.append((name, "hits", locs[:4], qst, nxt))
            continue
        first = oracle.ungap(qs, hs, qst, sst)
        if first[2] != qst + r1:   # max_qed: the FIRST position of the maximum
            bad.append((name, "max_qed", first[2] - qst))
        # the seed behind it: bounded on the left by the maximum's position; a tie leaves it the +1 pair behind the first maximum
        bounded = oracle.ungap(qs, hs, nxt, nxt + d, qst + r1, qst + r1 + d)
        if bounded[0] != (1 if tie else 0):
            bad.append((name, "bounded", bounded))
        if r1 >= K - 1 and oracle.ungap(qs, hs, nxt, nxt + d)[0] <= bounded[0]:   # unbounded it climbs the first segment
            bad.append((name, "unbounded"))
        chain = oracle.ungap_chain(qs, hs, [(p, p + d) for p in locs])
        if chain[0] != first[0] + bounded[0]:
            bad.append((name, "chain", chain[0], first[0]))
        if isinstance(name, tuple) and name[0] == "gap":
            ninv.add(min(max(qst + r1 + 1 - (nxt - 16), 0), 16))   # masked bytes of the next seed's first left window
    if ninv != set(range(17)):
        bad.append(("ninv", sorted(ninv)))
    for L in (512, 1024, 2048):
        if len(m.refs[where["cover"][("len", L)][0]]) != L:
            bad.append(("len", L))
    # no query of the large pass brings more than BG_CAP hits: its bucket is sorted in one piece whatever the range width
    if max(m.n_hits([q]) for q in range(len(m.refs)) if len(m.refs[q]) < 512) > BG_CAP:
        bad.append("BG_CAP")
    return bad


# ================================================================================================================
# many lanes at once, the ring, k_bkt_group's segments, more than BG_BINS sequences
# ================================================================================================================
def _strong_pieces(oracle, rng, n):
    """n 6-mers over AA18, no two of one class string, each scoring MIN_UNGAP = 25 and more against itself"""
    out, seen = [], set()
    while len(out) < n:
        p = AA18[rng.integers(0, 18, size=K)]
        key = CLS[p].tobytes()
        if key not in seen and sum(b62(oracle, a, a) for a in p) >= 25:
            seen.add(key), out.append(p)
    return out


def _join(pieces, sep):
    s = np.frombuffer(sep, dtype=np.uint8)
    return np.concatenate([s] + [x for p in pieces for x in (p, s)])


LANES_SEGMENTS = (1, 2, 16, 17, 64, 65)


def lanes_set(oracle, seed=40415, n_ref=1100):
    """(reference fasta, query fasta, model, where): -F F.  Subjects 0 .. 64 and 66 .. 130 are G + a 6-mer + G + a 6-mer (two singletons; the
    second one's right pass ends behind six residues at the subject's end, its left pass at the subject's position 0 at the latest: both
    inside ONE step); subject 65 is G + a 7-mer (a group of two hits); subjects 131 .. 136 are G + 1, 2, 16, 17, 64 and 65 6-mers with a G behind each; the rest, up to n_ref >
    BG_BINS sequences, are G + a 6-mer.  All designed subjects have ids below 256: one bucket per query whatever range width the pass takes
    down to wb = 8 (31 - 12 diagonal bits - 11 position bits).  Queries (pieces with a P behind each):
      burst     the second 6-mers of 70 subjects: 70 singletons that reach MIN_UNGAP and finish in the same step
      ring      all 260 6-mers and the 7-mer: 130 singletons on either side of the bucket's only longer group
      segments  the 6-mers of subjects 131 .. 136 in shuffled order: per-subject segments of 1, 2, 16, 17, 64 and 65 hits in one bucket"""
    rng = np.random.default_rng(seed)
    for _ in range(32):
        pc = _strong_pieces(oracle, rng, 261 + (n_ref - 137) + sum(LANES_SEGMENTS))
        up, pc = pc[-sum(LANES_SEGMENTS):], pc[:-sum(LANES_SEGMENTS)]
        g = np.frombuffer(b"G", dtype=np.uint8)
        two = [np.concatenate([g, pc[2 * i], g, pc[2 * i + 1]]) for i in range(130)]
        seven = np.concatenate([pc[260], AA18[rng.integers(0, 18, size=1)]])
        refs = two[:65] + [np.concatenate([g, seven])] + two[65:]
        at = np.cumsum((0,) + LANES_SEGMENTS)
        U = [_join(up[a:b], b"G") for a, b in zip(at[:-1], at[1:])]
        refs += U
        refs += [np.concatenate([g, p]) for p in pc[261:]]
        # (ring: a subject's two 6-mers far apart, or they would share a diagonal)
        qrys = [_join([pc[2 * i + 1] for i in range(70)], b"P"), _join(pc[0:260:2] + [seven] + pc[1:260:2], b"P"),
                _join([up[i] for i in rng.permutation(len(up))], b"P")]
        m = BucketModel(oracle, refs, qrys)
        where = {"burst": 0, "ring": 1, "segments": 2, "U": list(range(131, 137))}
        bad = lanes_problems(oracle, m, where)
        if not bad:
            return to_fasta(refs), to_fasta(qrys), m, where
    raise AssertionError("the planted cases keep meeting chance matches: %r" % (bad[:4],))


def lanes_problems(oracle, m, where):
    bad = []
    if len(m.refs) <= BG_BINS or max(len(q) for q in m.qrys) > U1_QCAP:
        bad.append("sizes")
    sizes = m.sizes_along(where["burst"], range(256))
    if len(sizes) < 70 or set(sizes) != {1}:
        bad.append(("burst", len(sizes)))
    for rev in (False, True):
        sizes = m.sizes_along(where["ring"], range(256), rev)
        if [n for n in sizes if n > 1] != [2] or sizes.index(2) <= 128:
            bad.append(("ring", rev))
    got = [sum(m.hits_on(where["segments"], s).values()) for s in where["U"]]
    if got != list(LANES_SEGMENTS):
        bad.append(("segments", got))
    return bad


# ================================================================================================================
# list pieces: more chain heads / passing singletons in one bucket than a wave's reserved piece holds
# ================================================================================================================
def list_set(oracle, seed=40416):
    """(reference fasta, query fasta, model): -F F.  Query 0: 250 pieces of 7 residues, each in five subjects (in shuffled order: other
    diagonals) -- some 1250 chain heads in one bucket, more than U1_LCHUNK - 64 = 960; query 1: 290 6-mers that score MIN_UNGAP and more,
    each in three subjects -- some 870 passing singletons, more than U1_CHUNK = 512.  Eight subjects in all, 2500 hits per bucket and a few
    chance hits (< BG_CAP)."""
    rng = np.random.default_rng(seed)
    for _ in range(32):
        p7 = [np.concatenate([p, AA18[rng.integers(0, 18, size=1)]]) for p in _strong_pieces(oracle, rng, 250)]
        p6 = _strong_pieces(oracle, rng, 290)
        def sub(pc):   # (one to three G between two pieces: few pieces share a diagonal)
            g = np.frombuffer(b"GGG", dtype=np.uint8)
            return np.concatenate([g[:1]] + [x for i in rng.permutation(len(pc)) for x in (pc[i], g[:int(rng.integers(1, 4))])])

        refs = [sub(p7) for _ in range(5)] + [sub(p6) for _ in range(3)]
        qrys = [_join(p7, b"P"), _join(p6, b"P")]
        m = BucketModel(oracle, refs, qrys)
        bad = list_problems(m)
        if not bad:
            return to_fasta(refs), to_fasta(qrys), m
    raise AssertionError("the planted cases keep meeting chance matches: %r" % (bad[:4],))


def list_problems(m):
    bad = []
    if max(len(q) for q in m.qrys) > U1_QCAP or max(m.n_hits([q]) for q in (0, 1)) >= BG_CAP:
        bad.append("sizes")
    if m.n_chain([0]) <= 1024 - 64:
        bad.append(("heads", m.n_chain([0])))
    if m.n_single([1]) <= 512:
        bad.append(("singles", m.n_single([1])))
    return bad


# ================================================================================================================
# a bucket of BG_CAP - 1, BG_CAP and BG_CAP + 1 hits
# ================================================================================================================
def cap_set(oracle, target, seed=40417, unit=310):
    """(fasta, model, queries): all-vs-all, -F T; copies of one iid protein of `unit` residues and one partial copy, the _family way, and
    nothing else: with one subject range per chunk (SOHIT_BUCKET_AVG=100000) a copy's bucket holds ALL its hits, `target` of them for the
    queries listed (the protein's chance hits with itself are counted, the partial copy's length is chosen for the rest)"""
    rng = np.random.default_rng(seed + target)
    for _ in range(32):
        p = _iid(rng, unit)
        own = BucketModel(oracle, [p], flt=True)
        per = own.n_hits() - int(own.hits(0)[3].sum())   # kept hits of the protein with one copy of itself
        k = target // per
        for ln in range(K + 2, unit):
            seqs = [p.copy() for _ in range(k)] + [np.concatenate([_iid(rng, 1), p[:ln]])]
            m = BucketModel(oracle, seqs, flt=True)
            n = int((~m.hits(1)[3]).sum())
            if n >= target:
                break
        if n == target:
            return to_fasta(seqs), m, [q for q in range(1, k) if int((~m.hits(q)[3]).sum()) == target]
    raise AssertionError("no family of %d hits" % target)


def band_set(oracle):
    """(reference fasta, query fasta, model): uqchain_inputs.band_set for this seed -- 260 queries of 60 .. 200 residues against themselves
    and one subject of 6000 residues that holds a 40-residue segment (a group of 35 hits) of every fourth query.  band_plan for queries
    below 2^8 residues: every subject in one band needs 13 diagonal bits and 9 band bits (22); 9 diagonal bits leave the short subjects
    (<= 2^9 - 2^8 residues) one band each and cut the long one into (6000 + 256 + 511) >> 9 = 13: 273 bands, 9 + 9 = 18 bits -- the narrower
    layout wins, some subject owns several bands, and the pass resolves bands through `btab` (the BANDS instances of every kernel)."""
    ref, qry, m = ci.band_set(oracle, ssd=SEED)
    return ref, qry, BucketModel(oracle, m.refs, m.qrys, flt=True)
