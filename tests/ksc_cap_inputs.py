"""Inputs for tests/test_gpu_ksc_cap.py: protein sets whose queries stand on the edges of the FREQUENCY CAP -- k_cap_all, k_cap, the k-mer
order kernels k_ksc_order_lds<512|1024|4096> / k_ksc_order_g and the choice among them in chunk_qhits / chunk_qhits_deferred -- and plain
models of that stage.

The stage (fsearch.py:2647-2677).  A query of `len` residues has nk = len - mink + 1 windows (mink: the shortest seed span).  Window i has a
self score ksc[i] (BLOSUM62 of its mink residues against themselves, on the MASKED query) and a count cnt[i]: the index entries of its
buckets in the chunk at hand, summed over seed patterns and alphabets.  The windows are walked in the order of the reference's unstable
quicksort of -ksc (oracle.qsort_perm) and rank r is taken iff the total of the ranks in front of it is <= limit = threshold * len (the test
precedes the add): a prefix of the order (cap_marks, the definition the kernels implement).  A query's WORK in a chunk is the sum of cnt
over its taken windows, its work the sum over the chunks: Searcher.query_work().  The threshold is `thr` when thr >= 1 or the chunk's own
is 0.  The reference figure comes from the oracle (oracle_work: find_msav_m on every chunk's oracle.Index, tuples counted); the model here
(model_of / cap_marks) restates it in numpy and carries the WRONG variants (variant_work) that say what a set can tell apart.

A sum says as much as the marks only where a wrong prefix has another sum, so the counts must vary along the query.  Construction: queries
in a file of their own, -F F (but the seg set), seed 111111 over the 9-class alphabet, step 1.  The reference is the queries cut into
pieces of P = min(300, max(12, len // 6)) WINDOWS (P + 5 residues: neighbours share five, so every window of the seed lies in exactly one
piece), piece k present CYC[(k + rot) % 5] times (CYC = 1, 5, 2, 7, 3): a window counts what its piece does, and what chance adds.  A query
of at most 8 windows is too short for pieces: the reference holds its prefixes of 6 + i residues, `boost` times each, so that window i counts boost * (nk - i).  thr is set per set so that the median query's limit is half
its total count.  The generator then asks the model, query by query, whether every variant the query is there for (`need`) gives another
work figure; a query that cannot tell one apart gets another rotation of CYC (then other residues) and the set is built again
(search_design: deterministic; what it found for the larger sets is kept in DESIGN, and tests/test_ksc_cap_inputs.py asserts the
inequalities on the sets as built).

Key shapes (every size from 33 windows up; residues of equal self score but different classes give ties without collapsing the buckets:
R Q E K M T score 5, N D G F 6, A I L S V 4):
  tied    R Q E K M T only: every window scores 30, the order is ALL the quicksort's
  two     scores 6 5 6 5 5 6 5 with period 7: a window lacks one position of the period, 32 and 33 interleaved
  asc     residues of score 4, then 5, then 6: self scores ascend in plateaus;  desc: the reverse
  saw     score 4 + (i % 24) // 8: a sawtooth
  rand20  seeded iid over the 20 residues
  seg     -F T: scores 4 / 5, and a run of A between two stretches of W C H Y F D N that SEG masks: the windows of a few strong residues and
          x stand EARLY in the order with a count of 0 (ranks consumed without adding hits), the all-x windows last
Behind the designed queries of a shape set and of the small set stand as many LIGHT ones and one more (40 residues of P W H, nothing of
them in the reference: a total of next to nothing), so that the designed ones are a minority of the batch: with the orders on demand they go through the
open list (k_ksc_order_* and k_cap over a list), with SOHIT_KSC_LAZY=0 through the instances over the whole batch.
Sizes (SIZES; the `small` set holds 1, 2, 6, 7, 8, 31, 32 on scores 5 / 6): insertion sort below 7, the pivot l + 3 at exactly 7, the first
partition at 8; WQS_PAR = 32 from both sides; the ballot and PF steps at 63 .. 65, 128, 129; every LDS instance at its last and the next
at its first window count (512 / 513, 1024 / 1025, 4096 / 4097: u32 words and u16 lists against u64 words, u32 lists, PF = 16, leafbuf).

What each case is there for (`need`, asserted in tests/test_ksc_cap_inputs.py):
  every query of >= 7 windows   stable (ties by position), reverse (ties by descending position), early (the test behind the add), late
                                (one rank more), and from 17 windows numpy (its own quicksort: below 17 it is an insertion sort, the
                                stable variant); carry (the total dropped at a 64-rank step of k_cap) where the cut lies behind rank 64
  2 .. 6 windows                reverse, early, late: the reference's order below 7 windows IS the stable one (an insertion sort)
  1 window                      nothing: it is taken whatever happens
  513, 1025, 4097 windows       tier: the order as if the instance below had sorted its own capacity and left the rest in place
  cut set                       (below)
cut sets (cut_eq62 .. cut_last): ONE set per place, the tied and the two-valued query of 129 and of 1025 windows in each, every query once
in the reference (its pieces) and the smallest thr at which the place can be reached by ADDING to one window's count: a weight, sequences
(w P) x D for a window w whose class string no other window of the set has, adds D to that window and to nothing else (no query holds a P).
  eq62 .. eq65   the total in front of rank r IS the limit (taken), rank r + 1 is refused: r = 62, 63 end k_cap's first step in front of its
                 edge, 64, 65 behind it (ntake == 64, then 1 or 2).  need: early, late, strict (< for <=); carry for 64, 65
  first          the first rank's count alone exceeds the limit: one window taken.  need: early (takes none), late
  last           the total exceeds the limit only with the last rank: k_cap_all opens the query, k_cap keeps it whole.  need: early
  (a limit is at least the query's length, so a query of 1025 windows needs weights of some thousand copies: 16 000 reference residues a set)
closed_set: the same four queries with a total EQUAL to the limit: k_cap_all keeps them closed -- no variant of k_cap can show (an opened
query would be kept whole); the GPU test reads it off the profile keys: nothing is ordered.
What CANNOT be told apart by a sum, with the reason: late on `last` (nothing is left to take), carry in front of rank 64 and on `last`
(dropping the total only takes more), strict anywhere but on an exact total, anything on one window.

flush_set: ONE tied query whose order makes k_ksc_order_g's leaf list (WQS_LEAF = 512 ranges below 32 elements) fill and flush: on tied
keys a partition of n elements ends with its pivot at (n - 1) // 2 whatever the residues, so the leaves are a function of n alone
(tied_leaves, checked against the move-for-move model qsort_model) and FLUSH_NK = 16384 is the smallest TIED window count above 4096 with
more than 512 (random residues would get there near 10 500 windows, but only the tied family has leaves that no draw can change).
The LDS instances cannot flush: the most leaves any family above produces at 512 / 1024 / 4096 windows (seven families, qsort_model) is
far below 128 / 256 / 512 (tests/test_ksc_cap_inputs.py asserts the maxima) -- no such case exists among them.

flow sets (eight queries of 100 residues per batch; heavy = scores 5 / 6, pieces as above; light = rand20, once in the reference: its total
stays below the limit):
  half, half1   four / five of eight queries reach their cap: open * 2 <= nq orders the open ones, one more orders everybody
  chunks3       three chunks: nothing open in chunk 0, queries 1 and 3 in chunk 1, queries 2 and 3 in chunk 2 (a second list; have[] holds
                query 3's order)
  deferred      the flush query behind seven light ones: an open query above 4096 windows in a class of its own at the end of a class-ordered
                batch (side stream, chunk_qhits_deferred); with SOHIT_QCLASS=0 the same on the main stream
multi sets: seeds 111111,11111011111 (mink 6, counts summed over both spans) and two alphabets (counts summed over both)."""
import numpy as np

K = 6
SEED = "111111"
HT = 5000011                      # above 9^6: every class string of the seed has a bucket of its own
CYC = (1, 5, 2, 7, 3)
SIZES = (33, 63, 64, 65, 128, 129, 512, 513, 1024, 1025, 4096, 4097)
SMALL = (1, 2, 6, 7, 8, 31, 32)
BOOST = {1: 3, 2: 5, 6: 2, 7: 2, 8: 2}
SHAPES = ("tied", "two", "asc", "desc", "saw", "rand20", "seg")
TIERS = {513: 512, 1025: 1024, 4097: 4096}
WQS_PAR, WQS_LEAF = 32, 512       # refsort.h
LDS_LEAFCAP = {512: 128, 1024: 256, 4096: 512}   # k_seed.hip: k_ksc_order_lds
ORDER_VARIANTS = ("stable", "reverse", "numpy")
CUT_VARIANTS = ("early", "late", "strict", "carry")
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
_G = {4: np.frombuffer(b"AILSV", dtype=np.uint8), 5: np.frombuffer(b"RQEKMT", dtype=np.uint8), 6: np.frombuffer(b"NDGF", dtype=np.uint8)}
_LOW = np.frombuffer(b"AILSVEKMQRT", dtype=np.uint8)
_HIGH = np.frombuffer(b"WCHYFDN", dtype=np.uint8)
TWO_ALPHABETS = "AST,CFILMVY,DN,EQ,G,H,KR,P,W/A,KR,EDNQ,C,G,H,ILVM,FYW,P,ST"


def to_fasta(seqs):
    return b"".join(b">t%04d|p%07d\n%s\n" % (i % 2, i, s.tobytes()) for i, s in enumerate(seqs))


# ================================================================================================================
# the models
# ================================================================================================================
def qsort_model(keys):
    """(permutation, leaves): the reference quicksort of refsort.h move for move on a list of keys -- insertion sort below 7 elements,
    pivot l + 3 at exactly 7, else l + int(0.3745401188473625 * gap), Hoare partition -- and the number of ranges of 2 .. WQS_PAR - 1
    elements that the wave version hands to its lanes (the entries of its leaf list)"""
    x = [(int(k), i) for i, k in enumerate(keys)]
    stk, leaves = [(0, len(x) - 1, True)], 0
    while stk:
        l, r, top = stk.pop()
        if r <= l:
            continue
        gap = r - l + 1
        if top and gap < WQS_PAR:
            leaves, top = leaves + 1, False
        if gap < 7:
            for i in range(l, r + 1):
                v, j = x[i], i - 1
                while j >= l and x[j][0] > v[0]:
                    x[j + 1] = x[j]
                    j -= 1
                x[j + 1] = v
            continue
        m = l + 3 if gap == 7 else l + int(0.3745401188473625 * gap)
        x[l], x[m] = x[m], x[l]
        p, i, j = x[l][0], l, r + 1
        while True:
            i += 1
            while i <= r and x[i][0] < p:
                i += 1
            j -= 1
            while x[j][0] > p:
                j -= 1
            if i > j:
                break
            x[i], x[j] = x[j], x[i]
        x[l], x[j] = x[j], x[l]
        stk += [(l, j - 1, top), (j + 1, r, top)]
    return [i for _, i in x], leaves


def tied_leaves(n, _memo={}):
    """leaves of qsort_model on n EQUAL keys: both scans stop on every element, the pivot lands at (n - 1) // 2"""
    if n < 2:
        return 0
    if n < WQS_PAR:
        return 1
    if n not in _memo:
        a = (n - 1) // 2
        _memo[n] = tied_leaves(a) + tied_leaves(n - 1 - a)
    return _memo[n]


FLUSH_NK = next(n for n in range(4097, 1 << 16) if tied_leaves(n) > WQS_LEAF)


def cap_marks(order, cnt, limit):
    """the windows the cap takes, in rank order: the prefix of `order` up to the first rank whose PRECEDING total exceeds the limit"""
    order = np.asarray(order, dtype=np.int64)
    c = cnt[order]
    over = np.flatnonzero(np.cumsum(c) - c > limit)
    return order[:int(over[0]) if len(over) else len(order)]


def variant_order(oracle, ksc, variant):
    if variant == "stable":
        return np.argsort(-ksc, kind="stable")
    if variant == "reverse":
        return np.lexsort((-np.arange(len(ksc)), -ksc))
    if variant == "numpy":   # (16-bit keys: numpy's plain introsort on every machine, no vector sort)
        return np.argsort((-ksc).astype(np.int16), kind="quicksort")
    if isinstance(variant, tuple) and variant[0] == "tier":
        cap = variant[1]
        return np.array(oracle.qsort_perm(-ksc[:cap]) + list(range(cap, len(ksc))), dtype=np.int64)
    return np.array(oracle.qsort_perm(-ksc), dtype=np.int64)


def variant_work(oracle, ksc, cnt, limit, variant=None):
    """a query's work in one chunk under the reference's rule (None) or under ONE wrong variant"""
    if len(ksc) == 0:
        return 0
    order = variant_order(oracle, ksc, variant)
    c = cnt[order]
    pre = np.cumsum(c) - c
    n = len(cap_marks(order, cnt, limit))
    if variant == "early":       # cum += cnt; if cum > limit: break; mark
        over = np.flatnonzero(pre + c > limit)
        n = int(over[0]) if len(over) else len(c)
    elif variant == "late":      # one rank more
        n = min(n + 1, len(c))
    elif variant == "strict":    # < for <=
        over = np.flatnonzero(pre >= limit)
        n = int(over[0]) if len(over) else len(c)
    elif variant == "carry":     # k_cap's 64-rank steps with the carried total dropped at each
        n = 0
        for r0 in range(0, len(c), 64):
            s = c[r0:r0 + 64]
            over = np.flatnonzero(np.cumsum(s) - s > limit)
            n += int(over[0]) if len(over) else len(s)
            if len(over):
                break
    return int(c[:n].sum())


class CapSet:
    """refs, qrys: uint8 arrays; need {query: variants it must tell apart}; tag {query: name of the case}"""

    def __init__(self, name, refs, qrys, thr, ssd=SEED, nr=None, flt="F", chk=50000, need=None, tag=None):
        self.name, self.refs, self.qrys, self.thr, self.ssd, self.nr, self.flt, self.chk = name, refs, qrys, int(thr), ssd, nr, flt, chk
        self.need, self.tag = need or {}, tag or {}
        self.ref, self.qry = to_fasta(refs), to_fasta(qrys)
        self.mink = min(len(s) for s in ssd.split(","))

    def kw(self, oracle):
        return dict(ssd=self.ssd, nr=self.nr or oracle.AA9, ht=HT, chk=self.chk, step=1, v=500, expect=1e-5, flt=self.flt, thr=self.thr)

    def masked(self, oracle, q):
        b = self.qrys[q].tobytes()
        return oracle.seg(b) if self.flt == "T" else b

    def nk(self, q):
        return max(0, len(self.qrys[q]) - self.mink + 1)


def _seeds(oracle, S, b, cache):
    if b not in cache:
        w = oracle.spseeds(b, S.ssd, S.nr or oracle.AA9, HT, 1)
        cache[b] = (np.array([x[0] for x in w], dtype=np.int64), np.array([x[1] for x in w], dtype=np.int64))
    return cache[b]


def model_of(oracle, S):
    """per query (ksc, [cnt per chunk], limit): self scores of the masked query's windows, the entries of every window's buckets in
    every chunk (the chunk's last slot, the smallest entry of its highest bucket, is never read: fsearch.py's `ed = min(ed, L)`)"""
    cache = {}
    chunks = []
    for c0 in range(0, len(S.refs), S.chk):
        bk = np.sort(np.concatenate([_seeds(oracle, S, s.tobytes(), cache)[0] for s in S.refs[c0:c0 + S.chk]] + [np.zeros(0, dtype=np.int64)]))
        chunks.append(bk)
    self_sc = np.array([oracle.b62(a, a) for a in range(256)], dtype=np.int64)
    out = []
    for q in range(len(S.qrys)):
        mq = np.frombuffer(S.masked(oracle, q), dtype=np.uint8)
        nk = S.nk(q)
        if nk == 0:
            out.append((np.zeros(0, dtype=np.int64), [np.zeros(0, dtype=np.int64) for _ in chunks], 0))
            continue
        cs = np.concatenate([[0], np.cumsum(self_sc[mq])])
        ksc = cs[S.mink:S.mink + nk] - cs[:nk]
        b, p = _seeds(oracle, S, mq.tobytes(), {})
        cnts = []
        for bk in chunks:
            n = np.searchsorted(bk, b, "right") - np.searchsorted(bk, b, "left")
            if len(bk):
                n = n - ((b == bk[-1]) & (n > 0))
            cnts.append(np.bincount(p, weights=n, minlength=nk)[:nk].astype(np.int64))
        out.append((ksc, cnts, S.thr * len(mq)))
    return out


def model_work(oracle, S, model=None, variant=None):
    """work of every query, summed over the chunks, under the reference's rule or one variant"""
    model = model or model_of(oracle, S)
    return [sum(variant_work(oracle, ksc, c, limit, variant) for c in cnts) for ksc, cnts, limit in model]


def model_flow(S, model, lazy=True):
    """(seed.kmer_orders_open_chunks, seed.kmer_orders_all_at_chunk) of one search of the whole set in ONE batch, and the open queries
    per chunk: host_seed.hip's chunk_qhits restated"""
    nq, some, everybody, ready, opens = len(S.qrys), 0, 0, not lazy, []
    for ci in range(len(model[0][1])):
        o = [q for q, (ksc, cnts, limit) in enumerate(model) if len(ksc) and int(cnts[ci].sum()) > limit]
        opens.append(o)
        if ready or not o:
            continue
        if len(o) * 2 <= nq:
            some |= 1 << ci
        else:
            everybody, ready = everybody + ci + 1, True
    return (some, everybody), opens


def oracle_work(oracle, S):
    """(work per query, marks per query and chunk): the reference figure -- find_msav_m on every chunk's index, threshold set as
    chunk_qhits sets it, one tuple per visited entry"""
    nr, n = S.nr or oracle.AA9, len(S.refs)
    work, marks = [0] * len(S.qrys), [[] for _ in S.qrys]
    for c0 in range(0, n, S.chk):
        ix = oracle.Index(S.ref, S.ssd, nr, 1, HT, c0, min(c0 + S.chk, n))
        if S.thr >= 1 or ix.threshold == 0:
            ix.threshold = S.thr
        for q in range(len(S.qrys)):
            _, tuples, mk = ix.find_msav_m(S.masked(oracle, q), want_tuples=True, tcap=1 << 20)
            work[q] += len(tuples)
            marks[q].append(np.flatnonzero(mk))
    return work, marks


# ================================================================================================================
# shapes and references
# ================================================================================================================
def shape_seq(shape, n, rng):
    i = np.arange(n)
    if shape == "rand20":
        return AA[rng.integers(0, 20, n)]
    if shape == "mix56":
        lv = rng.integers(5, 7, n)
    elif shape == "tied":
        lv = np.full(n, 5)
    elif shape == "two":
        lv = np.array([6, 5, 6, 5, 5, 6, 5])[i % 7]
    elif shape == "asc":
        lv = 4 + (3 * i) // n
    elif shape == "desc":
        lv = 6 - (3 * i) // n
    elif shape == "saw":
        lv = 4 + (i % 24) // 8
    elif shape == "seg":
        run, fl = (10, 2) if n < 100 else (30, 12)
        at = max(0, (n - run - 2 * fl) // 3)
        s = _LOW[rng.integers(0, len(_LOW), n)]
        blk = np.concatenate([_HIGH[rng.integers(0, len(_HIGH), fl)], np.full(run, ord("A"), dtype=np.uint8), _HIGH[rng.integers(0, len(_HIGH), fl)]])
        s[at:at + len(blk)] = blk[:n - at]
        return s
    else:
        raise ValueError(shape)
    return np.array([_G[int(v)][int(rng.integers(len(_G[int(v)])))] for v in lv], dtype=np.uint8)


def pieces_of(q, rot=0, boost=1, scale=1):
    """the reference sequences of one query (head of the file): [(sequence, times)]"""
    n = len(q)
    nk = n - K + 1
    if nk <= 8:
        return [(q[:K + i], boost + rot) for i in range(nk)]
    P = min(300, max(12, n // 6))
    return [(q[a:a + P + K - 1], scale * CYC[(k + rot) % len(CYC)]) for k, a in enumerate(range(0, nk, P))]


def _refs_of(parts):
    return [s for s, t in parts for _ in range(t)]


def needs_of(nk):
    if nk < 2:
        return ()
    if nk < 7:
        return ("reverse", "early", "late")
    need = ("stable", "reverse", "early", "late") + (("numpy",) if nk >= 17 else ())
    return need + ((("tier", TIERS[nk]),) if nk in TIERS else ())


def undecided(oracle, S, model=None):
    """{query: variants of its `need` that give the reference's work figure} -- empty when the set tells everything apart; a query
    whose cut lies behind rank 64 must tell `carry` apart too"""
    model = model or model_of(oracle, S)
    ref = model_work(oracle, S, model)
    bad = {}
    for q, need in S.need.items():
        ksc, cnts, limit = model[q]
        need = tuple(need)
        if "stable" in need and any(64 < len(cap_marks(variant_order(oracle, ksc, None), c, limit)) < len(ksc) for c in cnts):
            need += ("carry",)
        same = [v for v in need if sum(variant_work(oracle, ksc, c, limit, v) for c in cnts) == ref[q]]
        if "stable" in need and not any(len(cap_marks(variant_order(oracle, ksc, None), c, limit)) < len(ksc) for c in cnts):
            same.append("no cut")
        if same:
            bad[q] = same
    return bad


def _auto_thr(model):
    r = [sum(int(c.sum()) for c in cnts) / (2.0 * max(1, limit)) for ksc, cnts, limit in model if len(ksc) > 8]
    return max(1, int(round(float(np.median(r))))) if r else 1


def _build(name, plan, seed, state, thr, mink, kw, light=0):
    qrys, refs = [], []
    for k, (shape, nk) in enumerate(plan):
        rot, draw = state[k]
        q = shape_seq(shape, nk + mink - 1, np.random.default_rng([seed, k, draw]))
        qrys.append(q)
        refs += _refs_of(pieces_of(q, rot, BOOST.get(nk, 1)))
    need = {k: needs_of(nk) for k, (shape, nk) in enumerate(plan)}
    tag = {k: "%s%d" % (shape, nk) for k, (shape, nk) in enumerate(plan)}
    for j in range(light):   # light queries behind the designed ones: P W H only, no piece in the reference, never above a limit
        qrys.append(np.frombuffer(b"PWH", dtype=np.uint8)[np.random.default_rng([seed, 9000 + j]).integers(0, 3, 40)])
    return CapSet(name, refs, qrys, thr, need=need, tag=tag, **kw)


def _design_one(oracle, k, shape, nk, mink, seed, thr, kw, tries=400):
    """(rotation, re-draw) of query k with which the query ALONE, against its own pieces, tells all its variants apart"""
    for t in range(tries):
        rot, draw = t % len(CYC), t // len(CYC)
        q = shape_seq(shape, nk + mink - 1, np.random.default_rng([seed, k, draw]))
        S = CapSet("one", _refs_of(pieces_of(q, rot, BOOST.get(nk, 1))), [q], thr, need={0: needs_of(nk)}, tag={0: shape}, **kw)
        if not undecided(oracle, S):
            return [rot, draw]
    return [0, 0]


def search_design(oracle, name, plan, seed, mink, kw, thr=None, light=0, rounds=80):
    """(thr, [(rotation, re-draw) per query]): the search that wrote DESIGN -- each query alone against its own pieces first, then the
    whole set (chance matches between the queries' pieces move the counts), a query that cannot tell one of its variants apart moved on
    to its next rotation / re-draw, until none is left"""
    state = [[0, 0] for _ in plan]
    thr = thr or _auto_thr(model_of(oracle, _build(name, plan, seed, state, 1, mink, kw)))
    state = [_design_one(oracle, k, shape, nk, mink, seed, thr, kw) for k, (shape, nk) in enumerate(plan)]
    bad = {}
    for _ in range(rounds):
        S = _build(name, plan, seed, state, thr, mink, kw, light)
        bad = undecided(oracle, S)
        if not bad:
            return thr, [tuple(x) for x in state]
        for q in bad:
            state[q][0] += 1
            if state[q][0] == len(CYC):
                state[q] = [0, state[q][1] + 1]
    raise AssertionError("%s: no design tells these apart: %r" % (name, {S.tag[q]: v for q, v in bad.items()}))


# name: (thr, [(rotation, re-draw) per query]) as search_design found them (a set that is not here is searched for when it is asked for)
DESIGN = {
    'tied': (11, [(1, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (1, 0), (0, 0), (0, 0), (1, 1), (1, 0)]),
    'two': (5, [(0, 0), (1, 0), (0, 0), (1, 0), (1, 0), (0, 0), (0, 0), (1, 0), (3, 5), (4, 19), (1, 0), (0, 0)]),
    'asc': (47, [(0, 1), (0, 0), (0, 1), (0, 0), (0, 0), (1, 0), (0, 0), (0, 0), (0, 0), (0, 0), (1, 9), (1, 14)]),
    'desc': (43, [(0, 3), (1, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (1, 1)]),
    'saw': (17, [(2, 1), (0, 1), (0, 0), (1, 0), (1, 0), (1, 1), (0, 0), (0, 0), (1, 0), (0, 0), (1, 5), (1, 4)]),
    'rand20': (3, [(1, 11), (2, 4), (2, 4), (4, 3), (1, 3), (2, 2), (3, 1), (2, 3), (4, 0), (0, 2), (0, 2), (0, 2)]),
    'seg': (1, [(4, 10), (1, 2), (3, 1), (4, 0), (4, 0), (1, 1), (4, 0), (2, 1), (1, 1), (2, 2), (0, 1), (3, 3)]),
    'small': (1, [(0, 0), (0, 0), (0, 0), (2, 0), (0, 0), (4, 0), (0, 1)]),
    'spans': (3, [(0, 0), (3, 0), (2, 0), (0, 0)]),
    'alphabets': (3, [(0, 0), (0, 1), (0, 0), (3, 0)]),
}


def designed_set(oracle, name, plan, seed, flt="F", ssd=SEED, nr=None, thr=None, light=0):
    """plan: [(shape, windows)]: the queries, their pieces and thr as DESIGN has them (head of the file); tests/test_ksc_cap_inputs.py
    asserts that the set so built tells every variant apart"""
    mink = min(len(s) for s in ssd.split(","))
    kw = dict(ssd=ssd, nr=nr, flt=flt)
    if name not in DESIGN:
        DESIGN[name] = search_design(oracle, name, plan, seed, mink, kw, thr, light)
    thr, state = DESIGN[name]
    return _build(name, plan, seed, state, thr, mink, kw, light)


def shape_set(oracle, shape):
    seg = shape == "seg"   # (thr 1: a masked window counts nothing, the short queries' totals are small)
    return designed_set(oracle, shape, [(shape, nk) for nk in SIZES], 61000 + SHAPES.index(shape), flt="T" if seg else "F", thr=1 if seg else None,
                        light=len(SIZES) + 1)


def small_set(oracle):
    return designed_set(oracle, "small", [("mix56", nk) for nk in SMALL], 61010, thr=1, light=len(SMALL))


def multi_set(oracle, which):
    plan = [("rand20", nk) for nk in (60, 65, 129, 513)]
    if which == "spans":
        return designed_set(oracle, "spans", plan, 61020, ssd="111111,11111011111")
    return designed_set(oracle, "alphabets", plan, 61021, nr=TWO_ALPHABETS)


def flush_set(oracle, extra=()):
    """the tied query of FLUSH_NK windows (`extra`: light queries in front of it)"""
    plan = [("rand20", 95)] * len(extra) + [("tied", FLUSH_NK)]
    for draw in range(20):
        qrys, refs = [], []
        for k, (shape, nk) in enumerate(plan):
            q = shape_seq(shape, nk + K - 1, np.random.default_rng([61030, k, draw]))
            qrys.append(q)
            refs += _refs_of(pieces_of(q) if shape == "tied" else [(q, 1)])
        last = len(plan) - 1
        S = CapSet("deferred" if extra else "flush", refs, qrys, 1, need={last: needs_of(FLUSH_NK)}, tag={last: "tied%d" % FLUSH_NK})
        model = model_of(oracle, S)
        S.thr = max(1, int(round(int(model[last][1][0].sum()) / (2.0 * len(qrys[last])))))
        model = [(ksc, cnts, S.thr * len(S.qrys[q])) for q, (ksc, cnts, _) in enumerate(model)]
        if not undecided(oracle, S, model):
            return S
    raise AssertionError("flush: no design")


# ================================================================================================================
# flows
# ================================================================================================================
def _settle(oracle, build, n, rounds=200):
    """build(state) -> set, state = [(rotation, re-draw)] of its n designed queries: moved on until the set tells everything apart"""
    state = [[0, 0] for _ in range(n)]
    for _ in range(rounds):
        S = build(state)
        bad = undecided(oracle, S)
        if not bad:
            return S
        for q in bad:
            state[S.designed.index(q)][0] += 1
            if state[S.designed.index(q)][0] == len(CYC):
                state[S.designed.index(q)] = [0, state[S.designed.index(q)][1] + 1]
    raise AssertionError("no design tells these apart: %r" % ({S.tag[q]: v for q, v in bad.items()},))


def flow_set(oracle, name):
    """half / half1: eight queries of 100 residues, the first four / five heavy (scores 5 / 6, their pieces as in the shape sets), the
    others light (rand20, once in the reference).  chunks3: chunk 0 holds the first 80 residues of every query, chunk 1 the pieces of
    queries 1 and 3, chunk 2 those of queries 2 and 3, each filled up to chk sequences with short fillers."""
    light = [shape_seq("rand20", 100, np.random.default_rng([61040, k])) for k in range(8)]
    heavy = {"half": [0, 1, 2, 3], "half1": [0, 1, 2, 3, 4], "chunks3": [1, 2, 3]}[name]
    fill = [shape_seq("rand20", 12, np.random.default_rng([61041, k])) for k in range(64)]
    chk = 64

    def build(state):
        qrys, parts = list(light), {}
        for (rot, draw), k in zip(state, heavy):
            qrys[k] = shape_seq("mix56", 100, np.random.default_rng([61042, k, draw]))
            parts[k] = _refs_of(pieces_of(qrys[k], rot))
        if name == "chunks3":
            refs = []
            for chunk in ([q[:80] for q in qrys], parts[1] + parts[3], parts[2] + parts[3]):
                assert len(chunk) <= chk
                refs += chunk + fill[:chk - len(chunk)]
        else:
            refs = [s for k in range(8) for s in (parts[k] if k in parts else [qrys[k]])]
        S = CapSet(name, refs, qrys, 1, chk=chk if name == "chunks3" else 50000, need={k: needs_of(95) for k in heavy}, tag={k: "heavy%d" % k for k in heavy})
        S.designed = heavy
        if name != "chunks3":
            S.thr = _auto_thr([model_of(oracle, S)[k] for k in heavy])
        return S

    return _settle(oracle, build, len(heavy))


# ================================================================================================================
# cut placement
# ================================================================================================================
PLACES = ("eq62", "eq63", "eq64", "eq65", "first", "last")
CUT_NEED = {"eq62": ("early", "late", "strict"), "eq63": ("early", "late", "strict"), "eq64": ("early", "late", "strict", "carry"),
            "eq65": ("early", "late", "strict", "carry"), "first": ("early", "late"), "last": ("early",), "sum": ()}


def _weights(w, d):
    """sequences that add d to the count of the 6-mer w and to nothing else a P-free query holds"""
    unit = np.concatenate([w, np.frombuffer(b"P", dtype=np.uint8)])
    return [np.tile(unit, min(42, d - a)) for a in range(0, d, 42)]


def _unique_windows(qrys):
    """{query: positions of the windows whose 6 residues' classes no other window of the set shares}"""
    from collections import Counter
    cls = np.zeros(256, dtype=np.int64)
    for i, g in enumerate("AST,CFILMVY,DN,EQ,G,H,KR,P,W".split(",")):
        for ch in g:
            cls[ord(ch)] = i
    keys = [[cls[q[i:i + K]].tobytes() for i in range(len(q) - K + 1)] for q in qrys]
    n = Counter(k for ks in keys for k in ks)
    return [[i for i, k in enumerate(ks) if n[k] == 1] for ks in keys]


def placed_set(oracle, name, place, seed=61050, tmax=12):
    """the tied and the two-valued queries of 129 and 1025 windows, once per place, at ONE thr: the smallest for which every place
    can be reached by ADDING weight to one window of each query (found by trying: a weight changes no order and no other window).  A
    query whose place needs a window that shares its class string with another one is drawn again."""
    plan = [(shape, nk, place) for nk in (129, 1025) for shape in ("tied", "two")]
    need = {k: CUT_NEED[place] for k, (_, _, place) in enumerate(plan)}
    tag = {k: "%s%d_%s" % p for k, p in enumerate(plan)}
    draw = [0] * len(plan)
    for _ in range(40):
        qrys = [shape_seq(shape, nk + K - 1, np.random.default_rng([seed, k, draw[k]])) for k, (shape, nk, place) in enumerate(plan)]
        base = []
        for k, q in enumerate(qrys):
            base += [piece for piece, _ in pieces_of(q)]
        uniq = _unique_windows(qrys)
        model = model_of(oracle, CapSet(name, base, qrys, 1))
        again = False
        for T in range(1, tmax):
            extra, ok = [], True
            for k, (shape, nk, place) in enumerate(plan):
                ksc, (cnt,), _ = model[k]
                limit = T * len(qrys[k])
                order = variant_order(oracle, ksc, None)
                c = cnt[order]
                pre = np.cumsum(c) - c
                u = set(uniq[k])
                fits = True   # (with this T)
                if place.startswith("eq"):
                    r = int(place[2:])
                    d, at = limit - int(pre[r]), [int(p) for p in order[:r] if int(p) in u]
                    sound = c[r] > 0 and c[r + 1] > 0
                elif place == "first":
                    d, at = limit + 1 - int(c[0]), [int(p) for p in order[:1] if int(p) in u]
                    sound = c[1] > 0
                elif place == "last":
                    d, at = limit + 1 - int(c.sum()), [int(p) for p in order[-1:] if int(p) in u]
                    sound, fits = True, int(pre[-1]) <= limit
                else:   # sum: the total IS the limit
                    d, at = limit - int(c.sum()), [int(p) for p in order if int(p) in u]
                    sound = True
                if not sound or not at:   # (no thr mends this: other residues)
                    draw[k], again = draw[k] + 1, True
                if d < 0 or not fits or not sound or not at:
                    ok = False
                    break
                if d:
                    extra += _weights(qrys[k][at[0]:at[0] + K], d)
            if again:
                break
            if ok:
                return CapSet(name, base + extra, qrys, T, need=need, tag=tag)
    raise AssertionError("%s: no thr below %d reaches every place" % (name, tmax))


def cut_set(oracle, place):
    return placed_set(oracle, "cut_" + place, place, seed=61050 + PLACES.index(place))


def closed_set(oracle):
    return placed_set(oracle, "closed", "sum", seed=61059)


SET_NAMES = SHAPES + ("small", "spans", "alphabets", "flush", "deferred", "half", "half1", "chunks3") + tuple("cut_" + p for p in PLACES) + ("closed",)
_SETS = {}


def get_set(oracle, name):
    """the set of that name, built once per process"""
    if name not in _SETS:
        if name in SHAPES:
            S = shape_set(oracle, name)
        elif name == "small":
            S = small_set(oracle)
        elif name in ("spans", "alphabets"):
            S = multi_set(oracle, name)
        elif name == "flush":
            S = flush_set(oracle)
        elif name == "deferred":
            S = flush_set(oracle, extra=range(7))
        elif name in ("half", "half1", "chunks3"):
            S = flow_set(oracle, name)
        elif name.startswith("cut_"):
            S = cut_set(oracle, name[4:])
        else:
            S = closed_set(oracle)
        _SETS[name] = S
    return _SETS[name]


_WORK = {}


def reference_work(oracle, name):
    """the oracle's work per query of the set (computed once per process)"""
    if name not in _WORK:
        _WORK[name] = oracle_work(oracle, get_set(oracle, name))
    return _WORK[name]
