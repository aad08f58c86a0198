"""Inputs for tests/test_gpu_uqchain.py: small protein sets whose MULTI-HIT diagonals -- the hits k_ungapq leaves over, which the chain flow
(k_uqsort_wave / k_uqsort_wg + k_ungap2, SOHIT_UQ_CHAINS) sorts per query (a wave's registers, a workgroup's LDS) and chains from the list of group heads -- are planted, and a
plain numpy model of them.

The model: seed pattern 11111011111 over the 9-class alphabet, one chunk, step 1, the frequency cap out of reach (thr).  A hit of query q
is a pair (query window, index entry of the window's bucket); its diagonal is (subject, subject position - query position).  The windows are
the oracle's own (oracle.spseeds; the query's after the SEG mask, the subjects' unmasked).  An index entry at subject position 0 is kept
under the sequence in front of it, at the position behind its last residue, as the reference keeps it (never scored: a protein's own diagonal
holds length - 11 hits).  A GROUP is a diagonal with two and more hits; a query's
LEFTOVER count is the sum of its groups' sizes.  k_ungapq may leave over a few lone hits more -- two lone diagonals on one of its 4096 counters
are BOTH left over, each a group of one hit for the chain kernel -- never fewer: the GPU tests compare the library's counters against these
figures from below.  (So a leftover count of exactly 1 does not exist: the smallest is 2.)"""
import numpy as np

from ungapq_inputs import AA, HT, SEED, to_fasta

__all__ = ["AA", "HT", "SEED", "to_fasta", "ChainModel", "shape_set", "tier_set", "band_set", "cap_set", "short_set"]

DSH = 20   # group key = subject << DSH | (diagonal + 2^(DSH - 1))


def windows(oracle, seq, masked=False, ssd=SEED):
    """(buckets, positions) of the seed windows of one protein (uint8 ASCII array); masked: as a QUERY (None: no SEG mask, -F F)"""
    b = seq.tobytes()
    if masked:
        b = oracle.seg(b)
    w = oracle.spseeds(b, ssd, oracle.AA9, HT, 1)
    return np.array([x[0] for x in w], dtype=np.int64), np.array([x[1] for x in w], dtype=np.int64)


class ChainModel:
    """groups of every query of `qrys` against the subjects `refs` (qrys None: all-vs-all).  ssd: the seed pattern (one); flt: the queries
    pass the SEG mask (-F T); chk: sequences per chunk (None: one chunk) -- the offset-0 entry of a chunk's FIRST sequence is the one the
    library drops (`drop`; the oracle counts it, a group that is never scored)"""

    def __init__(self, oracle, refs, qrys=None, ssd=SEED, flt=True, chk=None):
        self.oracle = oracle
        self.refs = refs
        self.qrys = refs if qrys is None else qrys
        self.ssd, self.flt = ssd, flt
        bk, sid, pos, drop, raw = [], [], [], [], []
        for s, seq in enumerate(refs):
            b, p = windows(oracle, seq, ssd=ssd)
            raw.append(p)
            z = p == 0   # (the offset-0 entry: see the head of the file)
            bk.append(b), pos.append(np.where(z, len(refs[s - 1]) if s else 0, p)), sid.append(np.where(z, s - 1, s).astype(np.int64))
            drop.append(z & ((s % chk == 0) if chk else (s == 0)))
        bk, sid, pos, drop = np.concatenate(bk), np.concatenate(sid), np.concatenate(pos), np.concatenate(drop)
        # the reference never reads the last slot of a chunk's index: the smallest entry (subject, position) of the chunk's highest bucket
        # is no hit for anybody (tests/test_gpu_parity.py check_index)
        own = np.repeat(np.arange(len(refs)), [len(x) for x in raw])
        raw = np.concatenate(raw)
        keep = np.ones(len(bk), dtype=bool)
        for c in np.unique(own // chk if chk else own * 0):
            i = np.flatnonzero((own // chk if chk else own * 0) == c)
            i = i[bk[i] == bk[i].max()]
            keep[i[np.lexsort((raw[i], own[i]))[0]]] = False
        bk, sid, pos, drop = bk[keep], sid[keep], pos[keep], drop[keep]
        o = np.argsort(bk, kind="stable")
        self.bk, self.sid, self.pos, self.drop = bk[o], sid[o], pos[o], drop[o]
        self._d, self._h = {}, {}

    def hits(self, q):
        """(subject, subject position, query position, dropped by the library) of every hit of query q"""
        if q not in self._h:
            b, p = windows(self.oracle, self.qrys[q], self.flt, self.ssd)
            lo, hi = np.searchsorted(self.bk, b, "left"), np.searchsorted(self.bk, b, "right")
            n = hi - lo
            at = np.repeat(lo, n) + (np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n))
            self._h[q] = (self.sid[at], self.pos[at], np.repeat(p, n), self.drop[at])
        return self._h[q]

    def diagonals(self, q):
        """(keys, sizes) of all diagonals of query q; key = subject << DSH | (diagonal + 2^(DSH - 1))"""
        if q not in self._d:
            sid, pos, qp, _ = self.hits(q)
            key = (sid << DSH) | (pos - qp + (1 << (DSH - 1)))
            self._d[q] = np.unique(key, return_counts=True)
        return self._d[q]

    def groups(self, q):
        """... of the diagonals with two and more hits"""
        u, c = self.diagonals(q)
        return u[c >= 2], c[c >= 2]

    def sizes_on(self, q, s):
        """{diagonal: hits} of query q's groups on subject s"""
        u, c = self.groups(q)
        m = (u >> DSH) == s
        return {int(k & ((1 << DSH) - 1)) - (1 << (DSH - 1)): int(n) for k, n in zip(u[m], c[m])}

    def left_counts(self):
        return np.array([int(self.groups(q)[1].sum()) for q in range(len(self.qrys))], dtype=np.int64)

    def n_groups(self):
        return int(sum(len(self.groups(q)[0]) for q in range(len(self.qrys))))


def _iid(rng, n):
    return AA[rng.integers(0, 20, size=n)]


def _plant(h, at, q, qa, n):
    """q[qa : qa + n] into h at offset `at`; the residues in front of and behind it made a mismatch in the 9-class alphabet, so that the shared
    windows are the segment's n - 10 and no chance match lengthens the group"""
    h[at:at + n] = q[qa:qa + n]
    for hp, qp in ((at - 1, qa - 1), (at + n, qa + n)):
        if 0 <= hp < len(h) and 0 <= qp < len(q):
            h[hp] = ord("G") if q[qp] == ord("W") else ord("W")   # (W and G are classes of their own)


def _host(rng, q, qa, n, length, at):
    """an iid protein of `length` residues with q[qa : qa + n] at offset `at`"""
    h = _iid(rng, length)
    _plant(h, at, q, qa, n)
    return h


# query residue -> a subject residue of the same 9-class letter that scores below zero against it (BLOSUM62: -2 or -1): a seed hit that
# adds nothing to an extension
_NEG = {ord(a): ord(b) for a, b in zip("CFIYLMV", "FCYCCCY")}


def shape_set(oracle, seed=30311, n_back=420):
    """(fasta, model, where): about 450 proteins (two chunks at chk=400), all-vs-all.  `where` names the planted cases:
      none          a protein of 11 residues: one window, one hit, no group (query without leftover hits; the shortest query)
      pair, triple  (query, host, diagonal): a shared segment of 12 / 13 residues: a group of exactly 2 / 3 hits
      g64, g65      the same with 74 / 75 residues: groups of exactly 64 and 65 hits
      copies        four copies of one 250-residue protein: on every copy a group of about 240 hits, four of them per query
      neighbours    (query, host, d): two 12-residue segments of the query in one host, on diagonals d and d + 1
      repeat        (query, host, d0, d1): one 12-residue segment of the query twice in one host: two groups on the same subject
      cover         (query, host, d, r1_end): 20 identical residues followed at once by 15 residues that are seed hits but score below zero:
                    the seeds inside the first segment's reach are covered, the one at r1_end + 1 runs with its left pass bounded at once
      cover_gap     the same with three residues in between that are no hit (-4 each): the left pass of the seed behind them runs three
                    residues and is bounded there (unbounded it would climb the 20 identical residues)
      long          a protein of 512 residues (the longest query of k_ungapq's slot)
      self63 ...    iid proteins of 74 / 75 / 76 residues: 63 / 64 / 65 hits on their own diagonal, the leftover hits of these queries"""
    rng = np.random.default_rng(seed)
    for _ in range(32):
        seqs = [_iid(rng, int(rng.integers(40, 121))) for _ in range(n_back)]
        where = {}

        def add(s):
            seqs.append(s)
            return len(seqs) - 1

        where["none"] = add(_iid(rng, 11))
        for name, ln in (("pair", 12), ("triple", 13), ("g64", 74), ("g65", 75)):
            q = _iid(rng, ln + 60)
            qi = add(q)
            hi = add(_host(rng, q, 25, ln, ln + 50, 10))
            where[name] = (qi, hi, 10 - 25)
        big = _iid(rng, 250)
        where["copies"] = [add(big.copy()) for _ in range(4)]
        q = _iid(rng, 120)
        h = _iid(rng, 140)
        _plant(h, 40, q, 20, 12)   # diagonal 20
        _plant(h, 71, q, 50, 12)   # diagonal 21
        where["neighbours"] = (add(q), add(h), 20)
        q = _iid(rng, 100)
        h = _iid(rng, 150)
        _plant(h, 15, q, 30, 12)   # diagonal -15
        _plant(h, 90, q, 30, 12)   # diagonal 60
        where["repeat"] = (add(q), add(h), -15, 60)
        for name, gap in (("cover", 0), ("cover_gap", 3)):
            q = _iid(rng, 110)
            q[50:50 + gap] = ord("W")
            q[50 + gap:65 + gap] = np.frombuffer(b"CFIYLMV", dtype=np.uint8)[rng.integers(0, 7, size=15)]
            h = _iid(rng, 120)
            _plant(h, 40, q, 30, 35 + gap)   # diagonal 10: 20 identical residues ...
            h[60:60 + gap] = ord("D")
            h[60 + gap:75 + gap] = [_NEG[int(x)] for x in q[50 + gap:65 + gap]]
            where[name] = (add(q), add(h), 10, 49)
        where["long"] = add(_iid(rng, 512))
        for c in (63, 64, 65):
            where["self%d" % c] = add(_iid(rng, c + 11))
        m = ChainModel(oracle, seqs)
        if shape_set_problems(oracle, seqs, m, where):
            continue   # (a chance match or a masked window spoilt a planted case: draw again)
        return to_fasta(seqs), m, where
    raise AssertionError("the planted cases keep meeting chance matches")


def shape_set_problems(oracle, seqs, m, where):
    """what keeps the set from being the one shape_set describes ([]: nothing)"""
    bad = []
    left = m.left_counts()
    if left[where["none"]] != 0:
        bad.append("none")
    for name, n in (("pair", 2), ("triple", 3), ("g64", 64), ("g65", 65)):
        q, h, d = where[name]
        if m.sizes_on(q, h) != {d: n}:
            bad.append(name)
    for q in where["copies"]:
        if any(m.sizes_on(q, s).get(0, 0) < 200 for s in where["copies"]):
            bad.append("copies")
    q, h, d = where["neighbours"]
    if m.sizes_on(q, h) != {d: 2, d + 1: 2}:
        bad.append("neighbours")
    q, h, d0, d1 = where["repeat"]
    if m.sizes_on(q, h) != {d0: 2, d1: 2}:
        bad.append("repeat")
    for name, gap in (("cover", 0), ("cover_gap", 3)):
        q, h, d, r1 = where[name]
        n = m.sizes_on(q, h)
        # the diagonal: the windows at query positions 30 .. 54 without a gap (25 of them); with it 30 .. 39 and 53 .. 57 (10 + 5).  (The 15
        # residues of one class make short groups on the diagonals next to it as well.)
        if n.get(d) != (25 if gap == 0 else 15):
            bad.append(name)
            continue
        qs, hs = seqs[q].tobytes(), seqs[h].tobytes()
        # the first seed's right pass has its maximum at the end of the identical residues; the seed behind them scores nothing to its right
        if oracle.ungap(qs, hs, 30, 30 + d)[2] != r1:
            bad.append(name + ":max_qed")
        nxt = r1 + 1 + gap
        if oracle.ungap(qs, hs, nxt, nxt + d, r1, r1 + d)[0] > 0:
            bad.append(name + ":next")
        # ... and its left pass, unbounded, would climb them
        if oracle.ungap(qs, hs, nxt, nxt + d)[0] <= 40:
            bad.append(name + ":unbounded")
    if len(seqs[where["long"]]) != 512 or left[where["long"]] < 400:
        bad.append("long")
    for c in (63, 64, 65):
        if left[where["self%d" % c]] != c:
            bad.append("self%d" % c)
    return bad


def _family(rng, seqs, target, unit=310):
    """proteins whose leftover count is `target`: k copies of one iid protein of `unit` residues (unit - 11 hits on each copy's diagonal) and a
    host with the first r + 10 residues of it (r more), k * (unit - 11) + r = target; returns the copies' indices"""
    per = unit - 11
    k = max(1, (target - 2) // per)
    r = target - k * per
    while r > per or (0 < r < 2):   # the partial copy is a group of 2 .. per hits (or absent)
        k, r = (k + 1, r - per) if r > per else (k - 1, r + per)
    p = _iid(rng, unit)
    idx = []
    for _ in range(k):
        seqs.append(p.copy())
        idx.append(len(seqs) - 1)
    if r:
        seqs.append(_host(rng, p, 0, r + 10, r + 10 + 30, 15))   # (its first window sits at query position 0 and subject position 15: r hits)
    return idx


def tier_set(oracle, limits, seed=30312, n_back=256):
    """(fasta, model, {count: [queries]}): all-vs-all; per tier limit L of `limits` three families of proteins whose leftover counts are
    L - 1, L and L + 1 (copies of one protein: their own diagonals, plus one partial copy); the queries listed are the ones whose model count is
    exactly that"""
    rng = np.random.default_rng(seed)
    for _ in range(32):
        seqs = [_iid(rng, int(rng.integers(40, 101))) for _ in range(n_back)]
        fam = {}
        for L in limits:
            for c in (L - 1, L, L + 1):
                fam[c] = _family(rng, seqs, c)
        m = ChainModel(oracle, seqs)
        fam = {c: [q for q in qs if int(m.groups(q)[1].sum()) == c] for c, qs in fam.items()}   # (a chance group with another protein moves a copy off its count)
        if all(fam.values()):
            return to_fasta(seqs), m, fam
    raise AssertionError("the families keep meeting chance matches")


def band_set(oracle, seed=30313, n_q=260, slen=6000, ssd=SEED):
    """(reference fasta, query fasta, model): n_q queries of 60 .. 200 residues against themselves and ONE subject of `slen` residues that
    holds a 40-residue segment of every fourth query: a subject too long for one diagonal band, with groups in every part of it"""
    rng = np.random.default_rng(seed)
    qs = [_iid(rng, int(rng.integers(60, 201))) for _ in range(n_q)]
    big = _iid(rng, slen)
    for k, q in enumerate(qs[::4]):
        at = 20 + k * ((slen - 100) // (len(qs[::4])))
        _plant(big, at, q, 10, 40)
    refs = qs + [big]
    return to_fasta(refs), to_fasta(qs), ChainModel(oracle, refs, qs, ssd=ssd)


def cap_set(oracle, seed=30314, n_back=256):
    """(fasta, model, query): all-vs-all; `query` (200 residues, 100 of them again in a host) has more leftover hits than any other protein"""
    rng = np.random.default_rng(seed)
    for _ in range(32):
        seqs = [_iid(rng, int(rng.integers(30, 71))) for _ in range(n_back)]
        q = _iid(rng, 200)
        seqs.append(q)
        seqs.append(_host(rng, q, 40, 100, 150, 20))
        m = ChainModel(oracle, seqs)
        left = m.left_counts()
        if left[n_back] >= 270 and left[n_back] > np.delete(left, n_back).max() + 20:
            return to_fasta(seqs), m, n_back
    raise AssertionError("no largest query")


def short_set(oracle, seed=30315, n=4000):
    """(fasta, model): n iid proteins of 30 .. 60 residues, all-vs-all: thousands of queries that each bring little more than their own diagonal
    -- few hits per pass, but every wave of the sorting kernels takes a piece of the chain list: the list's size must follow the waves, not
    the hits"""
    rng = np.random.default_rng(seed)
    seqs = [_iid(rng, int(rng.integers(30, 61))) for _ in range(n)]
    return to_fasta(seqs), ChainModel(oracle, seqs)
