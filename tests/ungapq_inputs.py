"""Inputs for tests/test_gpu_ungapq_edges.py: small protein sets whose per-query seed-hit counts sit on the edges of k_ungapq's walk (64-ordinal
steps, 256-ordinal tiles, the register cache of SOHIT_UQ_CACHE ordinals), and a plain numpy model of those counts to build them with.

The model: seed pattern 11111011111 over the 9-class alphabet, all-vs-all, one chunk, step 1, the frequency cap out of reach (thr): the hits
of a query are, window by window in position order, the index entries of the window's bucket (the oracle's hash of the window; the windows
of the SEG-masked query, against the unmasked subjects) -- so a query's count is the sum of its windows' bucket sizes, and the hit ordinals
of window w are [sum of the sizes before it, + its own).  The GPU test reads the counts back from the library (query_work) and asserts
that they are the model's."""
import numpy as np

SEED = "11111011111"
HT = 120000000
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
EDGE_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257)


def window_buckets(oracle, seq, masked=False):
    """index bucket of every seed window of one protein (uint8 ASCII array) by the oracle's own hash, in position order; masked: of the
    protein as a QUERY (the windows that the SEG mask touches are gone)"""
    b = seq.tobytes()
    if masked:
        b = oracle.seg(b)
    return np.array([bk for bk, _ in oracle.spseeds(b, SEED, oracle.AA9, HT, 1)], dtype=np.int64)


class Model:
    """window buckets of every protein, as subject and as query, computed once per protein (a redrawn protein: put() again)"""

    def __init__(self, oracle, seqs):
        self.oracle = oracle
        self.ref, self.qry = [], []
        for s in seqs:
            self.ref.append(window_buckets(oracle, s)), self.qry.append(window_buckets(oracle, s, True))

    def put(self, q, s):
        self.ref[q], self.qry[q] = window_buckets(self.oracle, s), window_buckets(self.oracle, s, True)

    def window_hits(self):
        """per protein: the number of index entries of each of its query windows, in position order"""
        u, cnt = np.unique(np.concatenate(self.ref), return_counts=True)
        out = []
        for c in self.qry:
            at = np.searchsorted(u, c)
            at[at >= len(u)] = 0
            out.append(np.where(u[at] == c, cnt[at], 0) if len(c) else np.zeros(0, dtype=np.int64))
        return out

    def hit_counts(self):
        return np.array([int(w.sum()) for w in self.window_hits()], dtype=np.int64)


def straddlers(wh, edge):
    """queries with a window of two and more entries whose hit ordinals lie on both sides of `edge` (the owner carried over the edge)"""
    out = []
    for q, m in enumerate(wh):
        beg = np.cumsum(m) - m
        if np.any((m >= 2) & (beg < edge) & (beg + m > edge)):
            out.append(q)
    return out


def to_fasta(seqs):
    return b"".join(b">t%04d|p%07d\n%s\n" % (i % 2, i, s.tobytes()) for i, s in enumerate(seqs))


def _iid(rng, n):
    return AA[rng.integers(0, 20, size=n)]


def edge_set(oracle, seed=20260, n_back=560):
    """(fasta, model, roles): about 600 proteins.
      background   n_back iid proteins of 200 .. 300 residues
      edge:<c>     an iid protein of 10 + c residues whose c windows meet nothing but themselves: c hits (EDGE_COUNTS; c = 0: no window at all;
                   c = 1: one hit, a singleton)
      mosaic       11-residue pieces of background proteins one residue apart: every piece one hit alone on its diagonal, beside the
                   protein's own diagonal
      runs         the same with 14-residue pieces: runs of four hits on a diagonal
      copies       one protein five times: 5 entries per window, more than 1024 hits per copy, seeds across every 64-ordinal edge"""
    rng = np.random.default_rng(seed)
    seqs = [_iid(rng, int(rng.integers(200, 301))) for _ in range(n_back)]
    roles = ["background"] * n_back

    def pieces(plen, n):
        out = []
        for _ in range(n):
            src = seqs[int(rng.integers(0, n_back))]
            at = int(rng.integers(0, len(src) - plen + 1))
            out.append(src[at:at + plen])
            out.append(_iid(rng, 1))
        return np.concatenate(out)

    for _ in range(20):
        seqs.append(pieces(11, 20)), roles.append("mosaic")
    for _ in range(20):
        seqs.append(pieces(14, 16)), roles.append("runs")
    big = _iid(rng, 250)
    for _ in range(5):
        seqs.append(big.copy()), roles.append("copies")
    first_edge = len(seqs)
    for c in EDGE_COUNTS:
        seqs.append(_iid(rng, 10 + c)), roles.append("edge:%d" % c)
    m = Model(oracle, seqs)
    for _ in range(64):   # a chance match with another protein (or a masked window) moves a count off its edge: draw that protein again
        got = m.hit_counts()
        off = [first_edge + i for i, c in enumerate(EDGE_COUNTS) if got[first_edge + i] != c]
        if not off:
            break
        for q in off:
            seqs[q] = _iid(rng, len(seqs[q]))
            m.put(q, seqs[q])
    else:
        raise AssertionError("edge proteins keep meeting others")
    return to_fasta(seqs), m, roles


def straddle_set(oracle, seed=20261, n_back=300, edges=(128, 256, 512)):
    """(fasta, model, {edge: query}): per edge one protein whose hits up to ordinal edge - 3 are its own windows' (one each) and whose next
    window has seven entries (six copies of that 11-residue piece sit in six background proteins): a seed whose entries lie on both sides
    of the edge.  Proteins of edge + 40 residues or so: all below 512 residues only for edges up to 460 -- the edge at 512 is reached with
    doubled windows instead (a twin protein: two entries per window)."""
    rng = np.random.default_rng(seed)
    seqs = [_iid(rng, int(rng.integers(200, 301))) for _ in range(n_back)]
    where = {}
    for e in edges:
        twin = e > 400
        per = 2 if twin else 1
        # windows 0 .. nb - 1 hold `per` entries each; window nb (the piece) holds 6 + per: ordinals [per * nb, per * nb + 6 + per)
        nb = (e - 3) // per
        q = _iid(rng, nb + 11 + 30)
        piece = q[nb:nb + 11]
        hosts = rng.choice(n_back, size=6, replace=False)
        for h in hosts:
            s = seqs[int(h)].copy()
            at = int(rng.integers(20, len(s) - 31))
            s[at:at + 11] = piece
            seqs[int(h)] = s
        where[e] = len(seqs)
        seqs.append(q)
        if twin:
            seqs.append(q.copy())
    return to_fasta(seqs), Model(oracle, seqs), where
