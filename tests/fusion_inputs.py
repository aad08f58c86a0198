"""Designed hit tables for the gene-fusion stage (swiftortho_amd/fusion.py), shared by tests/test_fusion.py (CPU: the numpy definition
against the literal loop, the promises of every table) and tests/test_gpu_fusion.py (the device calls against the numpy definition).

A table is built from rows (q, s, qst, qed, sst, sed, slen) over name codes; name k is b'<taxon>|g<k>' with the taxon a fixed-width
number, so the taxon of a name is tax[k] and the .sc text of a table reads back to the same rows (under other codes).  Unless said
otherwise the composite of a run has taxon 0, components taxon 1, a component row covers its whole subject (sst 1, sed slen = 100).
"""
import functools

import numpy as np

from swiftortho_amd import fusion

DEFAULT = dict(max_overlap=0, num=7, den=10, same_taxon=True)
RUN_SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257)
DEVIATIONS = ('overlap', 'one_way', 'last', 'first_row')


class Case:
    """`table`, `tax`, `params` (the keyword arguments of fusion_links) and what the table promises: `links` (a sorted list of (row_a,
    row_b), or None where only the definition says)"""

    def __init__(self, rows, tax, links=None, **params):
        r = np.asarray(rows, dtype=np.int64).reshape(-1, 7)
        tax = np.asarray(tax, dtype=np.int64)
        names = np.asarray([b'%04d|g%07d' % (t, k) for k, t in enumerate(tax.tolist())], dtype='S17') if len(tax) else np.zeros(0, dtype='S1')
        self.table = fusion.Table(names, r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4], r[:, 5], r[:, 6], np.full(len(r), 1000, dtype=np.int64))
        self.tax, self.links, self.params = tax, links, dict(DEFAULT, **params)

    def definition(self):
        return fusion.fusion_links(self.table, self.tax, **self.params)

    def literal(self, deviate=None):
        return fusion.literal_links(self.table, self.tax, deviate=deviate, **self.params)


def row(q, s, qst, qed, sst=1, sed=100, slen=100):
    return (q, s, qst, qed, sst, sed, slen)


class Names:
    """fresh name codes with their taxa"""

    def __init__(self):
        self.tax = []

    def new(self, taxon):
        self.tax.append(taxon)
        return len(self.tax) - 1


def as_pairs(links):
    return list(zip(np.asarray(links.row_a).tolist(), np.asarray(links.row_b).tolist()))


def sc_text(table):
    """the table as 16-column .sc text (the columns the stage does not read hold fixed values)"""
    nm = [x.decode() for x in table.names.tolist()]
    cols = [np.asarray(getattr(table, k)).tolist() for k in ('q', 's', 'qst', 'qed', 'sst', 'sed', 'qlen', 'slen')]
    return ''.join('%s\t%s\t50.00\t100\t50\t0\t%d\t%d\t%d\t%d\t1e-20\t99\t%d\t%d\t0\t0\n' % (nm[q], nm[s], a, b, c, d, ql, sl) for q, s, a, b, c, d, ql, sl in zip(*cols))


HIT_DTYPE = np.dtype([(n, t) for n, t in (("qidx", "<i8"), ("sidx", "<i8"), ("identity", "<f8"), ("evalue", "<f8"), ("aln", "<i4"), ("mis", "<i4"), ("gap", "<i4"),
                                         ("qst", "<i4"), ("qed", "<i4"), ("sst", "<i4"), ("sed", "<i4"), ("bit", "<i4"), ("qlen", "<i4"), ("slen", "<i4"),
                                         ("matches", "<i4"), ("ungapped", "<i4"))])


def records_of(table, seed=0):
    """the table as so_hit records (include/sohit.h) with query / subject id lists that are NOT in name order -> (records, query_ids,
    subject_ids): ordinals and codes differ, the maps of the records call bring them together"""
    assert HIT_DTYPE.itemsize == 80
    rng = np.random.default_rng(seed)
    names = table.names.tolist()
    M = len(names)
    qperm, sperm = rng.permutation(M), rng.permutation(M)
    q_ord, s_ord = np.empty(M, dtype=np.int64), np.empty(M, dtype=np.int64)
    q_ord[qperm], s_ord[sperm] = np.arange(M), np.arange(M)
    rec = np.zeros(len(table), dtype=HIT_DTYPE)
    rec["qidx"], rec["sidx"] = q_ord[table.q], s_ord[table.s]
    for k in ("qst", "qed", "sst", "sed", "qlen", "slen"):
        rec[k] = getattr(table, k)
    return rec, [names[c] for c in qperm], [names[c] for c in sperm]


# ---------------------------------------------------------------------------------------------------------
# single rules
# ---------------------------------------------------------------------------------------------------------
def interval_case(max_overlap):
    """one run per layout of two intervals on the composite; the runs that must link are listed"""
    nm, rows, want = Names(), [], []
    o = max_overlap
    layouts = (('overlap exactly max_overlap', (1, 100), (101 - o, 250), True), ('one residue more', (1, 100), (100 - o, 250), False),
               ('touching', (1, 100), (101, 200), True), ('apart', (1, 100), (150, 200), True), ('nested', (1, 300), (100, 200), False),
               ('identical', (50, 150), (50, 150), False), ('b before a', (201, 300), (1, 200 + o), True),
               ('b before a, one residue more', (201, 300), (1, 201 + o), False), ('one residue each, same', (7, 7), (7, 7), o >= 1),
               ('one residue each, neighbours', (7, 7), (8, 8), True))
    for _, ia, ib, link in layouts:
        q, a, b = nm.new(0), nm.new(1), nm.new(1)
        if link:
            want.append((len(rows), len(rows) + 1))
        rows += [row(q, a, *ia), row(q, b, *ib)]
    return Case(rows, nm.tax, want, max_overlap=max_overlap)


def coverage_case(num, den, slen):
    """per run two components; in run 0 both reach num / den exactly (the least span that does), in run 1 one of them is a residue short"""
    nm, rows = Names(), []
    span = -(-num * slen // den)                   # the least span with span * den >= num * slen
    for short in (0, 1):
        q, a, b = nm.new(0), nm.new(1), nm.new(1)
        rows += [row(q, a, 1, 100, 1, max(span, 1), slen), row(q, b, 101, 200, 1, max(span - short, 1), slen)]
    want = [(0, 1)] if span > 1 else [(0, 1), (2, 3)]     # (a span of one residue cannot be shorter: what -c 0 and slen 0 leave)
    return Case(rows, nm.tax, want, num=num, den=den)


def representative_case():
    """run 0: subject a twice, the first row ineligible (short span) and overlapping b, the second eligible and beside b -> a link that
    'first_row' loses.  run 1: subject c twice, both eligible, the first beside d, the second over d -> a link that 'last' loses.
    runs 2, 3: one query in two runs (another query between them), e in the first and f in the second -> no link; e, f both in run 3 -> one"""
    nm, rows = Names(), []
    q0, a, b = nm.new(0), nm.new(1), nm.new(1)
    rows += [row(q0, a, 150, 250, 1, 10, 100), row(q0, b, 101, 300), row(q0, a, 1, 100)]           # rows 0 1 2: link (1, 2)
    q1, c, d = nm.new(0), nm.new(1), nm.new(1)
    rows += [row(q1, c, 1, 100), row(q1, d, 101, 200), row(q1, c, 120, 220)]                       # rows 3 4 5: link (3, 4)
    q2, e, f, other = nm.new(0), nm.new(1), nm.new(1), nm.new(0)
    rows += [row(q2, e, 1, 100), row(other, e, 1, 100), row(q2, f, 101, 200), row(q2, e, 1, 90)]   # rows 6 | 7 | 8 9: link (8, 9)
    return Case(rows, nm.tax, [(1, 2), (3, 4), (8, 9)])


def homology_case():
    """five composites, each with two components side by side; a row elsewhere decides: a -> b only, b -> a only, both, neither, and a row
    a -> b that is itself ineligible (a short span; the same taxon) and stands 600 rows away"""
    nm, rows, want, late = Names(), [], [], []
    for kind in ('ab', 'ba', 'both', 'neither', 'far'):
        q, a, b = nm.new(0), nm.new(1), nm.new(1)
        if kind == 'neither':
            want.append((len(rows), len(rows) + 1))
        rows += [row(q, a, 1, 100), row(q, b, 101, 200)]
        if kind in ('ab', 'both', 'far'):
            late.append(row(a, b, 1, 50, 1, 5, 100))          # (ineligible twice over: it is still a row of the table)
        if kind in ('ba', 'both'):
            late.append(row(b, a, 1, 50, 1, 5, 100))
    filler = nm.new(2)
    for _ in range(600):
        rows.append(row(filler, nm.new(2), 1, 100))
    return Case(rows + late, nm.tax, want)


def taxon_case(same_taxon):
    """run 0: both components of the composite's own taxon; run 1: components of two taxa; run 2: as the rule wants them"""
    nm, rows = Names(), []
    for ta, tb in ((0, 0), (1, 2), (1, 1)):
        q, a, b = nm.new(0), nm.new(ta), nm.new(tb)
        rows += [row(q, a, 1, 100), row(q, b, 101, 200)]
    return Case(rows, nm.tax, [(4, 5)] if same_taxon else [(0, 1), (2, 3), (4, 5)], same_taxon=same_taxon)


def self_hit_case():
    """the composite's own row never is a component"""
    nm = Names()
    q, a = nm.new(0), nm.new(1)
    return Case([row(q, q, 1, 100), row(q, a, 101, 200)], nm.tax, [], same_taxon=False)


def dense_case(m=64):
    """one run of m pairwise disjoint intervals: every pair is a link"""
    nm = Names()
    q = nm.new(0)
    rows = [row(q, nm.new(1), 10 * k + 1, 10 * k + 10) for k in range(m)]
    return Case(rows, nm.tax, [(i, j) for i in range(m) for j in range(i + 1, m)])


def no_eligible_case():
    nm = Names()
    q = nm.new(0)
    return Case([row(q, nm.new(1), 10 * k + 1, 10 * k + 10, 1, 10, 100) for k in range(5)], nm.tax, [])


def no_link_case():
    nm = Names()
    q = nm.new(0)
    return Case([row(q, nm.new(1), 1 + k, 100 + k) for k in range(40)], nm.tax, [])


def empty_case():
    return Case([], [], [])


# ---------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------
def _random_run(rng, rows, q, subjects, m_rows, qlen=2000, short=.2):
    """m_rows rows of query q over `subjects` (drawn with repeats), a share of them with a span too short to be eligible"""
    s = rng.choice(subjects, m_rows)
    qst = rng.integers(1, qlen - 300, m_rows)
    qed = qst + rng.integers(20, 300, m_rows)
    cut = rng.random(m_rows) < short
    for k in range(m_rows):
        rows.append(row(q, int(s[k]), int(qst[k]), int(qed[k]), 1, 40 if cut[k] else 100, 100))


@functools.lru_cache(maxsize=None)
def run_sizes_case():
    """runs with exactly RUN_SIZES representatives (every subject once and eligible, between ineligible rows of subjects already seen),
    over a pool of 300 components of 3 taxa, some of them homologous through rows of their own at the end"""
    rng = np.random.default_rng(11)
    nm, rows = Names(), []
    pool = [nm.new(1 + k % 3) for k in range(300)]
    for m in RUN_SIZES:
        q = nm.new(0)
        sub = rng.permutation(pool)[:m]
        if m == 0:
            rows.append(row(q, pool[0], 1, 100, 1, 10, 100))
        for k, s in enumerate(sub.tolist()):
            st = int(rng.integers(1, 3000))
            rows.append(row(q, s, st, st + int(rng.integers(10, 200))))
            if k % 7 == 3:
                rows.append(row(q, int(sub[k // 2]), 1, 5000))          # a second row of a subject seen before: never a representative
    for _ in range(2000):
        a, b = rng.choice(pool, 2).tolist()
        rows.append(row(a, b, 1, 100, 1, 5, 100))                       # (a short span: homology without a representative)
    return Case(rows, nm.tax)


@functools.lru_cache(maxsize=None)
def long_run_case(m=3000):
    """one run of m representatives of 50 taxa (m (m - 1) / 2 pairs, a fiftieth of them of one taxon) and 3000 homology rows"""
    rng = np.random.default_rng(12)
    nm, rows = Names(), []
    q = nm.new(0)
    pool = [nm.new(1 + k % 50) for k in range(m)]
    st = rng.integers(1, 30000, m)
    for k, s in enumerate(pool):
        rows.append(row(q, s, int(st[k]), int(st[k]) + 150))
    for _ in range(3000):
        a = int(rng.integers(0, m))
        b = a + 50 * int(rng.integers(-3, 4))
        if 0 <= b < m and b != a:
            rows.append(row(pool[a], pool[b], 1, 100))
    return Case(rows, nm.tax)


@functools.lru_cache(maxsize=None)
def short_runs_case(n_runs=20000):
    """n_runs runs of 1 .. 5 rows over 4000 names of 4 taxa, every name a query and a subject"""
    rng = np.random.default_rng(13)
    nm, rows = Names(), []
    pool = [nm.new(k % 4) for k in range(4000)]
    for _ in range(n_runs):
        _random_run(rng, rows, int(rng.choice(pool)), pool, int(rng.integers(1, 6)), short=.1)
    return Case(rows, nm.tax, max_overlap=30)


@functools.lru_cache(maxsize=None)
def random_case(seed):
    """a seeded table: 60 names of 4 taxa, runs of 1 .. 40 rows, parameters drawn too"""
    rng = np.random.default_rng(seed)
    nm, rows = Names(), []
    pool = [nm.new(k % 4) for k in range(60)]
    for _ in range(int(rng.integers(1, 40))):
        _random_run(rng, rows, int(rng.choice(pool)), pool, int(rng.integers(1, 41)), qlen=900, short=.3)
    return Case(rows, nm.tax, max_overlap=int(rng.choice([0, 0, 5, 50])), num=int(rng.choice([0, 1, 7])), den=10, same_taxon=bool(rng.integers(0, 2)))


AA = np.frombuffer(b'ACDEFGHIKLMNPQRSTVWY', dtype=np.uint8)
COMPOSITE = b'Y|C'
COMPONENT_PAIRS = {(b'X|A', b'X|B'), (b'Z|A', b'Z|B')}
UNRELATED = (b'X|U1', b'Y|U2', b'Z|U3', b'W|U4', b'W|U5')


def fusion_fasta(seed=7, length=300, rate=.1):
    """a proteome with one fusion: taxon X holds unrelated A and B of `length` residues, Y holds C -- a copy of A followed by one of B,
    each with a share `rate` of its residues replaced --, Z holds such copies of A and B apart, and five unrelated proteins stand about
    -> FASTA bytes.  The links at the defaults are C with (X|A, X|B) and C with (Z|A, Z|B), and no other protein is a composite."""
    rng = np.random.default_rng(seed)
    draw = lambda: AA[rng.integers(0, 20, length)]

    def copy(x):
        y = x.copy()
        at = rng.permutation(len(x))[:int(len(x) * rate)]
        y[at] = AA[(np.searchsorted(AA, x[at]) + rng.integers(1, 20, len(at))) % 20]       # another residue, always
        return y

    A, B = draw(), draw()
    recs = [(b'X|A', A), (b'X|B', B), (COMPOSITE, np.concatenate([copy(A), copy(B)])), (b'Z|A', copy(A)), (b'Z|B', copy(B))]
    recs += [(u, draw()) for u in UNRELATED]
    return b''.join(b'>' + n + b'\n' + s.tobytes() + b'\n' for n, s in recs)


def designed():
    """name -> Case: every small designed table (those with `links` promise them)"""
    out = {'interval, max_overlap 0': interval_case(0), 'interval, max_overlap 5': interval_case(5),
           'coverage 7/10 of 100': coverage_case(7, 10, 100), 'coverage 7/10 of 101': coverage_case(7, 10, 101),
           'coverage (2^20 - 2) / (2^20 - 1) of 2^31 - 2': coverage_case((1 << 20) - 2, (1 << 20) - 1, (1 << 31) - 2),
           'coverage 1/1 of 2^31 - 2': coverage_case(1, 1, (1 << 31) - 2), 'coverage 0 of 0': coverage_case(0, 1, 0),
           'representatives': representative_case(), 'homology': homology_case(), 'taxon rule on': taxon_case(True), 'taxon rule off': taxon_case(False),
           'self hit': self_hit_case(), 'dense': dense_case(), 'no eligible row': no_eligible_case(), 'no link': no_link_case(), 'empty': empty_case()}
    return out


# the input that catches each single deviation of the literal model
CATCHES = {'overlap': 'interval, max_overlap 0', 'one_way': 'homology', 'last': 'representatives', 'first_row': 'representatives'}
