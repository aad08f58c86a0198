"""Designed inputs of the gene-content tests (tests/test_pan_content.py, tests/test_gpu_pan_content.py) and the literal model the numpy
definitions of swiftortho_amd/pan.py are held to: presence tables, their member pairs, the text of small FASTA and groups files.

The ramp table: a seeded random presence table whose per-taxon density rises linearly from 0.1 to 0.9 -- no two genomes look alike, so
a shifted or swapped tile cannot hide in a symmetric matrix.  At the sizes of RAMP_CHECKED no two rows of S are equal and no denominator
of either metric is 0; ramp_facts() asserts that on the numpy result before a test compares anything with it."""
import numpy as np

RAMP_CHECKED = ((65, 65), (130, 129), (200, 193))


def ramp(R, T):
    """-> int32[R, T] presence (0 / 1)"""
    return (np.random.RandomState(7).rand(R, T) < np.linspace(.1, .9, T)).astype(np.int32)


def ramp_facts(S):
    """what makes the ramp table a test: every genome's row of S differs from every other's, and neither metric meets a denominator of 0"""
    S = np.asarray(S)
    d = np.diagonal(S)
    assert len({r.tobytes() for r in S}) == len(S)
    assert ((d[:, None] + d[None, :] - S) > 0).all() and (np.minimum(d[:, None], d[None, :]) > 0).all()


def members(counts):
    """count table -> (row, taxon) int32: every cell as often as it counts, in an order that is not the table's"""
    counts = np.asarray(counts)
    r, t = np.nonzero(counts)
    rep = counts[r, t]
    r, t = np.repeat(r, rep), np.repeat(t, rep)
    order = np.random.RandomState(11).permutation(len(r))
    return r[order].astype(np.int32), t[order].astype(np.int32)


def table_of(pan, counts):
    counts = np.asarray(counts)
    r, t = members(counts)
    return pan.MemberTable(r, t, counts.shape[0], counts.shape[0])


def loop_shared(counts, rows=None):
    """S by a literal triple loop over (row, a, b); rows: the drawn rows of a replicate, each as often as it is drawn"""
    x = (np.asarray(counts) > 0).tolist()
    T = len(x[0]) if x else np.asarray(counts).shape[1]
    S = [[0] * T for _ in range(T)]
    for r in (range(len(x)) if rows is None else rows):
        for a in range(T):
            if x[r][a]:
                for b in range(T):
                    if x[r][b]:
                        S[a][b] += 1
    return np.asarray(S, dtype=np.int64).reshape(T, T)


# ---- hand tables -------------------------------------------------------------------------------------------------------------------------
ZERO_GENOME = np.array([[1, 1, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=np.int32)      # genome 2 holds no family
ONE_ROW = np.array([[1, 0, 0]], dtype=np.int32)                                             # 1 x 3: genomes 1 and 2 are empty
TWINS = np.array([[1, 1, 0], [1, 1, 1], [0, 0, 1], [1, 1, 0], [2, 1, 1]], dtype=np.int32)  # genomes 0 and 1 are identical; row 1 and 4 are held by all
LISTED_TWICE = np.array([[2, 1], [0, 3], [1, 0]], dtype=np.int32)                            # counts above 1 are one presence


def planted(n_a=4, n_b=5, core=12, acc=25, own=3, seed=3):
    """two groups of genomes with disjoint accessory families: `core` rows held by everyone, `acc` rows held by (most of) group A only
    and as many by group B only, `own` rows per genome of its own.  Every accessory row misses at most one genome of its group, so the
    split A | B is in the tree of the table and of every bootstrap replicate that keeps a good part of the rows -> (counts, group A)"""
    rng = np.random.RandomState(seed)
    T = n_a + n_b
    rows = [np.ones(T, dtype=np.int32) for _ in range(core)]
    for lo, hi in ((0, n_a), (n_a, T)):
        for _ in range(acc):
            r = np.zeros(T, dtype=np.int32)
            r[lo:hi] = 1
            if rng.rand() < .5:
                r[rng.randint(lo, hi)] = 0
            rows.append(r)
    for t in range(T):
        for _ in range(own):
            r = np.zeros(T, dtype=np.int32)
            r[t] = 1
            rows.append(r)
    counts = np.stack(rows)
    return counts[rng.permutation(len(counts))], list(range(n_a))


def with_rare_genome(R=70, T=6):
    """a ramp table and one more genome that holds a single family: a replicate that does not draw that row leaves the genome empty and
    is dropped (about a third of them), the others are kept"""
    counts = np.concatenate([ramp(R, T), np.zeros((R, 1), dtype=np.int32)], 1)
    counts[R // 2, T] = 1
    return counts


def lonely(T=8):
    """every genome holds one family of its own: a replicate is kept only when it draws every row"""
    return np.eye(T, dtype=np.int32)


# ---- files -------------------------------------------------------------------------------------------------------------------------------
def names_of(T):
    """taxon names whose sorted order is a seeded shuffle of their code order"""
    return ['g%03d' % k for k in np.random.RandomState(100 + T).permutation(T)]


def files_of(counts, names, n_file_rows=None):
    """count table -> (fasta text, groups text): gene ids taxon|r<row>_<copy>; the rows from n_file_rows on are single genes that no
    group line lists (each holds exactly one member).  Every taxon needs a gene: the script knows a taxon by its headers"""
    counts = np.asarray(counts)
    R, T = counts.shape
    assert (counts.sum(0) > 0).all()
    n_file = R if n_file_rows is None else n_file_rows
    fasta, groups = [], []
    for r in range(R):
        ids = ['%s|r%d_%d' % (names[t], r, c) for t in range(T) for c in range(counts[r, t])]
        fasta += ['>%s\nMKV\n' % i for i in ids]
        assert ids
        if r < n_file:
            groups.append('\t'.join(ids) + '\n')
        else:
            assert len(ids) == 1
    return ''.join(fasta), ''.join(groups)


# the one way to a genome without a family through the script: the reference cuts the LAST character off a header line, whatever it is, so
# a last line `>ab` without a newline names taxon `a` -- while its record id, `ab`, is a gene of taxon `ab`
EMPTY_TAXON_FASTA = '>ab|g1\nMKV\n>cd|g1\nMKV\n>ab'
EMPTY_TAXON_GROUPS = 'ab|g1\tcd|g1\n'
