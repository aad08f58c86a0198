"""phy -- the second half of SwiftOrtho's scripts/rbh2phy.py without its external programs: from the core-gene families and the hits'
OWN alignments to the core-gene supermatrix, the distances between the taxa over it and a neighbour-joining tree.

The reference writes one FASTA file per core family, shells out to an aligner (famsa | mafft | muscle), joins the alignments, and hands
the join to trimal and fasttree.  No aligner is needed: every member of a core family is the best hit of the family's anchor gene (the
reference taxon's gene) in its taxon, and the search has aligned exactly that pair.  With CIGARs on the rows (Searcher.search(cigar=True),
find_hit.py -C T) the member is laid onto the anchor's coordinates -- the centre-star alignment with the insertions against the centre
dropped, what `mmseqs result2msa` builds.  There is no reference output to match (the reference's result is whatever its aligner and tree
program print): the definitions are the numpy functions of this module, and the device calls (include/sohit.h so_phy_rows, so_phy_build;
csrc/phy.hip) equal them array for array.

  * pick_rows: for every wanted (anchor, member) pair the row with q == anchor, s == member and the highest score, ties to the lowest
    row, -1 when there is none; rows need not be grouped; a NaN score refuses the call.  A query of 4096 residues and more has one row per
    tile: the best tile is picked, only that tile is projected, the rest of the block stays gaps.
  * families: rbh.core_groups unchanged -- family k's anchor is table.genes[k], its members the flagged ids, one per slot at most.  A
    member equal to the anchor needs no row: its residues are the block's row.  With -r naming another taxon than the largest the
    reference's quirk leaves the anchor out of its own family: it still gives the block its coordinates, no taxon gets its residues.
  * project: the row starts as '-'; from query position qst - 1 and subject position sst - 1 an M run copies member residues, an I run
    leaves its columns '-', a D run drops its residues.  Residues are the FASTA record's bytes (rbh.fasta_records): no folding, no mask.
  * supermatrix: matrix[T, L] (uint8), T = the FASTA's taxa in slot order (rbh.fasta_taxa), L = the anchors' lengths in family order
    (col_off[F + 1]); a taxon without a member in a family is '-' over the block (the reference's `empty`); gaps[L] = '-' per column;
    keep = the ascending columns with gaps <= floor(g * T) (g = 1: everything, the reference without trimal).
  * pair_counts: cmp[a, b] = kept columns where neither row is '-', same[a, b] = those where the bytes are equal; diagonal included.
  * host only: distances (p = 1 - same / cmp; poisson: -log(1 - p)), neighbor_joining (Saitou-Nei, float64, Newick with %.6f) and
    supermatrix_fasta (`>taxon\\nrow\\n` per taxon in SLOT order; the reference prints in the iteration order of a set).
  * bootstrap support (off unless asked for; the reference gets it from `fasttree -boot`): replicate b draws the K kept columns with
    replacement (boot_columns: splitmix64 of (b, k), scaled by a multiply and a shift), its pair counts (boot_counts) give distances
    (boot_distances: distances() that drops the replicate where it would refuse) and a topology (nj_splits: the T - 3 clades the joins
    make, as bit sets over the taxa, the side without taxon 0).  nj_splits is neighbor_joining's walk with SEQUENTIAL row sums -- the
    one summation order a GPU lane reproduces bit for bit; the printed tree keeps its own summation (tree_splits hands out its
    clades), so the supports always refer to the tree that is printed.  split_support counts, per clade of the printed tree, the kept
    replicates that hold it; bootstrap -> (count, valid); tree(boot=B) labels the nodes with count / valid, %.3f.  On the device
    (so_phy_boot_counts, so_phy_nj_splits, so_phy_boot) the counts are integers and the walks the same IEEE operations in the same
    order: every array equals numpy's.
  * substitution counts (pair_index, subst_counts, boot_subst): per pair of taxa i < j the 20 x 20 table N[a, b] of the kept columns where
    taxon i holds residue a and taxon j residue b (AA20 order; any other byte is uncoded and adds nothing).  Two more distances follow,
    neither of which needs a rate matrix: kimura, -log(1 - p - p * p / 5) from the pair counts, and logdet (Lake; Lockhart et al.),
    -(log det N - (sum log r + sum log c) / 2) / 20 with r, c the row and column sums of N, additive under a general Markov model,
    composition bias included.  The tensor is N = E E^T of one-hot matrices: on the device (so_phy_subst) a product on the matrix cores
    in 32-bit integers; determinants and logarithms stay numpy's, so the distances are the same bytes with and without the device.
  * gene concordance factors (off unless asked for; the reference has nothing like it -- its alignments come from an external aligner):
    for every inner branch of the printed tree the share of the single-family trees, among the families that can decide the branch, that
    hold it.  Family f owns keep[r[f]:r[f + 1]] (family_ranges: searchsorted(keep, col_off)); family_counts = pair_counts per family;
    taxon t is PRESENT in f iff cmp[f, t, t] > 0 (family_present: bit sets in slot order) -- a family may lack a tenth of the taxa;
    gene_distances = boot_distances among the present taxa (p, poisson, kimura; logdet is refused: a family's block is where it has no
    distance); nj_splits_subset = nj_splits over the present taxa with the bits in their original slots, the canonical side the one
    without the LOWEST PRESENT taxon, rows n - 3 .. zero.  concordance: for clade C of the printed tree (tree_splits) and present set P,
    A = C & P and B = P & ~C; the family is decisive iff both hold two taxa at least, concordant iff decisive and its tree holds the one
    of A and B without P's lowest taxon; a family in which a present pair has no distance is dropped.  gene_concordance ->
    (decisive, concordant, ok, n_present, splits); tree(concordance=True) labels join t with concordant[t] / decisive[t] (%.3f, NA where
    nobody decides, boot/gcf with boot > 0); gcf_table is what rbh2phy.py -k writes.  On the device (so_phy_gene for p: gather, pair counts
    per (tile, family), distances and presence, the bootstrap's walk started from the present bits, a (split, family) grid of popcounts
    and integer atomics, batches with one host wait each; so_phy_gene_counts and so_phy_nj_subsets for poisson and kimura, whose logarithm
    stays on the host with the printed tree's walk) only integers and bit sets come back: every array equals numpy's.  Refused: T outside
    2 .. 4096, offsets that do not rise from 0 to the kept columns, a kept column out of range, unknown flags, no device.

The module imports `_lib` (ctypes declarations only: the library itself is loaded by the first device call), so the numpy definitions need
no built library and no device.
"""
import math
import sys

import numpy as np

from . import _lib, rbh

GAP = 45   # '-'
_arr = _lib.result_array


def _call(fn, result, free, *args):
    """a device call of this module (_lib.call): a `with` block around the result; a refusal raises RuntimeError with the library's message"""
    return _lib.call(fn, getattr(_lib, result), free, 'so_phy_last_error', *args)


class Supermatrix:
    """`taxa` (bytes, slot order), `matrix` uint8[T, L] (None when a device call was asked for the counts only), `col_off` int64[F + 1],
    `gaps` int32[L], `keep` int64[L'], `cmp` / `same` int64[T, T] over the kept columns, `anchors` (name codes, family order), `stats`;
    `subst` int32[P, 20, 20]: the substitution counts over the kept columns, None until a model asks for them (tree(), model logdet)"""
    subst = None

    def __init__(self, taxa, matrix, col_off, gaps, keep, cmp, same, anchors=None, stats=None):
        self.taxa, self.matrix, self.col_off, self.gaps, self.keep, self.cmp, self.same = taxa, matrix, col_off, gaps, keep, cmp, same
        self.anchors, self.stats = anchors, stats or {}


# ---------------------------------------------------------------------------------------------------------
# the rows
# ---------------------------------------------------------------------------------------------------------
def _pair_keys(a, b):
    return (np.asarray(a, dtype=np.int64) << 32) | np.asarray(b, dtype=np.int64)


def pick_rows(cols_q, cols_s, score, pair_q, pair_s):
    """-> int64[n_pairs]: per wanted pair the row with q == pair_q, s == pair_s and the highest score (the lowest such row), or -1"""
    q, s = np.asarray(cols_q, dtype=np.int64), np.asarray(cols_s, dtype=np.int64)
    sco = np.asarray(score, dtype=np.float64)
    pq, ps = np.asarray(pair_q, dtype=np.int64), np.asarray(pair_s, dtype=np.int64)
    if not (len(q) == len(s) == len(sco)) or len(pq) != len(ps):
        raise ValueError('pick_rows: the columns differ in length')
    if len(sco) and np.isnan(sco).any():
        raise ValueError('pick_rows: row %d has a NaN score' % int(np.flatnonzero(np.isnan(sco))[0]))
    if len(pq) and (pq.min() < 0 or ps.min() < 0):
        raise ValueError('pick_rows: a wanted pair holds a negative name code')
    out = np.full(len(pq), -1, dtype=np.int64)
    if len(q) == 0 or len(pq) == 0:
        return out
    want = _pair_keys(pq, ps)
    rows = np.flatnonzero((q >= 0) & (s >= 0))
    key = _pair_keys(q[rows], s[rows])
    rows = rows[np.isin(key, want)]
    if len(rows) == 0:
        return out
    key = _pair_keys(q[rows], s[rows])
    order = np.lexsort((rows, -sco[rows], key))   # per key the largest score first, equal scores (0.0 and -0.0 too) by row
    sk = key[order]
    head = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))
    uk, best = sk[head], rows[order[head]]
    at = np.minimum(np.searchsorted(uk, want), len(uk) - 1)
    hit = uk[at] == want
    out[hit] = best[at[hit]]
    return out


def device_pick_rows(cols_q, cols_s, score, pair_q, pair_s, device=0):
    """pick_rows() on the GPU (so_phy_rows); a refusal raises RuntimeError with the library's message"""
    q32, s32 = _codes32(cols_q, 'device_pick_rows'), _codes32(cols_s, 'device_pick_rows')
    sco = np.ascontiguousarray(score, dtype=np.float64)
    pq, ps = _codes32(pair_q, 'device_pick_rows'), _codes32(pair_s, 'device_pick_rows')
    if not (len(q32) == len(s32) == len(sco)) or len(pq) != len(ps):
        raise ValueError('device_pick_rows: the columns differ in length')
    with _call('so_phy_rows', 'SoPhyResult', 'so_phy_free', int(device), len(q32), q32, s32, sco, len(pq), pq, ps, 0) as out:
        return _arr(out.row, len(pq), np.int64)


def _codes32(a, who):
    a = np.asarray(a)
    if len(a) and (int(a.max()) > 2 ** 31 - 1 or int(a.min()) < -2 ** 31):
        raise ValueError('%s: a name code does not fit 32 bits' % who)
    return np.ascontiguousarray(a, dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------
# families and projection
# ---------------------------------------------------------------------------------------------------------
def families(table, min_share=.9):
    """CoreTable -> [(anchor code, [(slot, member code), ...])] for the groups rbh.core_groups keeps, in its order (the same assembly, with
    the slots kept).  min_share: the share of the taxa a kept group holds at least -- the reference's 0.9; only measurements change it"""
    nt = len(table.slots)
    out = []
    for g, fwd, rec in zip(np.asarray(table.genes).tolist(), np.asarray(table.fwd).tolist(), np.asarray(table.rec).tolist()):
        ids, flag = [-1] * nt, [0] * nt
        ids[0], flag[0] = g, 1
        for t in range(nt):
            if fwd[t] >= 0:
                ids[t] = fwd[t]
            if rec[t]:
                flag[t] = 1
        mem = [(t, i) for t, (i, f) in enumerate(zip(ids, flag)) if f == 1]
        if len(mem) * 1. / nt >= min_share:
            out.append((g, mem))
    return out


def pack_runs(runs):
    """[(length, op)] with op in 'MID' or 0 / 1 / 2 -> uint32 runs, length << 4 | op"""
    code = {'M': 0, 'I': 1, 'D': 2, 0: 0, 1: 1, 2: 2}
    return np.asarray([(int(n) << 4) | code[op] for n, op in runs], dtype=np.uint32)


def project(anchor_len, member_seq, qst, sst, runs, what='the row'):
    """-> bytes[anchor_len]: the member on its anchor's coordinates; `runs`: uint32, length << 4 | op (0 M, 1 I, 2 D).  A row that leaves
    either sequence, or holds a run of length 0 or an unknown operation, is refused (ValueError naming `what`)."""
    member_seq = bytes(member_seq)
    qst, sst, anchor_len = int(qst), int(sst), int(anchor_len)
    if qst < 1 or sst < 1:
        raise ValueError('project: %s starts before the first residue (qst %d, sst %d)' % (what, qst, sst))
    rl = [(int(v) >> 4, int(v) & 15) for v in np.asarray(runs).tolist()]
    for n, op in rl:
        if n == 0 or op > 2:
            raise ValueError('project: %s has a run of length 0 or of an unknown operation' % what)
    if qst - 1 + sum(n for n, op in rl if op != 2) > anchor_len:
        raise ValueError('project: the runs of %s lead past the anchor (%d residues)' % (what, anchor_len))
    if sst - 1 + sum(n for n, op in rl if op != 1) > len(member_seq):
        raise ValueError('project: the runs of %s lead past the member (%d residues)' % (what, len(member_seq)))
    out = bytearray(b'-' * anchor_len)
    qp, sp = qst - 1, sst - 1
    for n, op in rl:
        if op == 0:
            out[qp:qp + n] = member_seq[sp:sp + n]
            qp, sp = qp + n, sp + n
        elif op == 1:
            qp += n
        else:
            sp += n
    return bytes(out)


class Tasks:
    """What so_phy_build reads: `n_taxa`, `col_off` int64[F + 1], and per (family, slot) task `fam`, `slot` (int32), `kind` (uint8: 1 = the
    anchor itself, 0 = a member to project), `res_off` (int64) / `res_len` (int32) into `residues` (uint8), `qst`, `sst` (int32, 1-based as
    printed), `run_off` int64[n + 1] into `runs` (uint32).  `label[t]`: how a message names task t."""

    def __init__(self, n_taxa, col_off, fam, slot, kind, res_off, res_len, qst, sst, run_off, runs, residues, label=None):
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
        self.n_taxa, self.col_off = int(n_taxa), i64(col_off)
        self.fam, self.slot, self.kind = i32(fam), i32(slot), np.ascontiguousarray(kind, dtype=np.uint8)
        self.res_off, self.res_len, self.qst, self.sst = i64(res_off), i32(res_len), i32(qst), i32(sst)
        self.run_off, self.runs = i64(run_off), np.ascontiguousarray(runs, dtype=np.uint32)
        self.residues = np.ascontiguousarray(np.frombuffer(bytes(residues), dtype=np.uint8) if isinstance(residues, (bytes, bytearray)) else residues, dtype=np.uint8)
        self.label = label
        n = len(self.fam)
        if not (len(self.slot) == len(self.kind) == len(self.res_off) == len(self.res_len) == len(self.qst) == len(self.sst) == n) or len(self.run_off) != n + 1:
            raise ValueError('Tasks: the task columns differ in length')

    def name(self, t):
        return self.label[t] if self.label else 'task %d (family %d, slot %d)' % (t, self.fam[t], self.slot[t])


def _check_tasks(tk, g):
    """what the device call refuses before it touches the device (the same words where a test reads them)"""
    F = len(tk.col_off) - 1
    if tk.n_taxa <= 0:
        raise ValueError('supermatrix: no taxa')
    if F <= 0:
        raise ValueError('supermatrix: no families')
    if not (0. <= g <= 1.):
        raise ValueError('supermatrix: the gap share must lie in [0, 1]')
    if tk.col_off[0] != 0 or (np.diff(tk.col_off) < 0).any():
        raise ValueError('supermatrix: inconsistent offsets: col_off does not rise from 0')
    if int(tk.col_off[-1]) > 2 ** 31 - 1:
        raise ValueError('supermatrix: more than 2^31 - 1 columns are not supported')
    n = len(tk.fam)
    if n == 0:
        return
    if tk.fam.min() < 0 or tk.fam.max() >= F or tk.slot.min() < 0 or tk.slot.max() >= tk.n_taxa:
        raise ValueError('supermatrix: a task names a family or a slot out of range')
    if tk.run_off[0] != 0 or (np.diff(tk.run_off) < 0).any() or tk.run_off[-1] != len(tk.runs):
        raise ValueError('supermatrix: inconsistent offsets: run_off does not rise from 0 to the number of runs')
    if (tk.res_off < 0).any() or (tk.res_len < 0).any() or (tk.res_off + tk.res_len > len(tk.residues)).any():
        raise ValueError('supermatrix: inconsistent offsets: residues outside the residue blob')
    cell = tk.fam.astype(np.int64) * tk.n_taxa + tk.slot
    if len(np.unique(cell)) != n:
        raise ValueError('supermatrix: two tasks fill one (family, slot) block')


def gap_limit(g, n_taxa):
    """the most '-' a kept column holds: floor(g * T)"""
    return int(math.floor(float(g) * n_taxa))


def fill_matrix(tk):
    """Tasks -> matrix uint8[T, L] by project(), task by task"""
    L = int(tk.col_off[-1])
    matrix = np.full((tk.n_taxa, L), GAP, dtype=np.uint8)
    res = tk.residues.tobytes()
    for t in range(len(tk.fam)):
        c0, c1 = int(tk.col_off[tk.fam[t]]), int(tk.col_off[tk.fam[t] + 1])
        seq = res[int(tk.res_off[t]):int(tk.res_off[t]) + int(tk.res_len[t])]
        if tk.kind[t]:
            if len(seq) != c1 - c0:
                raise ValueError('supermatrix: %s is the anchor, and its residues are not as many as the family\'s columns' % tk.name(t))
            row = seq
        else:
            row = project(c1 - c0, seq, tk.qst[t], tk.sst[t], tk.runs[int(tk.run_off[t]):int(tk.run_off[t + 1])], tk.name(t))
        matrix[tk.slot[t], c0:c1] = np.frombuffer(row, dtype=np.uint8)
    return matrix


def column_gaps(matrix):
    """-> int32[L]: '-' per column"""
    return (np.asarray(matrix) == GAP).sum(0).astype(np.int32)


def kept_columns(gaps, g, n_taxa):
    """-> int64[L']: the ascending columns with gaps <= floor(g * T)"""
    if not (0. <= g <= 1.):
        raise ValueError('supermatrix: the gap share must lie in [0, 1]')
    return np.flatnonzero(np.asarray(gaps) <= gap_limit(g, n_taxa)).astype(np.int64)


def pair_counts(matrix, keep):
    """-> (cmp, same) int64[T, T] over the kept columns.  One product per byte value present, in float32 over at most 2^20 columns at a
    time: every partial count is an integer below 2^24, so the sums are exact."""
    matrix = np.asarray(matrix, dtype=np.uint8)
    T = matrix.shape[0]
    cmp_, same = np.zeros((T, T), dtype=np.int64), np.zeros((T, T), dtype=np.int64)
    keep = np.asarray(keep, dtype=np.int64)
    for c0 in range(0, len(keep), 1 << 20):
        K = matrix[:, keep[c0:c0 + (1 << 20)]]
        ng = (K != GAP).astype(np.float32)
        cmp_ += np.rint(ng @ ng.T).astype(np.int64)
        for v in np.unique(K).tolist():
            if v == GAP:
                continue
            e = (K == v).astype(np.float32)
            same += np.rint(e @ e.T).astype(np.int64)
    return cmp_, same


def build(tk, g=1.0):
    """Tasks -> (matrix, gaps, keep, cmp, same) by the numpy definitions"""
    _check_tasks(tk, g)
    matrix = fill_matrix(tk)
    gaps = column_gaps(matrix)
    keep = kept_columns(gaps, g, tk.n_taxa)
    cmp_, same = pair_counts(matrix, keep)
    return matrix, gaps, keep, cmp_, same


def device_build(tk, g=1.0, want_matrix=True, device=0, out=None, stats=None):
    """build() in one device call (so_phy_build) -> (matrix or None, gaps, keep, cmp, same); a refusal raises RuntimeError with the
    library's message.  `out`: a uint8[T, L] array of the caller's that receives the matrix too -- a refused call leaves it untouched."""
    F, n = len(tk.col_off) - 1, len(tk.fam)
    with _call('so_phy_build', 'SoPhyResult', 'so_phy_free', int(device), tk.n_taxa, F, tk.col_off, n, tk.fam, tk.slot, tk.kind, tk.res_off, tk.res_len, tk.qst, tk.sst,
               tk.run_off, tk.runs, len(tk.runs), tk.residues, len(tk.residues), float(g), 0 if want_matrix else 1) as res:
        T, nc, nk = tk.n_taxa, int(res.n_cols), int(res.n_keep)
        matrix = _arr(res.matrix, T * nc, np.uint8).reshape(T, nc) if want_matrix else None
        if out is not None and matrix is not None:
            out[...] = matrix
        if stats is not None:
            stats['waits'] = int(res.waits)
        return (matrix, _arr(res.gaps, nc, np.int32), _arr(res.keep, nc, np.int64)[:nk], _arr(res.cmp, T * T, np.int64).reshape(T, T),
                _arr(res.same, T * T, np.int64).reshape(T, T))


# ---------------------------------------------------------------------------------------------------------
# where the rows come from: the records of a search with CIGARs, or the text of a 17-column .sc file
# ---------------------------------------------------------------------------------------------------------
class RecordRows:
    """the rows of a search with cigar=True: `cols` (find_orth.columns_from_records of the records), the records' qst / sst and
    Hits.cigar_buffer()"""

    def __init__(self, cols, qst, sst, ops, off):
        self.q, self.s, self.score = cols.q, cols.s, cols.score
        self._qst, self._sst, self._ops, self._off = qst, sst, ops, off

    def alignment(self, rows):
        """-> (qst, sst, [runs]) of the chosen rows"""
        rows = np.asarray(rows, dtype=np.int64)
        return (np.asarray(self._qst)[rows].astype(np.int64), np.asarray(self._sst)[rows].astype(np.int64),
                [np.array(self._ops[int(self._off[r]):int(self._off[r + 1])], dtype=np.uint32) for r in rows.tolist()])


class MissingCigar(ValueError):
    pass


class TextRows:
    """the rows of a find_hit .sc file with a 17th column (find_hit.py -C T): ids and score (column 12) of every line; columns 7, 9 and
    17 are read for the chosen rows only.  `names`: the sorted distinct ids the codes index (find_orth.columns_from_text(...).names)."""

    def __init__(self, data, names):
        from .fsearch import parse_cigar
        self._parse = parse_cigar
        data = data.replace(b'\r\n', b'\n').replace(b'\r', b'\n')
        self.lines = [l for l in data.split(b'\n') if l]
        code = {n: k for k, n in enumerate(np.asarray(names).tolist())}
        n = len(self.lines)
        self.q, self.s, self.score = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.float64)
        for k, line in enumerate(self.lines):
            f = line.split(b'\t', 12)
            if k == 0 and line.count(b'\t') < 16:
                raise MissingCigar('the rows have no 17th column (the CIGAR): write the hits with find_hit.py -C T')
            try:
                sco = float(f[11])
            except (ValueError, IndexError):
                continue           # (a row find_orth's tokeniser drops too)
            if sco != sco:
                continue
            self.q[k], self.s[k], self.score[k] = code.get(f[0], -1), code.get(f[1], -1), sco

    def alignment(self, rows):
        qst, sst, runs = [], [], []
        for r in np.asarray(rows).tolist():
            f = self.lines[r].split(b'\t')
            if len(f) < 17:
                raise MissingCigar('row %d has no 17th column (the CIGAR): write the hits with find_hit.py -C T' % (r + 1))
            qst.append(int(f[6])), sst.append(int(f[8]))
            runs.append(pack_runs(self._parse(f[16].strip())))
        return np.asarray(qst, dtype=np.int64), np.asarray(sst, dtype=np.int64), runs


# ---------------------------------------------------------------------------------------------------------
# the stage
# ---------------------------------------------------------------------------------------------------------
def tasks_from_families(names, table, records, rows_src, device_stage=False, device=0, min_share=.9):
    """families + the picked rows' alignments -> (Tasks, anchor codes).  `records`: rbh.fasta_records of the FASTA the search read"""
    nm = np.asarray(names).tolist()
    fams = families(table, min_share)
    T = len(table.slots)
    if T == 0:
        raise ValueError('supermatrix: no taxa')
    if not fams:
        raise ValueError('supermatrix: no core family (nothing to align)')

    def seq_of(code):
        if nm[code] not in records:
            raise ValueError('supermatrix: %r is not a record of the FASTA file' % nm[code])
        return records[nm[code]][1]

    pq, ps = [], []
    for a, mem in fams:
        for _, m in mem:
            if m != a:
                pq.append(a), ps.append(m)
    pick = device_pick_rows if device_stage else pick_rows
    rows = pick(rows_src.q, rows_src.s, rows_src.score, pq, ps, **({'device': device} if device_stage else {}))
    lost = np.flatnonzero(rows < 0)
    if len(lost):
        k = int(lost[0])
        raise ValueError('supermatrix: no row aligns member %r to its anchor %r' % (nm[ps[k]], nm[pq[k]]))
    qst, sst, runs = rows_src.alignment(rows)
    col_off = np.zeros(len(fams) + 1, dtype=np.int64)
    fam, slot, kind, res_off, res_len, tq, ts, run_off, label = [], [], [], [], [], [], [], [0], []
    blob, pos, run_list, k = [], 0, [], 0
    for f, (a, mem) in enumerate(fams):
        col_off[f + 1] = col_off[f] + len(seq_of(a))
        for t, m in mem:
            seq = seq_of(m)
            fam.append(f), slot.append(t), res_off.append(pos), res_len.append(len(seq))
            blob.append(seq)
            pos += len(seq)
            if m == a:
                kind.append(1), tq.append(1), ts.append(1)
                label.append('anchor %r' % nm[a])
            else:
                kind.append(0), tq.append(int(qst[k])), ts.append(int(sst[k]))
                run_list.append(runs[k])
                label.append('row %d (anchor %r, member %r)' % (int(rows[k]) + 1, nm[a], nm[m]))
                k += 1
            run_off.append(run_off[-1] + (0 if m == a else len(run_list[-1])))
    all_runs = np.concatenate(run_list).astype(np.uint32) if run_list else np.zeros(0, dtype=np.uint32)
    tk = Tasks(T, col_off, fam, slot, kind, res_off, res_len, tq, ts, run_off, all_runs, b''.join(blob), label)
    return tk, np.asarray([a for a, _ in fams], dtype=np.int64)


def supermatrix(names, table, records, rows_src, gap_share=1.0, device_stage=False, want_matrix=True, device=0):
    """core table + the rows of the search -> Supermatrix; device_stage: the rows are picked and the matrix, the gap counts, the kept
    columns and the pair counts are built on the GPU (no fallback), else by the numpy definitions"""
    tk, anchors = tasks_from_families(names, table, records, rows_src, device_stage, device)
    stats = {'families': len(anchors), 'tasks': len(tk.fam)}
    if device_stage:
        try:
            matrix, gaps, keep, cmp_, same = device_build(tk, gap_share, want_matrix, device, stats=stats)
        except RuntimeError as e:
            import re
            m = re.search(r'task (\d+) \(family', str(e))      # the library names the task: say which row of the search that is
            raise ValueError('supermatrix: %s%s' % (e, ': ' + tk.label[int(m.group(1))] if m and tk.label else ''))
    else:
        matrix, gaps, keep, cmp_, same = build(tk, gap_share)
    return Supermatrix(list(table.slots), matrix, tk.col_off, gaps, keep, cmp_, same, anchors, stats)


# ---------------------------------------------------------------------------------------------------------
# host only: distances, neighbour joining, text
# ---------------------------------------------------------------------------------------------------------
def _label(x):
    return x.decode('utf-8', 'replace') if isinstance(x, bytes) else str(x)


AA20 = b'ARNDCQEGHILKMFPSTWYV'   # residue code a = the index in it; every other byte is uncoded
MODELS = ('p', 'poisson', 'kimura', 'logdet')
_NO_MODEL = "distances: the model is 'p', 'poisson', 'kimura' or 'logdet'"


class DistanceRefused(ValueError):
    """a pair of taxa has no kimura or logdet distance (rbh2phy.py exits with code 2)"""


def residue_codes(matrix):
    """-> uint8 like matrix: the index in AA20, 0xFF for every uncoded byte"""
    lut = np.full(256, 0xFF, dtype=np.uint8)
    lut[np.frombuffer(AA20, dtype=np.uint8)] = np.arange(20, dtype=np.uint8)
    return lut[np.asarray(matrix, dtype=np.uint8)]


def pair_index(T):
    """-> int64[P, 2], P = T (T - 1) / 2: the pairs (i, j), i < j, row-major -- (0, 1), (0, 2), .., (T - 2, T - 1)"""
    i, j = np.triu_indices(int(T), 1)
    return np.stack([i, j], 1).astype(np.int64)


def subst_counts(matrix, keep):
    """-> int32[P, 20, 20]: N[p, a, b] = the kept columns where taxon i of pair p holds residue a and taxon j residue b (pair_index);
    a column where either byte is uncoded adds nothing to the pair.  N = E E^T of the one-hot matrix E (row 20 i + a over the columns
    is code[i] == a), in float32 over at most 2^20 columns at a time (fewer for many taxa: E is held whole): every partial count is an
    integer below 2^24, so the sums are exact."""
    matrix = np.asarray(matrix, dtype=np.uint8)
    if matrix.ndim != 2:
        raise ValueError('subst_counts: the matrix has two dimensions')
    T = matrix.shape[0]
    keep = np.asarray(keep, dtype=np.int64)
    if len(keep) >= 2 ** 31:
        raise ValueError('subst_counts: 2^31 kept columns and more are not supported (32-bit counts)')
    pi = pair_index(T)
    N = np.zeros((len(pi), 20, 20), dtype=np.int64)
    step = max(1024, min(1 << 20, (1 << 26) // max(1, 20 * T)))
    res = np.arange(20, dtype=np.uint8)
    for c0 in range(0, len(keep), step):
        code = residue_codes(matrix[:, keep[c0:c0 + step]])
        E = (code[:, None, :] == res[None, :, None]).astype(np.float32).reshape(20 * T, -1)
        G = np.rint(E @ E.T).astype(np.int64).reshape(T, 20, T, 20)
        N += G[pi[:, 0], :, pi[:, 1], :]
    return N.astype(np.int32)


def boot_subst(matrix, keep, seed, b):
    """-> int32[P, 20, 20] of replicate b: subst_counts over keep[boot_columns(seed, b, len(keep))], as boot_counts draws them"""
    keep = np.asarray(keep, dtype=np.int64)
    return subst_counts(matrix, keep[boot_columns(seed, b, len(keep))])


def _logdet_pair(N):
    """one 20 x 20 table -> (d, None), or (nan, why) where the pair has no logdet distance"""
    N = np.asarray(N).astype(np.float64)
    r, c = N.sum(1), N.sum(0)
    if (r == 0).any() or (c == 0).any():
        a = int(np.flatnonzero((r == 0) | (c == 0))[0])
        return np.nan, 'residue %s never occurs in one of the two over the columns they share' % AA20[a:a + 1].decode()
    sign, ld = np.linalg.slogdet(N)
    if not sign > 0:
        return np.nan, 'their table of residue pairs is singular (or its determinant is negative)'
    return ((np.log(r).sum() + np.log(c).sum()) / 2. - ld) / 20., None      # = -(ld - (..) / 2) / 20, and 0.0 (not -0.0) where the two are equal


def _logdet(subst, T):
    """-> (D float64[T, T], first bad (i, j, why) or None): every pair once, mirrored, the diagonal 0.0 -- symmetric bit for bit"""
    if subst is None:
        raise ValueError("distances: model 'logdet' needs the substitution counts (subst_counts)")
    subst = np.asarray(subst)
    pi = pair_index(T)
    if subst.shape != (len(pi), 20, 20):
        raise ValueError('distances: the substitution counts are not [%d, 20, 20]' % len(pi))
    D, bad = np.zeros((T, T), dtype=np.float64), None
    for (i, j), N in zip(pi.tolist(), subst):
        d, why = _logdet_pair(N)
        if why is not None and bad is None:
            bad = (i, j, why)
        D[i, j] = D[j, i] = d
    return D, bad


def _kimura(p):
    """-> (D, argwhere of the pairs without a distance): -log(1 - p - p * p / 5)"""
    q = (1. - p) - p * p / 5.
    bad = np.argwhere(~(q > 0.))
    with np.errstate(divide='ignore', invalid='ignore'):
        return -np.log(q) + np.zeros(p.shape), bad


def distances(cmp, same, model='p', names=None, subst=None):
    """-> float64[T, T]: p = 1 - same / cmp; poisson: -log(1 - p); kimura: -log(1 - p - p * p / 5); logdet: from `subst` (subst_counts),
    per pair -(log det N - (sum log r + sum log c) / 2) / 20 with r, c the row and column sums of N (the column total cancels: no
    frequencies are formed).  A pair without a compared column, poisson with p >= 1, kimura with 1 - p - p * p / 5 <= 0 and logdet with a
    residue that one of the two taxa never shows, or with a singular table, refuse (the last two as DistanceRefused)"""
    if model not in MODELS:
        raise ValueError(_NO_MODEL)
    cmp, same = np.asarray(cmp, dtype=np.int64), np.asarray(same, dtype=np.int64)
    T = len(cmp)
    who = lambda k: _label(names[k]) if names is not None else str(k)
    bad = np.argwhere(cmp == 0)
    if len(bad):
        raise (ValueError if model in ('p', 'poisson') else DistanceRefused)('distances: taxa %s and %s share no compared column' % (who(bad[0][0]), who(bad[0][1])))
    if model == 'logdet':
        D, bad = _logdet(subst, T)
        if bad is not None:
            raise DistanceRefused('distances: taxa %s and %s have no logdet distance: %s' % (who(bad[0]), who(bad[1]), bad[2]))
        return D
    p = 1. - same.astype(np.float64) / cmp.astype(np.float64)
    if model == 'p':
        return p
    if model == 'kimura':
        D, bad = _kimura(p)
        if len(bad):
            raise DistanceRefused('distances: taxa %s and %s differ in too many compared columns (p = %.4f): no kimura distance' % (who(bad[0][0]), who(bad[0][1]), p[tuple(bad[0])]))
        return D
    bad = np.argwhere(p >= 1.)
    if len(bad):
        raise ValueError('distances: taxa %s and %s differ in every compared column: no poisson distance' % (who(bad[0][0]), who(bad[0][1])))
    return -np.log(1. - p) + np.zeros((T, T))


def _clade_words(c, T):
    """a clade (Python int, bit t = taxon t) -> its canonical uint64[W] words: complemented inside T bits where it holds taxon 0"""
    if c & 1:
        c = ~c & ((1 << T) - 1)
    return [(c >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range((T + 63) // 64)]


def _nj_walk(D, names, support=None, labels=None):
    """the walk of neighbor_joining -> (Newick bytes, uint64[T - 3, W] splits of the joins in join order, canonical as nj_splits' are).
    support[t] (a share in [0, 1]) labels the node join t makes, %.3f as fasttree prints it; labels[t]: a ready-made label string
    instead (not both)"""
    D = np.array(D, dtype=np.float64)
    n = T = len(names)
    if D.shape != (n, n):
        raise ValueError('neighbor_joining: D is not a square matrix over the names')
    if n < 2:
        raise ValueError('neighbor_joining: a tree needs two taxa at least')
    if support is not None and len(support) != max(T - 3, 0):
        raise ValueError('neighbor_joining: %d supports for %d joins' % (len(support), max(T - 3, 0)))
    if labels is not None:
        if support is not None:
            raise ValueError('neighbor_joining: supports or ready-made labels, not both')
        if len(labels) != max(T - 3, 0):
            raise ValueError('neighbor_joining: %d labels for %d joins' % (len(labels), max(T - 3, 0)))
    tag = (lambda t: '') if support is None and labels is None else (lambda t: str(labels[t])) if labels is not None else (lambda t: '%.3f' % support[t])
    node = [_label(x) for x in names]
    clade, splits = [1 << k for k in range(T)], []
    fmt = lambda s, l: '%s:%.6f' % (s, l)
    if n == 2:
        return ('(%s,%s);' % (fmt(node[0], D[0, 1] / 2.), fmt(node[1], D[0, 1] / 2.))).encode('utf-8'), np.zeros((0, 1), dtype=np.uint64)
    while n > 3:
        r = D.sum(1)
        Q = (n - 2) * D - r[:, None] - r[None, :]
        Q[np.tril_indices(n)] = np.inf
        i, j = divmod(int(np.argmin(Q)), n)      # (the first minimum in row-major order: the lowest (i, j))
        dij = D[i, j]
        li = dij / 2. + (r[i] - r[j]) / (2. * (n - 2))
        lj = dij - li
        du = (D[i] + D[j] - dij) / 2.
        D[i, :], D[:, i] = du, du
        D[i, i] = 0.
        D = np.delete(np.delete(D, j, 0), j, 1)
        node[i] = '(%s,%s)%s' % (fmt(node[i], li), fmt(node[j], lj), tag(len(splits)))
        clade[i] |= clade[j]
        splits.append(_clade_words(clade[i], T))
        del node[j], clade[j]
        n -= 1
    la = (D[0, 1] + D[0, 2] - D[1, 2]) / 2.
    lb = (D[0, 1] + D[1, 2] - D[0, 2]) / 2.
    lc = (D[0, 2] + D[1, 2] - D[0, 1]) / 2.
    newick = ('(%s,%s,%s);' % (fmt(node[0], la), fmt(node[1], lb), fmt(node[2], lc))).encode('utf-8')
    return newick, np.array(splits, dtype=np.uint64).reshape(len(splits), (T + 63) // 64)


def neighbor_joining(D, names, support=None, labels=None):
    """Saitou-Nei over float64 -> Newick bytes.  The pair with the smallest Q is joined, ties to the lexicographically lowest (i, j) in
    the current node order; the new node takes position i, j is removed; the last three nodes are a trifurcation; T = 2 is
    (A:d/2,B:d/2); branch lengths %.6f, negative ones as they come.  support (None: no labels): float[T - 3], support[t] labels the node
    join t makes, as in (A:0.100000,B:0.200000)0.950:0.300000 -- %.3f, the way fasttree prints it; the last trifurcation has no label.
    labels (instead of support): str[T - 3], printed as they are -- what tree(concordance=True) hands in."""
    return _nj_walk(D, names, support, labels)[0]


def tree_splits(D):
    """-> uint64[T - 3, W]: the splits of the tree neighbor_joining(D, ...) prints, join by join, in the canonical form of nj_splits"""
    return _nj_walk(D, [''] * len(D))[1]


# ---------------------------------------------------------------------------------------------------------
# bootstrap support: columns drawn with replacement, a tree per replicate, the share of the trees that hold a split
# ---------------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def boot_columns(seed, b, K):
    """-> int64[K]: the K draws of replicate b from K kept columns.  Draw k is splitmix64 of the counter (b << 32) + k + 1 in wrapping
    uint64 arithmetic (seed: any uint64, b < 2^31, K < 2^31), its high 32 bits scaled into [0, K) by a multiply and a shift:
    ((z >> 32) * K) >> 32.  The multiply-shift is off from uniform by at most K / 2^32 per column."""
    seed, b, K = int(seed), int(b), int(K)
    if not (0 <= seed <= _M64 and 0 <= b < 2 ** 31 and 0 <= K < 2 ** 31):
        raise ValueError('boot_columns: seed is a uint64, b and K lie below 2^31')
    u = np.uint64
    with np.errstate(over='ignore'):
        ctr = np.arange(1, K + 1, dtype=np.uint64) + u((b << 32) & _M64)
        z = u(seed) + ctr * u(0x9E3779B97F4A7C15)
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        z ^= z >> u(31)
        return (((z >> u(32)) * u(K)) >> u(32)).astype(np.int64)


def boot_counts(matrix, keep, seed, b):
    """-> (cmp, same) int64[T, T] of replicate b: pair_counts over keep[boot_columns(seed, b, len(keep))] (the order of the draws does
    not matter, a column drawn twice counts twice)"""
    keep = np.asarray(keep, dtype=np.int64)
    return pair_counts(matrix, keep[boot_columns(seed, b, len(keep))])


def boot_distances(cmp, same, model='p', subst=None):
    """-> (D float64[T, T], ok): distances() without its refusals.  ok is False when a pair has no compared column, under poisson also
    when a pair has p >= 1, under kimura when 1 - p - p * p / 5 <= 0, under logdet when a pair's table lacks a residue on one side or is
    singular: such a replicate is dropped, not refused (its D holds NaN or inf there)."""
    if model not in MODELS:
        raise ValueError(_NO_MODEL)
    cmp, same = np.asarray(cmp, dtype=np.int64), np.asarray(same, dtype=np.int64)
    ok = not (cmp == 0).any()
    if model == 'logdet':
        D, bad = _logdet(subst, len(cmp))
        return D, ok and bad is None
    with np.errstate(divide='ignore', invalid='ignore'):
        p = 1. - same.astype(np.float64) / cmp.astype(np.float64)
        if model == 'p':
            return p, ok
        if model == 'kimura':
            D, bad = _kimura(p)
            return D, ok and not len(bad)
        ok = ok and not (p >= 1.).any()
        return -np.log(1. - p) + np.zeros(p.shape), ok


def nj_splits(D):
    """-> uint64[T - 3, W], W = ceil(T / 64): the non-trivial splits of the neighbour-joining topology of D in join order.  The walk of
    neighbor_joining with ONE difference, which makes it reproducible on a GPU: the row sums are sequential -- r[i] is the left-to-right
    float64 sum over the live nodes in ascending order (np.cumsum(D, 1)[:, -1]), not D.sum(1), whose pairwise order no kernel shares.
    Q = ((n - 2) * D[i, j] - r[i]) - r[j], the minimum over i < j with ties to the lowest (i, j); the new row is
    ((D[i] + D[j]) - D[i, j]) / 2., it takes position i, j is removed.  A node's clade is a bit set over the taxa in slot order; a join
    ORs the two clades and emits the result, complemented inside T bits where it holds taxon 0.  T < 4: no split.  A non-finite D is
    refused."""
    D = np.array(D, dtype=np.float64)
    T = len(D)
    if D.ndim != 2 or D.shape != (T, T):
        raise ValueError('nj_splits: D is not a square matrix')
    if not np.isfinite(D).all():
        raise ValueError('nj_splits: D holds a value that is not finite')
    W = (T + 63) // 64
    clade, splits, n = [1 << k for k in range(T)], [], T
    while n > 3:
        r = np.cumsum(D, axis=1)[:, -1]
        Q = ((n - 2) * D - r[:, None]) - r[None, :]
        Q[np.tril_indices(n)] = np.inf
        i, j = divmod(int(np.argmin(Q)), n)
        du = ((D[i] + D[j]) - D[i, j]) / 2.
        D[i, :], D[:, i] = du, du
        D[i, i] = 0.
        D = np.delete(np.delete(D, j, 0), j, 1)
        clade[i] |= clade[j]
        splits.append(_clade_words(clade[i], T))
        del clade[j]
        n -= 1
    return np.array(splits, dtype=np.uint64).reshape(len(splits), W)


def split_support(ref_splits, rep_splits, ok):
    """-> int32[T - 3]: per split of the printed tree (ref_splits uint64[S, W]) the number of ok replicates whose tree holds it
    (rep_splits uint64[B, S, W], ok bool[B])"""
    ref = np.ascontiguousarray(ref_splits, dtype=np.uint64)
    rep = np.ascontiguousarray(rep_splits, dtype=np.uint64)
    out = np.zeros(len(ref), dtype=np.int32)
    keys = [row.tobytes() for row in ref]
    for b in np.flatnonzero(np.asarray(ok, dtype=bool)).tolist():
        held = {row.tobytes() for row in rep[b]}
        for s, k in enumerate(keys):
            if k in held:
                out[s] += 1
    return out


def batch_size(n, bytes_each, env=None):
    """items (replicates, families) per device call of a path whose distances are made on the host: the switch `env` names
    (SOHIT_PHY_BOOT_BATCH, SOHIT_PHY_GENE_BATCH) where it is set, else what about 2^30 bytes hold at bytes_each a piece; n and 32768 (the
    most a device call takes) at the most, one at least"""
    import os
    forced = int(os.environ.get(env, '0') or 0) if env else 0
    return max(1, min(n, 32768, forced if forced > 0 else (1 << 30) // max(1, bytes_each)))


def replicate_trees(n, step, counts_of, distance_of, trees_of, S, W):
    """-> (ok bool[n], splits uint64[n, S, W], calls): the loop every tree per replicate or per family is made in, `step` items at a time.
    counts_of(i0, k) -> (the inputs of items i0 .. i0 + k - 1, the device calls that took); distance_of(batch, j) -> (D float64[T, T], ok)
    of item j of the batch; trees_of(D float64[m, T, T], idx) -> uint64[m, S, W], the splits of the items idx that have a distance, asked
    for once per batch (a call) where there is such an item and S > 0.  An item without a distance is not ok, its splits are zeros."""
    ok, splits, calls = np.zeros(n, dtype=bool), np.zeros((n, S, W), dtype=np.uint64), 0
    for i0 in range(0, n, step):
        k = min(step, n - i0)
        batch, made = counts_of(i0, k)
        dist = [distance_of(batch, j) for j in range(k)]
        good = [j for j in range(k) if dist[j][1]]
        idx = [i0 + j for j in good]
        calls += made
        if good and S:
            splits[idx] = trees_of(np.stack([dist[j][0] for j in good]), idx)
            calls += 1
        ok[idx] = True
    return ok, splits, calls


def device_boot_counts(matrix, keep, seed, b0, nb, device=0):
    """boot_counts() of replicates b0 .. b0 + nb - 1 in one device call (so_phy_boot_counts) -> (cmp, same) int64[nb, T, T]"""
    matrix, keep = _lib.matrix2d('device_boot_counts', matrix), np.ascontiguousarray(keep, dtype=np.int64)
    T, nc = matrix.shape
    with _call('so_phy_boot_counts', 'SoPhyBootResult', 'so_phy_boot_free', int(device), T, nc, matrix, len(keep), keep, int(seed) & _M64, int(b0), int(nb), 0) as res:
        return _arr(res.cmp, nb * T * T, np.int64).reshape(nb, T, T), _arr(res.same, nb * T * T, np.int64).reshape(nb, T, T)


def _device_subst(who, matrix, keep, seed, b0, nb, device, stats=None, want=True, timed=False):
    """so_phy_subst -> int32[max(nb, 1), P, 20, 20] (None without `want`); nb = 0: the kept columns"""
    matrix, keep = _lib.matrix2d(who, matrix), np.ascontiguousarray(keep, dtype=np.int64)
    T, nc = matrix.shape
    flags = (0 if want else 1) | (2 if timed else 0)
    with _call('so_phy_subst', 'SoPhySubstResult', 'so_phy_subst_free', int(device), T, nc, matrix, len(keep), keep, int(seed) & _M64, int(b0), int(nb), flags) as res:
        if stats is not None:
            stats['waits'], stats['bytes'] = int(res.waits), int(res.bytes)
            if timed:
                stats['code_ms'], stats['product_ms'] = float(res.code_ms), float(res.product_ms)
        n, P = int(res.n_reps), int(res.n_pairs)
        return _arr(res.subst, n * P * 400, np.int32).reshape(n, P, 20, 20) if want else None


def device_subst_counts(matrix, keep, device=0, stats=None):
    """subst_counts() in one device call (so_phy_subst) -> int32[P, 20, 20]; a refusal raises RuntimeError with the library's message"""
    return _device_subst('device_subst_counts', matrix, keep, 0, 0, 0, device, stats)[0]


def device_boot_subst(matrix, keep, seed, b0, nb, device=0, stats=None):
    """boot_subst() of replicates b0 .. b0 + nb - 1 in one device call (so_phy_subst) -> int32[nb, P, 20, 20]"""
    if int(nb) < 1:
        raise ValueError('device_boot_subst: a replicate at least')
    return _device_subst('device_boot_subst', matrix, keep, seed, b0, nb, device, stats)


def model_subst(sm, model, device_stage=False, device=0):
    """the substitution counts `model` needs over sm's kept columns (None for every model but logdet), computed once and kept in
    sm.subst: device_stage: so_phy_subst, else subst_counts"""
    if model != 'logdet':
        return None
    if getattr(sm, 'subst', None) is None:
        if sm.matrix is None:
            raise ValueError('tree: the supermatrix was built without its matrix')
        try:
            sm.subst = device_subst_counts(sm.matrix, sm.keep, device) if device_stage else subst_counts(sm.matrix, sm.keep)
        except RuntimeError as e:
            raise ValueError('tree: %s' % e)
    return sm.subst


def _walk_args(who, D):
    """-> (D as contiguous float64[nb, T, T], nb, T, S = T - 3 splits, W words per split): what the two walk calls take"""
    D = np.ascontiguousarray(D, dtype=np.float64)
    if D.ndim != 3 or D.shape[1] != D.shape[2]:
        raise ValueError('%s: D is float64[nb, T, T]' % who)
    nb, T = D.shape[0], D.shape[1]
    return D, nb, T, max(T - 3, 0), (T + 63) // 64


def device_nj_splits(D, device=0, clades_in_global=False, stats=None):
    """nj_splits() of nb matrices D float64[nb, T, T] in one device call (so_phy_nj_splits), a workgroup per matrix -> uint64[nb, T - 3, W].
    The device reads D[k][i] for D[i][k]: a D that is not symmetric bit for bit is refused, as a non-finite one is.  clades_in_global
    (tests): the clade bit sets in global scratch, where the call keeps them once they outgrow the LDS.  stats: 'nj_tier', where they were
    kept (0: T < 4, no walk; 1: LDS; 2: global scratch)"""
    D, nb, T, S, W = _walk_args('device_nj_splits', D)
    with _call('so_phy_nj_splits', 'SoPhyBootResult', 'so_phy_boot_free', int(device), nb, T, D, 1 if clades_in_global else 0) as res:
        if stats is not None:
            stats['nj_tier'] = int(res.nj_tier)
        return _arr(res.splits, nb * S * W, np.uint64).reshape(nb, S, W)


def device_boot(matrix, keep, seed, B, ref_splits, want_splits=False, device=0, stats=None, timed=False):
    """the fused bootstrap of model p (so_phy_boot): counts, D = 1 - same / cmp, the trees and their comparison with ref_splits stay on
    the device, in batches of replicates with one host wait each -> (count int32[T - 3], valid, ok bool[B], splits uint64[B, T - 3, W] or
    None); a dropped replicate's splits are zeros.  stats: 'waits', 'batches'; a stats that comes with the key 'nj_tier' gets it filled
    (device_nj_splits: where the walk kept its bit sets; the callers that compare or print the whole dict see no new key); timed: also
    'counts_ms', 'trees_ms', 'support_ms', the device time of the stages by events"""
    matrix, keep = _lib.matrix2d('device_boot', matrix), np.ascontiguousarray(keep, dtype=np.int64)
    T, nc = matrix.shape
    S, W = max(T - 3, 0), (T + 63) // 64
    ref = np.ascontiguousarray(ref_splits, dtype=np.uint64)
    if ref.size != S * W:
        raise ValueError('device_boot: the printed tree has %d splits of %d words' % (S, W))
    with _call('so_phy_boot', 'SoPhyBootResult', 'so_phy_boot_free', int(device), T, nc, matrix, len(keep), keep, int(seed) & _M64, int(B), ref,
               (1 if want_splits else 0) | (2 if timed else 0)) as res:
        if stats is not None:
            stats['waits'], stats['batches'] = int(res.waits), int(res.batches)
            if 'nj_tier' in stats:
                stats['nj_tier'] = int(res.nj_tier)
            if timed:
                stats['counts_ms'], stats['trees_ms'], stats['support_ms'] = float(res.counts_ms), float(res.trees_ms), float(res.support_ms)
        splits = _arr(res.splits, B * S * W, np.uint64).reshape(B, S, W) if want_splits else None
        return _arr(res.count, S, np.int32), int(res.valid), _arr(res.ok, B, np.uint8).astype(bool), splits


def bootstrap_replicates(sm, B, seed=1, model='p', device_stage=False, device=0, stats=None, want_splits=True):
    """-> (count int32[T - 3], valid, ok bool[B], splits uint64[B, T - 3, W] or None): everything bootstrap() is made from.  Host: the
    numpy definitions replicate by replicate.  device_stage, model p: so_phy_boot; poisson: the counts of a batch by so_phy_boot_counts,
    the distances on the host (the device's log is not numpy's), the trees by so_phy_nj_splits, the support by split_support; kimura
    goes poisson's way, logdet too, with the tensors of the batch by so_phy_subst and the determinants on the host.  Either way the
    replicates go through replicate_trees, the host's one at a time."""
    B, seed = int(B), int(seed)
    if not 1 <= B < 2 ** 31:
        raise ValueError('bootstrap: B lies in 1 .. 2^31 - 1')
    if sm.matrix is None:
        raise ValueError('bootstrap: the supermatrix was built without its matrix')
    T = len(sm.taxa)
    S, W = max(T - 3, 0), (T + 63) // 64
    logdet = model == 'logdet'
    ref = tree_splits(distances(sm.cmp, sm.same, model, sm.taxa, model_subst(sm, model, device_stage, device))) if T >= 2 else np.zeros((0, W), dtype=np.uint64)
    if len(sm.keep) == 0:
        raise ValueError('bootstrap: no kept column to draw from')
    try:
        if device_stage and model == 'p':
            return device_boot(sm.matrix, sm.keep, seed, B, ref, want_splits, device, stats)
        if device_stage:
            Kp = (len(sm.keep) + 15) & ~15
            step = batch_size(B, T * Kp + 16 * T * T + (2 * T * Kp + 800 * T * (T - 1) if logdet else 0), 'SOHIT_PHY_BOOT_BATCH')   # (logdet: codes and the tensor, 1600 bytes a pair)

            def counts_of(b0, nb):
                cmp_, same = device_boot_counts(sm.matrix, sm.keep, seed, b0, nb, device)
                return (cmp_, same, device_boot_subst(sm.matrix, sm.keep, seed, b0, nb, device) if logdet else [None] * nb), 2 if logdet else 1
            trees_of = lambda D, idx: device_nj_splits(D, device)
        else:
            step = 1

            def counts_of(b, _):
                cmp_, same = boot_counts(sm.matrix, sm.keep, seed, b)
                return ([cmp_], [same], [boot_subst(sm.matrix, sm.keep, seed, b) if logdet else None]), 0
            trees_of = lambda D, idx: nj_splits(D[0])[None]
        ok, splits, calls = replicate_trees(B, step, counts_of, lambda c, k: boot_distances(c[0][k], c[1][k], model, c[2][k]), trees_of, S, W)
    except RuntimeError as e:
        raise ValueError('bootstrap: %s' % e)
    if stats is not None and device_stage:
        stats['calls'] = calls
    return split_support(ref, splits, ok), int(ok.sum()), ok, splits if want_splits else None


def bootstrap(sm, B, seed=1, model='p', device_stage=False, device=0, stats=None):
    """Felsenstein's bootstrap of the neighbour-joining tree over the kept columns -> (count int32[T - 3], valid): B replicates draw the
    kept columns with replacement (boot_columns), each gives pair counts (boot_counts), distances (boot_distances) and a topology
    (nj_splits); a replicate that leaves a pair without a distance is dropped; count[t] = the valid replicates that hold the split join t
    of the printed tree makes (tree_splits).  No valid replicate: ValueError."""
    count, valid = bootstrap_replicates(sm, B, seed, model, device_stage, device, stats, want_splits=False)[:2]
    if valid == 0:
        raise ValueError('bootstrap: none of the %d replicates gives every pair of taxa a distance' % int(B))
    return count, valid


# ---------------------------------------------------------------------------------------------------------
# gene concordance factors: a tree per core family over the taxa it holds, the share of the deciding families that hold a split
# ---------------------------------------------------------------------------------------------------------
GENE_MODELS = ('p', 'poisson', 'kimura')
_NO_GENE_MODEL = "gene concordance: the model is 'p', 'poisson' or 'kimura' (a family's block is where logdet has no distance)"


class ConcordanceRefused(ValueError):
    """no gene concordance factor can be given (rbh2phy.py exits with code 2)"""


def family_ranges(keep, col_off):
    """-> int64[F + 1]: family f owns keep[r[f]:r[f + 1]], the kept columns of its block col_off[f] .. col_off[f + 1] (keep ascending)"""
    return np.searchsorted(np.asarray(keep, dtype=np.int64), np.asarray(col_off, dtype=np.int64)).astype(np.int64)


def family_counts(matrix, keep, col_off):
    """-> (cmp, same) int64[F, T, T]: pair_counts over each family's kept columns"""
    keep = np.asarray(keep, dtype=np.int64)
    r = family_ranges(keep, col_off)
    T = np.asarray(matrix).shape[0]
    cmp_, same = np.zeros((len(r) - 1, T, T), dtype=np.int64), np.zeros((len(r) - 1, T, T), dtype=np.int64)
    for f in range(len(r) - 1):
        cmp_[f], same[f] = pair_counts(matrix, keep[r[f]:r[f + 1]])
    return cmp_, same


def _bool_words(flags):
    """bool[..., T] -> uint64[..., W]: bit t & 63 of word t >> 6 is flag t"""
    flags = np.asarray(flags, dtype=bool)
    T = flags.shape[-1]
    W = (T + 63) // 64
    bits = np.zeros(flags.shape[:-1] + (W * 64,), dtype=np.uint8)
    bits[..., :T] = flags
    return np.ascontiguousarray(np.packbits(bits, axis=-1, bitorder='little')).view(np.uint64).reshape(flags.shape[:-1] + (W,))


def _words_bool(words, T):
    """uint64[..., W] -> bool[..., T]"""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    return np.unpackbits(words.view(np.uint8), axis=-1, bitorder='little')[..., :T].astype(bool)


def _popcount(words):
    """uint64[..., W] -> int64[...]: the bits set over the last axis"""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    return np.unpackbits(words.view(np.uint8), axis=-1).sum(-1, dtype=np.int64)


def family_present(cmp):
    """int64[F, T, T] (or [T, T]) -> uint64[F, W] (or [W]): taxon t is present in family f iff cmp[f, t, t] > 0 -- it holds a byte that is
    not '-' in a kept column of the block; bit sets in slot order, W = ceil(T / 64)"""
    cmp = np.asarray(cmp)
    return _bool_words(np.diagonal(cmp, axis1=-2, axis2=-1) > 0)


def gene_distances(cmp_f, same_f, present_f, model='p'):
    """-> (D float64[T, T], ok): boot_distances restricted to present x present (present_f: uint64[W]).  ok is False when two present taxa
    share no compared column, or when the model refuses a present pair.  Entries outside present x present are unspecified: nothing reads
    them.  logdet is refused."""
    if model not in GENE_MODELS:
        raise ValueError(_NO_GENE_MODEL)
    cmp_f, same_f = np.asarray(cmp_f, dtype=np.int64), np.asarray(same_f, dtype=np.int64)
    T = len(cmp_f)
    idx = np.flatnonzero(_words_bool(present_f, T))
    D = np.zeros((T, T), dtype=np.float64)
    sub, ok = boot_distances(cmp_f[np.ix_(idx, idx)], same_f[np.ix_(idx, idx)], model)
    D[np.ix_(idx, idx)] = sub
    return D, bool(ok)


def nj_splits_subset(D, present):
    """-> uint64[T - 3, W]: nj_splits of D[present][:, present] with the clade bits moved back to the original slots (present: uint64[W]).
    A clade that holds the LOWEST PRESENT taxon is complemented inside the present set (nj_splits complements the clade of its taxon 0
    inside its own taxa: the same thing).  With n present taxa the rows n - 3 .. are zero; n < 4: all zeros."""
    D = np.asarray(D, dtype=np.float64)
    T = len(D)
    W = (T + 63) // 64
    out = np.zeros((max(T - 3, 0), W), dtype=np.uint64)
    idx = np.flatnonzero(_words_bool(present, T))
    n = len(idx)
    if n < 4:
        return out
    bits = np.zeros((n - 3, W * 64), dtype=bool)
    bits[:, idx] = _words_bool(nj_splits(D[np.ix_(idx, idx)]), n)
    out[:n - 3] = _bool_words(bits)
    return out


def concordance(ref_splits, present, gene_splits, ok):
    """-> (decisive, concordant) int32[S].  For split s of the printed tree (ref_splits uint64[S, W], clade C) and an ok family with present
    set P (present uint64[F, W]): A = C & P, B = P & ~C; the family is decisive for s iff both hold two taxa at least, and concordant iff it
    is decisive and its tree (gene_splits uint64[F, S, W], nj_splits_subset) holds whichever of A and B does not contain P's lowest taxon.
    A dropped family (ok False) is counted nowhere."""
    ref = np.ascontiguousarray(ref_splits, dtype=np.uint64)
    present = np.ascontiguousarray(present, dtype=np.uint64)
    gene = np.ascontiguousarray(gene_splits, dtype=np.uint64)
    S = len(ref)
    dec, con = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)
    if S == 0:
        return dec, con
    for f in np.flatnonzero(np.asarray(ok, dtype=bool)).tolist():
        P = present[f]
        A, B = ref & P, ~ref & P
        d = (_popcount(A) >= 2) & (_popcount(B) >= 2)
        if not d.any():
            continue
        dec += d
        w = int(np.flatnonzero(P)[0])                     # (a decisive family has four present taxa at least)
        low = P[w] & (~P[w] + np.uint64(1))               # the lowest present taxon's bit
        side = np.where(((A[:, w] & low) != 0)[:, None], B, A)
        held = {row.tobytes() for row in gene[f]}
        for s in np.flatnonzero(d).tolist():
            if side[s].tobytes() in held:
                con[s] += 1
    return dec, con


def _gene_args(who, matrix, keep, fam_off):
    return _lib.matrix2d(who, matrix), np.ascontiguousarray(keep, dtype=np.int64), np.ascontiguousarray(fam_off, dtype=np.int64)


def device_gene(matrix, keep, fam_off, ref_splits, want_splits=False, device=0, stats=None, timed=False):
    """the fused gene concordance of model p (so_phy_gene): the families' kept columns, their pair counts, D = 1 - same / cmp, presence, the
    trees over the present taxa and their comparison with ref_splits stay on the device, in batches of families with one host wait each
    -> (decisive int32[T - 3], concordant int32[T - 3], ok bool[F], n_present int32[F], present uint64[F, W] or None, splits
    uint64[F, T - 3, W] or None).  stats: 'waits', 'batches', 'nj_tier'; timed: also 'counts_ms', 'trees_ms', 'concord_ms' by events"""
    matrix, keep, fam_off = _gene_args('device_gene', matrix, keep, fam_off)
    T, nc = matrix.shape
    F, S, W = len(fam_off) - 1, max(T - 3, 0), (T + 63) // 64
    ref = np.ascontiguousarray(ref_splits, dtype=np.uint64)
    if ref.size != S * W:
        raise ValueError('device_gene: the printed tree has %d splits of %d words' % (S, W))
    with _call('so_phy_gene', 'SoPhyGeneResult', 'so_phy_gene_free', int(device), T, nc, matrix, len(keep), keep, F, fam_off, ref,
               (1 if want_splits else 0) | (2 if timed else 0)) as res:
        if stats is not None:
            stats['waits'], stats['batches'], stats['nj_tier'] = int(res.waits), int(res.batches), int(res.nj_tier)
            if timed:
                stats['counts_ms'], stats['trees_ms'], stats['concord_ms'] = float(res.counts_ms), float(res.trees_ms), float(res.concord_ms)
        return (_arr(res.decisive, S, np.int32), _arr(res.concordant, S, np.int32), _arr(res.ok, F, np.uint8).astype(bool), _arr(res.n_present, F, np.int32),
                _arr(res.present, F * W, np.uint64).reshape(F, W) if want_splits else None, _arr(res.splits, F * S * W, np.uint64).reshape(F, S, W) if want_splits else None)


def device_gene_counts(matrix, keep, fam_off, f0=0, nf=None, device=0):
    """family_counts() of the families f0 .. f0 + nf - 1 in one device call (so_phy_gene_counts) -> (cmp, same) int64[nf, T, T]"""
    matrix, keep, fam_off = _gene_args('device_gene_counts', matrix, keep, fam_off)
    T, nc = matrix.shape
    nf = len(fam_off) - 1 - int(f0) if nf is None else int(nf)
    with _call('so_phy_gene_counts', 'SoPhyGeneResult', 'so_phy_gene_free', int(device), T, nc, matrix, len(keep), keep, len(fam_off) - 1, fam_off, int(f0), nf, 0) as res:
        return _arr(res.cmp, nf * T * T, np.int64).reshape(nf, T, T), _arr(res.same, nf * T * T, np.int64).reshape(nf, T, T)


def device_nj_subsets(D, present, device=0, clades_in_global=False, stats=None):
    """nj_splits_subset() of nb matrices D float64[nb, T, T], each with its own present words uint64[nb, W], in one device call
    (so_phy_nj_subsets) -> uint64[nb, T - 3, W].  Only present x present is read; there D is finite and symmetric bit for bit, or the
    call is refused.  clades_in_global, stats['nj_tier']: as device_nj_splits"""
    D, nb, T, S, W = _walk_args('device_nj_subsets', D)
    present = np.ascontiguousarray(present, dtype=np.uint64)
    if present.shape != (nb, W):
        raise ValueError('device_nj_subsets: present is uint64[nb, %d]' % W)
    with _call('so_phy_nj_subsets', 'SoPhyGeneResult', 'so_phy_gene_free', int(device), nb, T, D, present, 1 if clades_in_global else 0) as res:
        if stats is not None:
            stats['nj_tier'] = int(res.nj_tier)
        return _arr(res.splits, nb * S * W, np.uint64).reshape(nb, S, W)


def gene_concordance(sm, model='p', device_stage=False, device=0, stats=None, want_splits=False):
    """the gene concordance factors of the printed tree -> (decisive int32[T - 3], concordant int32[T - 3], ok bool[F], n_present int32[F],
    splits uint64[F, T - 3, W] or None).  Every core family's kept columns (family_ranges) give pair counts (family_counts), the taxa it
    holds (family_present), distances among them (gene_distances) and a tree over them (nj_splits_subset); concordance() compares the
    trees with the splits of the printed tree (tree_splits).  A family in which two present taxa share no compared column, or a present
    pair has no distance under the model, is dropped.  Host: the numpy definitions family by family.  device_stage, model p: so_phy_gene;
    poisson and kimura: the counts of a batch of families by so_phy_gene_counts, the distances on the host (the device's log is not
    numpy's), the trees by so_phy_nj_subsets, the comparison by concordance().  Either way the families go through replicate_trees."""
    if model not in GENE_MODELS:
        raise ConcordanceRefused(_NO_GENE_MODEL)
    if sm.matrix is None:
        raise ValueError('gene concordance: the supermatrix was built without its matrix')
    T, F = len(sm.taxa), len(sm.col_off) - 1
    S, W = max(T - 3, 0), (T + 63) // 64
    keep = np.asarray(sm.keep, dtype=np.int64)
    ref = tree_splits(distances(sm.cmp, sm.same, model, sm.taxa)) if T >= 2 else np.zeros((0, W), dtype=np.uint64)
    r = family_ranges(keep, sm.col_off)
    present = np.zeros((F, W), dtype=np.uint64)

    def counts_of(f0, nf):
        if device_stage:
            cmp_, same = device_gene_counts(sm.matrix, keep, r, f0, nf, device)
        else:
            cmp_, same = family_counts(sm.matrix, keep[r[f0]:r[f0 + nf]], sm.col_off[f0:f0 + nf + 1])
        present[f0:f0 + nf] = family_present(cmp_)
        return (cmp_, same, present[f0:f0 + nf]), 1 if device_stage else 0
    try:
        if device_stage and model == 'p':
            dec, con, ok, npres, _, splits = device_gene(sm.matrix, keep, r, ref, want_splits, device, stats)
            return dec, con, ok, npres, splits
        trees_of = (lambda D, idx: device_nj_subsets(D, present[idx], device)) if device_stage else (lambda D, idx: nj_splits_subset(D[0], present[idx[0]])[None])
        ok, splits, calls = replicate_trees(F, batch_size(F, 16 * T * T, 'SOHIT_PHY_GENE_BATCH') if device_stage else 1, counts_of,
                                            lambda c, k: gene_distances(c[0][k], c[1][k], c[2][k], model), trees_of, S, W)
    except RuntimeError as e:
        raise ValueError('gene concordance: %s' % e)
    if stats is not None and device_stage:
        stats['calls'] = calls
    dec, con = concordance(ref, present, splits, ok)
    return dec, con, ok, _popcount(present).astype(np.int32), splits if want_splits else None


def gcf_labels(decisive, concordant):
    """-> [str]: concordant / decisive as %.3f, NA where no family is decisive"""
    return ['NA' if d == 0 else '%.3f' % (c / float(d)) for d, c in zip(np.asarray(decisive).tolist(), np.asarray(concordant).tolist())]


def gcf_table(taxa, ref_splits, decisive, concordant):
    """-> bytes: a header line and one line per join of the printed tree, in join order, tab-separated: join, taxa_in_clade, decisive,
    concordant, gcf (Python's repr of concordant / decisive, NA when undecided) and the clade's taxa in slot order, comma-separated (the
    clade as tree_splits hands it out: the side without the first taxon)"""
    T = len(taxa)
    ref = np.ascontiguousarray(ref_splits, dtype=np.uint64).reshape(len(decisive), (T + 63) // 64)
    lines = ['join\ttaxa_in_clade\tdecisive\tconcordant\tgcf\ttaxa\n']
    for t, (d, c) in enumerate(zip(np.asarray(decisive).tolist(), np.asarray(concordant).tolist())):
        inside = np.flatnonzero(_words_bool(ref[t], T)).tolist()
        lines.append('%d\t%d\t%d\t%d\t%s\t%s\n' % (t, len(inside), d, c, 'NA' if d == 0 else repr(c / float(d)), ','.join(_label(taxa[k]) for k in inside)))
    return ''.join(lines).encode('utf-8')


def supermatrix_fasta(taxa, matrix, keep):
    """-> bytes: `>taxon\\nrow\\n` per taxon in slot order, the kept columns only"""
    matrix, keep = np.asarray(matrix, dtype=np.uint8), np.asarray(keep, dtype=np.int64)
    return b''.join(b'>' + (t if isinstance(t, bytes) else str(t).encode('utf-8')) + b'\n' + matrix[k, keep].tobytes() + b'\n' for k, t in enumerate(taxa))


def tree(sm, model='p', boot=0, seed=1, device_stage=False, device=0, stats=None, concordance=False):
    """Supermatrix -> Newick bytes over its taxa; boot > 0: every node a join makes carries the share of the valid bootstrap replicates
    that hold its split (bootstrap(); stats: 'boot', 'boot_valid' and the device's counters).  concordance: the node of join t carries its
    gene concordance factor concordant[t] / decisive[t] (gene_concordance(); %.3f, NA where no family decides the branch); with boot > 0
    as well the label is boot/gcf, as in )0.950/0.812:0.300000.  stats then holds 'gcf': ref splits, decisive, concordant, ok, n_present
    and the device's counters of that stage.  No family left to ask (every one dropped): ConcordanceRefused."""
    if concordance and model not in GENE_MODELS:
        raise ConcordanceRefused(_NO_GENE_MODEL)
    D = distances(sm.cmp, sm.same, model, sm.taxa, model_subst(sm, model, device_stage, device))
    if int(boot) <= 0 and not concordance:
        return neighbor_joining(D, sm.taxa)
    labels = None
    if concordance:
        gs = {}
        dec, con, ok, npres, _ = gene_concordance(sm, model, device_stage, device, gs)
        if not ok.any():
            raise ConcordanceRefused('gene concordance: none of the %d families gives every pair of its taxa a distance' % len(ok))
        labels = gcf_labels(dec, con)
        if stats is not None:
            stats['gcf'] = {'splits': tree_splits(D), 'decisive': dec, 'concordant': con, 'ok': ok, 'n_present': npres, 'device': gs}
    if int(boot) <= 0:
        return neighbor_joining(D, sm.taxa, labels=labels)
    count, valid = bootstrap(sm, boot, seed, model, device_stage, device, stats)
    if stats is not None:
        stats['boot'], stats['boot_valid'] = int(boot), valid
    if labels is None:
        return neighbor_joining(D, sm.taxa, count / float(valid))
    return neighbor_joining(D, sm.taxa, labels=['%.3f/%s' % (b, g) for b, g in zip((count / float(valid)).tolist(), labels)])


# ---------------------------------------------------------------------------------------------------------
# scripts/rbh2phy.py -A T
# ---------------------------------------------------------------------------------------------------------
def run_align(sc_bytes, fasta_bytes, cols, table, gap_share=1.0, model='p', tree_path='', device_stage=False, out=None, boot=0, seed=1, concordance=False, gcf_path=''):
    """the -A T half of rbh2phy.py: the supermatrix FASTA to `out` (default: stdout), the tree to `tree_path` when named -> Supermatrix;
    boot > 0: the tree's nodes carry their bootstrap support over `boot` replicates drawn from `seed` (sm.stats: boot, boot_valid);
    concordance: they carry their gene concordance factors (tree()), and `gcf_path`, when named, receives gcf_table()"""
    if concordance and model not in GENE_MODELS:
        raise ConcordanceRefused(_NO_GENE_MODEL)      # (before the supermatrix is built)
    rows_src = TextRows(sc_bytes, cols.names)
    sm = supermatrix(cols.names, table, rbh.fasta_records(fasta_bytes), rows_src, gap_share, device_stage)
    newick = tree(sm, model, boot, seed, device_stage, stats=sm.stats, **({'concordance': True} if concordance else {})) if tree_path else None      # (before anything is printed: a refusal leaves no half output)
    o = out if out is not None else sys.stdout.buffer
    o.write(supermatrix_fasta(sm.taxa, sm.matrix, sm.keep))
    o.flush()
    if tree_path:
        with open(tree_path, 'wb') as f:
            f.write(newick + b'\n')
        if concordance and gcf_path:
            g = sm.stats['gcf']
            with open(gcf_path, 'wb') as f:
                f.write(gcf_table(sm.taxa, g['splits'], g['decisive'], g['concordant']))
    return sm
