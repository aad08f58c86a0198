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
"""
import math
import sys

import numpy as np

from . import rbh

GAP = 45   # '-'


class Supermatrix:
    """`taxa` (bytes, slot order), `matrix` uint8[T, L] (None when a device call was asked for the counts only), `col_off` int64[F + 1],
    `gaps` int32[L], `keep` int64[L'], `cmp` / `same` int64[T, T] over the kept columns, `anchors` (name codes, family order), `stats`"""

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
    import ctypes as C
    from . import _lib
    L = _lib.load()
    q32, s32 = _codes32(cols_q, 'device_pick_rows'), _codes32(cols_s, 'device_pick_rows')
    sco = np.ascontiguousarray(score, dtype=np.float64)
    pq, ps = _codes32(pair_q, 'device_pick_rows'), _codes32(pair_s, 'device_pick_rows')
    if not (len(q32) == len(s32) == len(sco)) or len(pq) != len(ps):
        raise ValueError('device_pick_rows: the columns differ in length')
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    out = _lib.SoPhyResult()
    if L.so_phy_rows(int(device), len(q32), ptr(q32), ptr(s32), ptr(sco), len(pq), ptr(pq), ptr(ps), 0, C.byref(out)) != 0:
        raise RuntimeError(L.so_phy_last_error().decode())
    try:
        return _lib.result_array(out.row, len(pq), np.int64)
    finally:
        L.so_phy_free(C.byref(out))


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
    import ctypes as C
    from . import _lib
    L = _lib.load()
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    res = _lib.SoPhyResult()
    F, n = len(tk.col_off) - 1, len(tk.fam)
    rc = L.so_phy_build(int(device), tk.n_taxa, F, ptr(tk.col_off), n, ptr(tk.fam), ptr(tk.slot), ptr(tk.kind), ptr(tk.res_off), ptr(tk.res_len), ptr(tk.qst),
                        ptr(tk.sst), ptr(tk.run_off), ptr(tk.runs), len(tk.runs), ptr(tk.residues), len(tk.residues), float(g), 0 if want_matrix else 1, C.byref(res))
    if rc != 0:
        raise RuntimeError(L.so_phy_last_error().decode())
    try:
        arr = _lib.result_array
        T, nc, nk = tk.n_taxa, int(res.n_cols), int(res.n_keep)
        matrix = arr(res.matrix, T * nc, np.uint8).reshape(T, nc) if want_matrix else None
        if out is not None and matrix is not None:
            out[...] = matrix
        if stats is not None:
            stats['waits'] = int(res.waits)
        return (matrix, arr(res.gaps, nc, np.int32), arr(res.keep, nc, np.int64)[:nk], arr(res.cmp, T * T, np.int64).reshape(T, T),
                arr(res.same, T * T, np.int64).reshape(T, T))
    finally:
        L.so_phy_free(C.byref(res))


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


def distances(cmp, same, model='p', names=None):
    """-> float64[T, T]: p = 1 - same / cmp, or -log(1 - p) (poisson); a pair without a compared column, or poisson with p >= 1, refuses"""
    if model not in ('p', 'poisson'):
        raise ValueError("distances: the model is 'p' or 'poisson'")
    cmp, same = np.asarray(cmp, dtype=np.int64), np.asarray(same, dtype=np.int64)
    T = len(cmp)
    who = lambda k: _label(names[k]) if names is not None else str(k)
    bad = np.argwhere(cmp == 0)
    if len(bad):
        raise ValueError('distances: taxa %s and %s share no compared column' % (who(bad[0][0]), who(bad[0][1])))
    p = 1. - same.astype(np.float64) / cmp.astype(np.float64)
    if model == 'p':
        return p
    bad = np.argwhere(p >= 1.)
    if len(bad):
        raise ValueError('distances: taxa %s and %s differ in every compared column: no poisson distance' % (who(bad[0][0]), who(bad[0][1])))
    return -np.log(1. - p) + np.zeros((T, T))


def neighbor_joining(D, names):
    """Saitou-Nei over float64 -> Newick bytes.  The pair with the smallest Q is joined, ties to the lexicographically lowest (i, j) in
    the current node order; the new node takes position i, j is removed; the last three nodes are a trifurcation; T = 2 is
    (A:d/2,B:d/2); branch lengths %.6f, negative ones as they come."""
    D = np.array(D, dtype=np.float64)
    n = len(names)
    if D.shape != (n, n):
        raise ValueError('neighbor_joining: D is not a square matrix over the names')
    if n < 2:
        raise ValueError('neighbor_joining: a tree needs two taxa at least')
    node = [_label(x) for x in names]
    fmt = lambda s, l: '%s:%.6f' % (s, l)
    if n == 2:
        return ('(%s,%s);' % (fmt(node[0], D[0, 1] / 2.), fmt(node[1], D[0, 1] / 2.))).encode('utf-8')
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
        node[i] = '(%s,%s)' % (fmt(node[i], li), fmt(node[j], lj))
        del node[j]
        n -= 1
    la = (D[0, 1] + D[0, 2] - D[1, 2]) / 2.
    lb = (D[0, 1] + D[1, 2] - D[0, 2]) / 2.
    lc = (D[0, 2] + D[1, 2] - D[0, 1]) / 2.
    return ('(%s,%s,%s);' % (fmt(node[0], la), fmt(node[1], lb), fmt(node[2], lc))).encode('utf-8')


def supermatrix_fasta(taxa, matrix, keep):
    """-> bytes: `>taxon\\nrow\\n` per taxon in slot order, the kept columns only"""
    matrix, keep = np.asarray(matrix, dtype=np.uint8), np.asarray(keep, dtype=np.int64)
    return b''.join(b'>' + (t if isinstance(t, bytes) else str(t).encode('utf-8')) + b'\n' + matrix[k, keep].tobytes() + b'\n' for k, t in enumerate(taxa))


def tree(sm, model='p'):
    """Supermatrix -> Newick bytes over its taxa"""
    return neighbor_joining(distances(sm.cmp, sm.same, model, sm.taxa), sm.taxa)


# ---------------------------------------------------------------------------------------------------------
# scripts/rbh2phy.py -A T
# ---------------------------------------------------------------------------------------------------------
def run_align(sc_bytes, fasta_bytes, cols, table, gap_share=1.0, model='p', tree_path='', device_stage=False, out=None):
    """the -A T half of rbh2phy.py: the supermatrix FASTA to `out` (default: stdout), the tree to `tree_path` when named -> Supermatrix"""
    rows_src = TextRows(sc_bytes, cols.names)
    sm = supermatrix(cols.names, table, rbh.fasta_records(fasta_bytes), rows_src, gap_share, device_stage)
    newick = tree(sm, model) if tree_path else None      # (before anything is printed: a refusal leaves no half output)
    o = out if out is not None else sys.stdout.buffer
    o.write(supermatrix_fasta(sm.taxa, sm.matrix, sm.keep))
    o.flush()
    if tree_path:
        with open(tree_path, 'wb') as f:
            f.write(newick + b'\n')
    return sm
