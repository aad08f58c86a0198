"""Exact-duplicate collapse / expand around the search: counterparts of SwiftOrtho's
scripts/nr_flt.py and scripts/nr2full.py, the two helpers scripts/run_all_fast.py wraps around find_hit
(run_all_fast.py:109-118): identical sequences are searched once and the hits are multiplied back afterwards.
`search_collapsed()` is that wrapper: nr_flt -> find_hit -> nr2full with the reference's file names.

nr_flt (scripts/nr_flt.py:1-27): records with the same residue string are merged in order of first
appearance; the merged header is the record ids joined by ';;;'; the sequence is printed on one line.
The reference reads the file with Bio.SeqIO.parse(.., 'fasta') (Biopython is absent from this image): the
record rules below are Biopython's documented ones -- title = the '>' line without '>' and trailing blanks,
id = its first word, sequence = the following lines right-stripped and joined with blanks and carriage
returns removed, text before the first '>' ignored.  Pinned by the golden `nr_dups.nr.fsa` = stdout of the
REAL nr_flt.py on plain FASTA (where every parser agrees; tools/refharness/make_nr_goldens.py); the handling
of inner blanks / CR / leading text follows the documented rules and is NOT pinned by a run of Biopython.

nr2full (scripts/nr2full.py:14-44): every row of the collapsed search is expanded to the cross product of the
';;;'-separated query ids and subject ids; columns 3..14 are kept, the last two columns (query ordinal,
subject header) are replaced by the individual query and subject names; inside a run of rows with the same
collapsed query the expanded rows come out grouped by individual query, groups in order of first
appearance.  Pinned by the golden `nr_dups.full.sc` = stdout of the REAL nr2full.py.

The text functions above are host utilities.  The same two steps as TABLES, for the one-process pipeline (pipeline.py, collapse=True):
`collapse_tables()` is nr_flt as member tables (grouping on the host), `expand_records()` the numpy definition of nr2full on so_hit
records, and `device_expand()` runs that expansion on the GPU (so_nr_expand, csrc/nr.hip): the records of the collapsed search stay in
HBM, are multiplied out there in nr2full's exact order, and find_orth's device stages read them where they lie.
"""
import collections
import itertools
import os
import sys

JOIN = ';;;'
EXPAND_PIECE = 256   # output records one workgroup of the emit kernel writes (csrc/nr.hip NR_PIECE; the tests place outputs at its edges)


def fasta_records(lines):
    """(title, sequence) per record, by Biopython's FASTA rules (see the module docstring)"""
    title, seq = None, []
    for line in lines:
        if line[:1] == '>':
            if title is not None:
                yield title, ''.join(seq).replace(' ', '').replace('\r', '')
            title, seq = line[1:].rstrip(), []
        elif title is not None:
            seq.append(line.rstrip())
    if title is not None:
        yield title, ''.join(seq).replace(' ', '').replace('\r', '')


def nr_flt(lines):
    """FASTA lines -> output lines of nr_flt.py: one '>id;;;id...' + residue line per distinct sequence"""
    members = {}
    for title, seq in fasta_records(lines):
        words = title.split(None, 1)
        members.setdefault(seq, []).append(words[0] if words else '')
    return [l for seq, ids in members.items() for l in ('>' + JOIN.join(ids), seq)]


def nr2full(lines):
    """.sc rows of the collapsed search -> expanded rows (no newline)"""
    out = []
    rows = (l[:-1].split('\t') for l in lines)
    for _, run in itertools.groupby(rows, key=lambda c: c[0]):
        expanded, rank = [], {}
        for c in run:
            mid = c[2:-2]
            for qname in c[0].split(JOIN):
                q = qname.split(' ')[0]
                k = rank.setdefault(q, len(rank))
                for sname in c[1].split(JOIN):
                    expanded.append((k, '\t'.join([q, sname.split(' ')[0]] + mid + [qname, sname])))
        expanded.sort(key=lambda t: t[0])   # stable: rows of one individual query stay in generation order
        out.extend(t[1] for t in expanded)
    return out


CollapseTables = collections.namedtuple('CollapseTables', 'ids rep_of off mem fasta')


def collapse_tables(lines_or_bytes):
    """nr_flt as tables.  Input: the FASTA file as bytes, or its text lines (what nr_flt takes).  Records are read by fasta_records(), the
    id is the first word of the title; distinct residue strings are numbered by first appearance, compared case-sensitively.
    -> CollapseTables: ids[record] (bytes, file order), rep_of[record] = the number of the record's distinct sequence (int32),
    off[n_distinct + 1] (int64) / mem[n_records] (int32) = the record ordinals of each distinct sequence in file order, fasta = the
    collapsed FASTA as bytes, exactly the lines nr_flt() yields.
    The grouping stays on the host, a dict over the residue strings: hashing on the device would upload every residue a second time
    (the search uploads the collapsed file anyway) for no gain -- the dict is one pass over bytes that are already in host memory.
    Refused with a ValueError that names the id, because nr2full keys its runs and its per-query groups on id STRINGS while the device
    works on record NUMBERS, and the two stop agreeing: an empty id, an id that contains ';;;', an id on two records.  (nr_flt / nr2full
    keep serving such files.)"""
    import numpy as np
    if isinstance(lines_or_bytes, (bytes, bytearray, memoryview)):
        enc = 'latin-1'
        lines = bytes(lines_or_bytes).decode(enc).split('\n')
    else:
        enc, lines = 'utf-8', lines_or_bytes
    number, ids, rep, seqs, seen = {}, [], [], [], set()
    for title, seq in fasta_records(lines):
        words = title.split(None, 1)
        i = words[0] if words else ''
        if i == '':
            raise ValueError('collapse_tables: record %d has an empty id' % len(ids))
        if JOIN in i:
            raise ValueError("collapse_tables: the id %r contains '%s', the separator of the collapsed headers" % (i, JOIN))
        if i in seen:
            raise ValueError('collapse_tables: the id %r names two records' % (i,))
        seen.add(i)
        d = number.setdefault(seq, len(number))
        if d == len(seqs):
            seqs.append(seq)
        ids.append(i)
        rep.append(d)
    rep_of = np.asarray(rep, dtype=np.int32)
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum(np.bincount(rep_of, minlength=len(seqs)), out=off[1:])
    mem = np.argsort(rep_of, kind='stable').astype(np.int32)
    fasta = ''.join('>%s\n%s\n' % (JOIN.join(ids[m] for m in mem[off[d]:off[d + 1]].tolist()), seqs[d]) for d in range(len(seqs))).encode(enc)
    return CollapseTables([i.encode(enc) for i in ids], rep_of, off, mem, fasta)


def _member_table(off, mem, side):
    import numpy as np
    off, mem = np.asarray(off, dtype=np.int64), np.asarray(mem, dtype=np.int64)
    if len(off) < 1 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != len(mem):
        raise ValueError('expand_records: the %s member table does not rise from 0 to its number of members' % side)
    if len(mem) and not np.array_equal(np.sort(mem), np.arange(len(mem))):
        raise ValueError('expand_records: the %s member table does not name every member exactly once' % side)
    return off, mem


def expand_records(rec, qoff, qmem, soff, smem):
    """nr2full on so_hit records (the structured array Hits.array() returns): the numpy definition of so_nr_expand.
    rec: the records of the collapsed search in the order the search returns them (ascending qidx); qmem[qoff[c]:qoff[c + 1]] = the
    ordinals in the full file of the members of collapsed query c, soff / smem the same for the subjects.  A run = a maximal stretch of
    consecutive records with one qidx.  For the run of collapsed query c with members m_0 .. m_{k-1}, rows j = 0 .. t-1, n_j = members of
    row j's subject, S = sum n_j, P_j = sum_{i<j} n_i: the record of (member a, row j, subject member b) stands at
    base_c + a * S + P_j + b (base_c = the expanded records of all earlier runs) and equals row j with qidx = m_a, sidx = subject
    member b, every other field unchanged -- nr2full's order: inside a run the rows grouped by individual query in first-appearance
    order, inside a group in generation order.  All totals are 64-bit."""
    import numpy as np
    rec = np.asarray(rec)
    qoff, qmem = _member_table(qoff, qmem, 'query')
    soff, smem = _member_table(soff, smem, 'subject')
    n = len(rec)
    if n == 0:
        return rec.copy()
    q, s = rec['qidx'].astype(np.int64), rec['sidx'].astype(np.int64)
    if q.min() < 0 or q.max() >= len(qoff) - 1:
        raise ValueError('expand_records: a qidx lies outside the query member table')
    if s.min() < 0 or s.max() >= len(soff) - 1:
        raise ValueError('expand_records: a sidx lies outside the subject member table')
    k, nj = qoff[q + 1] - qoff[q], soff[s + 1] - soff[s]
    head = np.concatenate([[True], q[1:] != q[:-1]])
    start, run = np.flatnonzero(head), np.cumsum(head) - 1
    before = np.cumsum(nj) - nj                       # members of all earlier rows
    P = before - before[start][run]                   # ... of the earlier rows of the run
    S_run = np.add.reduceat(nj, start)
    w_run = k[start] * S_run
    base, S = (np.cumsum(w_run) - w_run)[run], S_run[run]
    w = k * nj
    total = int(w.sum())
    src = np.repeat(np.arange(n, dtype=np.int64), w)  # every (a, b) of a row, a-major
    t = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(w) - w, w)
    a, b = t // nj[src], t % nj[src]
    pos = base[src] + a * S[src] + P[src] + b
    out = np.empty(total, dtype=rec.dtype)
    out[pos] = rec[src]
    out['qidx'][pos] = qmem[qoff[q[src]] + a]
    out['sidx'][pos] = smem[soff[s[src]] + b]
    return out


class ExpandedHits:
    """the records so_nr_expand left in device memory; owned until close().  find_orth's device stages take it like a fsearch.DeviceHits"""

    def __init__(self, L, res, device):
        self.L, self.res, self.device = L, res, int(device)
        self.n, self.n_in, self.n_runs, self.waits = int(res.n_out), int(res.n_in), int(res.n_runs), int(res.waits)

    def device_pointer(self):
        return int(self.res.d_out or 0) if self.res is not None else 0

    def __len__(self):
        return self.n

    def close(self):
        if self.res is not None:
            import ctypes as C
            self.L.so_nr_expand_free(C.byref(self.res))
            self.res = None

    __del__ = close


def expand_device_pointer(d_ptr, n, device, qoff, qmem, soff, smem, count_only=False):
    """so_nr_expand on n records at the device address d_ptr -> ExpandedHits (count_only: its length is the answer, it holds no records).
    RuntimeError with the library's message for everything the call refuses."""
    import ctypes as C
    import numpy as np
    from . import _lib
    L = _lib.load()
    qo, so = np.ascontiguousarray(qoff, dtype=np.int64), np.ascontiguousarray(soff, dtype=np.int64)
    qm, sm = np.ascontiguousarray(qmem, dtype=np.int32), np.ascontiguousarray(smem, dtype=np.int32)
    if len(qo) < 1 or len(so) < 1:
        raise ValueError('expand_device_pointer: a member table needs its closing offset')
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    res = _lib.SoNrExpandResult()
    rc = L.so_nr_expand(int(device), C.c_void_p(int(d_ptr) or None), int(n), ptr(qo), ptr(qm), len(qo) - 1, ptr(so), ptr(sm), len(so) - 1, 1 if count_only else 0,
                        C.byref(res))
    if rc != 0:
        raise RuntimeError(L.so_nr_last_error().decode())
    return ExpandedHits(L, res, device)


def device_expand(dev, tables, subject_tables=None):
    """the records `dev` holds (a fsearch.DeviceHits of the search of collapse_tables()'s FASTA, or anything with device_pointer(),
    __len__ and a device index) expanded on the GPU by so_nr_expand -> ExpandedHits: device_pointer(), __len__, .device, close().
    `tables`: the CollapseTables of the queries; `subject_tables` those of the reference when it is another file (default: a
    self-search).  No torch is needed."""
    st = tables if subject_tables is None else subject_tables
    device = dev.device if hasattr(dev, 'device') else dev.s.device
    return expand_device_pointer(dev.device_pointer(), len(dev), device, tables.off, tables.mem, st.off, st.mem)


def collapsed_search_kw(seed='1111111', hits='1000'):
    """the Searcher keywords of the search search_collapsed() runs: bin/find_hit.py -e 1e-5 -m 5e-2 -s seed -v hits, its other defaults"""
    from . import find_hit
    p = find_hit.resolve(dict(find_hit.DEFAULTS, **{'-p': 'blastp', '-i': 'x', '-d': 'x', '-e': '1e-5', '-m': '5e-2', '-s': seed, '-v': str(hits)}))
    kw = find_hit.searcher_kwargs(p)
    del kw['device']
    return kw


def search_collapsed(fas, seed='1111111', cpus='1', hits='1000', device_flags=(), python=sys.executable):
    """run_all_fast.py:95-118 -- `<fas>_nr.fsa` (collapsed proteome), `<fas>_results/<name>_nr.fsa.sc` (its self-search:
    bin/find_hit.py -e 1e-5 -m 5e-2 -s seed -a cpus -v hits), `<fas>_results/<name>.sc` (hits multiplied back).
    Returns the path of the last file."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name = fas.split(os.sep)[-1]
    res = fas + '_results'
    os.makedirs(res, exist_ok=True)
    nr_fa = fas + '_nr.fsa'
    with open(fas, 'r') as f, open(nr_fa, 'w') as o:
        for l in nr_flt(f):
            o.write(l + '\n')
    nr_sc = os.path.join(res, name + '_nr.fsa.sc')
    cmd = [python, os.path.join(root, 'bin', 'find_hit.py'), '-p', 'blastp', '-i', nr_fa, '-d', nr_fa, '-o', nr_sc, '-e', '1e-5', '-s', seed,
           '-m', '5e-2', '-a', str(cpus), '-v', str(hits)] + list(device_flags)
    with open(os.path.join(res, 'log'), 'w') as log:
        rc = subprocess.run(cmd, stdout=log, stderr=subprocess.STDOUT).returncode
    if rc != 0 or not os.path.isfile(nr_sc):
        raise RuntimeError('find_hit failed (exit %d): see %s' % (rc, os.path.join(res, 'log')))
    full = os.path.join(res, name + '.sc')
    with open(nr_sc, 'r') as f, open(full, 'w') as o:
        for l in nr2full(f):
            o.write(l + '\n')
    return full


def main_nr_flt(argv=None):
    argv = list(sys.argv if argv is None else argv)
    f = open(argv[1], 'r') if len(argv) > 1 else sys.stdin
    for l in nr_flt(f):
        print(l)
    return 0


def main_nr2full(argv=None):
    argv = list(sys.argv if argv is None else argv)
    if len(argv) < 2:
        print('python this.py foo.sc')
        return 0
    with open(argv[1], 'r') as f:
        for l in nr2full(f):
            print(l)
    return 0
