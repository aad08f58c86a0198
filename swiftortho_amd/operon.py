"""operon -- counterpart of SwiftOrtho's scripts/operon_cluster.py: from a file of gene families (one per line) and a file of operons
(first column: x0-->x1-->x2 or x0<--x1<--x2) to the scored operon pairs the script prints -- two operons that share more than two gene
families, one of them to more than half, with the harmonic mean of the two shared fractions.

Nothing here is a transcription of the script, which looks up the operons behind every family of an operon in a dict and, for each of
them, splits both strings again and intersects two sets.  The stage is a table of the operons' distinct families (operon_table, host),
one integer definition on it (candidate_pairs: numpy -- a sparse boolean product, operon x family times its transpose) and one device
call that computes the same (device_operon_pairs: include/sohit.h so_operon_pairs, csrc/operon.hip).  What the script defines, quirks
included (pinned by the goldens: tools/refharness/make_operon_goldens.py runs the REAL script):
  * groups file: line f (from 0) is family f; its genes are the line without its last character (whatever it is: a file without a
    final newline loses a letter), split at tabs; a gene named on two lines belongs to the later one; an empty line defines the gene '';
  * operon file: the operon string is the first tab-separated column of the line without its last character; a string that starts with
    `gene_id` is skipped and takes no number; operon i is split at '-->' when the string holds one, else at '<--' (a string with neither
    is one gene); two equal strings are two operons;
  * len(op) counts every token: genes of no family, repeated genes, empty tokens;
  * index: an operon is listed under family k of each of its genes only `if k:` -- family 0 is never indexed, unknown genes are skipped;
  * the candidates of operon i: the index lists of its genes' families one after the other, in token order, made a set and ITERATED IN
    THE SET'S ORDER.  i is its own candidate whenever it has an indexed gene; an operon of family-0 and unknown genes alone has none;
  * score of candidate j: N = families the two operons share, FAMILY 0 INCLUDED; cv0 = N / len(op_i), cv1 = N / len(op_j),
    score = 2. * cv0 * cv1 / (cv0 + cv1) in doubles, left to right; the line `op_i \\t op_j \\t score` is printed when N > 2 and
    max(cv0, cv1) > .5.  For lengths below 400 that is the integer test N > 2 and 2 * N > min(len_i, len_j) (tests/test_operon.py).
The set's order: a repeated add changes nothing, so list(set(c)) of a candidate list c equals list(set(d)) of its distinct elements d in
order of first occurrence -- `reference_order` replays it with a real Python set of d, no emulation of the table.
Not provided: the networkx graph the script builds and throws away.
"""
import sys

import numpy as np

from .pan import _lines

_CHUNK = 1 << 22     # expansions per block of operons of the numpy definition (a memory bound, nothing more)


# ---------------------------------------------------------------------------------------------------------
# host: text -> the operon table
# ---------------------------------------------------------------------------------------------------------
class OperonTable:
    """`names[i]`: the operon strings; `length[i]` (int32): len(op_i); `has0[i]` (uint8): operon i holds a gene of family 0;
    `start[n_ops + 1]` (int64), `fam[]` (int32): per operon its distinct indexed families (>= 1) in order of first token; `n_fam`:
    families of the groups file (at least 1)"""

    def __init__(self, names, length, has0, start, fam, n_fam):
        self.names, self.length, self.has0, self.start, self.fam, self.n_fam = names, length, has0, start, fam, n_fam

    @property
    def n_ops(self):
        return len(self.length)


def gene_families(groups_text):
    """gene -> family (line number) as the script's dict ends up; -> (dict, number of lines)"""
    groups, n = {}, 0
    for n, line in enumerate(_lines(groups_text), 1):
        for gene in line[:-1].split('\t'):
            groups[gene] = n - 1
    return groups, n


def operon_tokens(op):
    return op.split('-->') if '-->' in op else op.split('<--')


def table_of(names, token_families, lengths, n_fam):
    """operon strings, per operon the families of its tokens (None: an unknown gene) and len(op) -> OperonTable"""
    start, fam, has0 = [0], [], []
    for fams in token_families:
        seen = {}
        for k in fams:
            if k:
                seen.setdefault(k, None)
        fam.extend(seen)
        start.append(len(fam))
        has0.append(1 if any(k == 0 for k in fams) else 0)
    return OperonTable(list(names), np.asarray(lengths, dtype=np.int32).reshape(-1), np.asarray(has0, dtype=np.uint8).reshape(-1),
                       np.asarray(start, dtype=np.int64), np.asarray(fam, dtype=np.int32).reshape(-1), max(int(n_fam), 1))


def operon_table(groups_text, operon_text):
    """the text of the two files -> OperonTable"""
    groups, n_fam = gene_families(groups_text)
    names, fams, lengths = [], [], []
    for line in _lines(operon_text):
        op = line[:-1].split('\t')[0]
        if op.startswith('gene_id'):
            continue
        toks = operon_tokens(op)
        names.append(op), fams.append([groups.get(t) for t in toks]), lengths.append(len(toks))
    return table_of(names, fams, lengths, n_fam)


# ---------------------------------------------------------------------------------------------------------
# the definition (numpy) the device call is held to
# ---------------------------------------------------------------------------------------------------------
class Candidates:
    """every distinct (i, j) that shares an indexed family, i == j included, ordered by (i, rank, j): `i`, `j`, `nshr` (int32: shared
    indexed families, + 1 when both hold a gene of family 0), `rank` (int32: position in i's fam slice of the first family that lists j;
    None from the device), `cand_start[n_ops + 1]` (int64), `stats`"""

    def __init__(self, i, j, nshr, rank, cand_start, stats=None):
        self.i, self.j, self.nshr, self.rank, self.cand_start, self.stats = i, j, nshr, rank, cand_start, stats or {}


def candidate_pairs(table):
    """OperonTable -> Candidates.  Every family's operon list ascends, so (i, rank, j) is the order of first occurrence in the
    concatenation of i's lists"""
    n_ops, start, fam = table.n_ops, np.asarray(table.start, dtype=np.int64), np.asarray(table.fam, dtype=np.int64)
    E = len(fam)
    eop = np.repeat(np.arange(n_ops, dtype=np.int64), np.diff(start))
    erank = np.arange(E, dtype=np.int64) - start[eop]
    order = np.argsort(fam, kind='stable')            # the inverted index: entries by family, operons ascending inside one
    lop = eop[order]
    fsize = np.bincount(fam, minlength=table.n_fam)
    fbeg = np.concatenate(([0], np.cumsum(fsize)))[:-1]
    llen, lbeg = fsize[fam], fbeg[fam]
    optot = np.concatenate(([0], np.cumsum(llen)))[start]          # expansions in front of every operon
    has0 = np.asarray(table.has0) != 0
    out = [[], [], [], []]
    lo = 0
    while lo < n_ops:
        hi = int(np.searchsorted(optot, optot[lo] + _CHUNK, side='right')) - 1
        hi = min(max(hi, lo + 1), n_ops)
        e0, e1 = int(start[lo]), int(start[hi])
        ln = llen[e0:e1]
        X = int(ln.sum())
        if X:
            src = np.repeat(np.arange(e0, e1), ln)
            within = np.arange(X, dtype=np.int64) - np.repeat(np.cumsum(ln) - ln, ln)
            i, j, r = eop[src], lop[lbeg[src] + within], erank[src]
            key, first, count = np.unique(i * n_ops + j, return_index=True, return_counts=True)   # (first: the first occurrence)
            pi, pj, pr = key // n_ops, key % n_ops, r[first]
            o = np.lexsort((pj, pr, pi))
            pi, pj, pr, count = pi[o], pj[o], pr[o], count[o]
            for k, a in enumerate((pi, pj, count + (has0[pi] & has0[pj]), pr)):
                out[k].append(a.astype(np.int32))
        lo = hi
    i, j, nshr, rank = (np.concatenate(a) if a else np.zeros(0, dtype=np.int32) for a in out)
    cand_start = np.concatenate(([0], np.cumsum(np.bincount(i, minlength=n_ops)))).astype(np.int64)
    return Candidates(i, j, nshr, rank, cand_start)


def passes(nshr, len_i, len_j):
    """the script's filter N > 2 and max(cv0, cv1) > .5 as the integer test (lengths below 400: tests/test_operon.py)"""
    nshr = np.asarray(nshr, dtype=np.int64)
    return (nshr > 2) & (2 * nshr > np.minimum(np.asarray(len_i, dtype=np.int64), np.asarray(len_j, dtype=np.int64)))


def scores(nshr, len_i, len_j):
    """2. * cv0 * cv1 / (cv0 + cv1) in float64, left to right"""
    n = np.asarray(nshr, dtype=np.float64)
    cv0, cv1 = n / np.asarray(len_i, dtype=np.float64), n / np.asarray(len_j, dtype=np.float64)
    return 2. * cv0 * cv1 / (cv0 + cv1)


def reference_order(cand_start, j):
    """-> the permutation of the candidate rows that puts every operon's candidates into the order a Python set of them iterates in
    (rows come in order of first occurrence, distinct per operon)"""
    cand_start, out = np.asarray(cand_start).tolist(), np.empty(len(j), dtype=np.int64)
    js = np.asarray(j).tolist()
    for a, b in zip(cand_start[:-1], cand_start[1:]):
        if b - a > 1:
            c = js[a:b]
            where = {v: a + k for k, v in enumerate(c)}
            out[a:b] = [where[v] for v in set(c)]
        elif b > a:
            out[a] = a
    return out


# ---------------------------------------------------------------------------------------------------------
# the stage on the GPU (include/sohit.h so_operon_pairs, csrc/operon.hip).  No fallback: without the library or a device this raises.
# ---------------------------------------------------------------------------------------------------------
ALL_CANDIDATES = 1     # flags bit 0: every candidate in first-occurrence order (else: the passing pairs in index order)


def device_operon_pairs(start, fam, length, has0, n_fam, flags=0, device=0, n_ops=None):
    """so_operon_pairs -> Candidates (rank None; without ALL_CANDIDATES: the passing pairs by (i, j), cand_start None); a refusal raises
    RuntimeError with the library's message"""
    import ctypes as C_
    from . import _lib
    L = _lib.load()
    col = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)      # (None: a null pointer -- the refusal tests; then n_ops says what the arrays hold)
    s64, f32, l32, h8 = col(start, np.int64), col(fam, np.int32), col(length, np.int32), col(has0, np.uint8)
    if n_ops is None:
        n = len(l32)
        if len(s64) != n + 1 or len(h8) != n:
            raise ValueError('device_operon_pairs: start holds n_ops + 1 offsets, length and has0 one entry per operon')
    else:
        n = int(n_ops)
    ptr = lambda a: C_.c_void_p(a.ctypes.data if a is not None else None)
    out = _lib.SoOperonResult()
    rc = L.so_operon_pairs(int(device), n, ptr(s64), ptr(f32), ptr(l32), ptr(h8), int(n_fam), int(flags), C_.byref(out))
    if rc != 0:
        raise RuntimeError(L.so_operon_last_error().decode())
    try:
        arr = _lib.result_array
        rows = int(out.n_candidates if flags & ALL_CANDIDATES else out.n_pairs)
        stats = {k: int(getattr(out, k)) for k in ('n_pairs', 'n_candidates', 'n_expansions', 'batches', 'waits')}
        return Candidates(arr(out.i, rows, np.int32), arr(out.j, rows, np.int32), arr(out.nshr, rows, np.int32), None,
                          arr(out.cand_start, n + 1, np.int64) if flags & ALL_CANDIDATES else None, stats)
    finally:
        L.so_operon_free(C_.byref(out))


def _device_candidates(table, flags, device):
    return device_operon_pairs(table.start, table.fam, table.length, table.has0, table.n_fam, flags, device)


def operon_pairs(table, order='reference', device_stage=False, device=0):
    """OperonTable -> (i, j, score) of the pairs the script prints: order='reference' in the script's order (every operon's candidates
    in the order of a Python set), order='index' by (i, j).  The integers come from candidate_pairs() or (device_stage) from the device
    call; the score is float64 arithmetic on the host either way"""
    if order not in ('reference', 'index'):
        raise ValueError("operon_pairs: order is 'reference' or 'index'")
    length = np.asarray(table.length)
    if order == 'index' and device_stage:
        c = _device_candidates(table, 0, device)
        i, j, nshr = c.i, c.j, c.nshr
    else:
        c = _device_candidates(table, ALL_CANDIDATES, device) if device_stage else candidate_pairs(table)
        i, j, nshr = c.i, c.j, c.nshr
        if order == 'reference':
            o = reference_order(c.cand_start, j)
            i, j, nshr = i[o], j[o], nshr[o]
        keep = passes(nshr, length[i], length[j])
        i, j, nshr = i[keep], j[keep], nshr[keep]
        if order == 'index':
            o = np.lexsort((j, i))
            i, j, nshr = i[o], j[o], nshr[o]
    return i, j, scores(nshr, length[i], length[j])


# ---------------------------------------------------------------------------------------------------------
# text
# ---------------------------------------------------------------------------------------------------------
def xyz_lines(names, i, j, score):
    """the lines the script prints (str() of a Python float is its repr)"""
    return ['%s\t%s\t%s' % (names[a], names[b], repr(s)) for a, b, s in zip(np.asarray(i).tolist(), np.asarray(j).tolist(), np.asarray(score, dtype=np.float64).tolist())]


# ---------------------------------------------------------------------------------------------------------
# the script
# ---------------------------------------------------------------------------------------------------------
def manual_print():
    print('Scored pairs of operons that share gene families')
    print('Usage:')
    print('  python this_script.py -g foo.groups -p foo.operon [-G T]')
    print('Parameters:')
    print(' -g: groups file, one protein/gene family per line, tab-separated')
    print(' -p: operon file; its first column reads x0-->x1-->x2 or x0<--x1<--x2')
    print(' -G: shared-family counts of the operon pairs on the GPU [T|F]. Default: F')


def run(groups_path, operon_path, device_stage=False, device=0):
    """the script on two files -> its output lines"""
    with open(groups_path, 'r') as f:
        groups = f.read()
    with open(operon_path, 'r') as f:
        operons = f.read()
    table = operon_table(groups, operons)
    i, j, score = operon_pairs(table, 'reference', device_stage, device)
    return xyz_lines(table.names, i, j, score)


def main(argv=None):
    from .fsearch import parse_flags
    argv = list(sys.argv if argv is None else argv)
    args = parse_flags(argv, {'-g': '', '-p': '', '-G': 'F'})
    if args['-g'] == '' or args['-p'] == '':
        manual_print()
        raise SystemExit()
    lines = run(args['-g'], args['-p'], str(args['-G']).upper()[:1] == 'T')
    sys.stdout.write(''.join(l + '\n' for l in lines))
    sys.stdout.flush()
    return 0
