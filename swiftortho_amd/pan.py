"""pan -- counterpart of SwiftOrtho's scripts/pan_genome.py: from a FASTA file and a file of ortholog groups (one group per line) to the
pan-genome statistics -- how many families are core, shared and specific, the family-by-taxon count table, and the rarefaction curves
(core families, new families and pan-genome size against the number of genomes) its curve fits are made from.

Nothing here is a transcription of the script, which writes two temporary files, maps one back and walks a rows x 20 array about ten
times per genome added.  The stage is a table of (row, taxon) pairs of the kept members (member_table, host), three integer
definitions on it (count_matrix, row_types, rarefaction: numpy) and one device call that computes the same three (device_pan_genome:
include/sohit.h so_pan_genome, csrc/pan.hip).  What the script defines, quirks included (pinned by the goldens:
tools/refharness/make_pan_goldens.py runs the REAL script):
  * taxa: of every line that starts with '>', the line without its first and LAST character (a last line without a newline loses a
    letter), up to the first blank, up to the first '|'; with -r file, only the names that file lists (one per line, stripped; an empty
    or absent file filters nothing).  N = their number.  The script's column order is Python's set order of the names, which differs
    from process to process: every function here takes the order as a list, only main() builds it from a set;
  * a row per line of the groups file, in file order: the members are the line without its last character (again whatever it is), split
    at tabs; a member's taxon is the text before its first '|'; a member of a filtered-out taxon is skipped (the row stays, possibly all
    zero); every kept member adds 1 to its cell -- listed twice, it counts twice -- and is remembered as visited; a kept member whose
    taxon is not in the FASTA makes the script raise KeyError: member_table refuses (ValueError);
  * then a row per FASTA record (id: the header without '>' up to the first white space) that was not visited and whose taxon is not
    filtered out: a single 1, type Specific;
  * type of a file row, thr = its taxa with a non-zero count: Ts = ts < 1 and max(ts * N, 1) or ts, Tc = tc < 1 and tc * N or tc (Python
    floats, for fractions, absolute counts, 0 and negative values alike); thr <= Ts: Specific, Ts < thr < Tc: Share, else Core.  thr is an
    integer, so the rule is thr <= floor(Ts), thr < ceil(Tc) (type_thresholds);
  * rarefaction, on the presence matrix (count > 0): seed 42, then 20 successive shuffles of ONE list 0 .. N - 1 (each starts from the
    order the last one left); ys = presence in each order's first genome; for i = 1 .. N - 1 and j = i + 1, Ts and Tc as above with j in
    place of N: spec = #(ys <= Ts - 1 and yn > 0), THEN ys += yn, core = #(ys >= Tc), panz = #(ys > 0).  ys is an integer, so the tests
    are ys <= floor(Ts - 1) and ys >= ceil(Tc) with the float expressions evaluated first (step_thresholds).  This is the branch the
    script takes when numexpr is not importable; with numexpr it tests ys <= Ts instead: that branch is NOT provided;
  * <groups file>_xy.txt: `j core spec panz` per line, tab-separated, the 20 orders of a j one after the other; empty for N < 2 (the
    script then dies in its fit).  Here the file is always kept (the script removes it when Rscript is installed).
Not provided: the three curve fits of the report (scipy's solver is not reproducible bit for bit; _xy.txt is their whole input, and a
line of the report says so), the R plot, the temporary pan.npy / type.txt.

Added, with no counterpart in the reference (-t, -d, -m, -B, -S; off unless asked for): the gene content of the genomes.  shared_counts:
S[a, b] = the rows present in both genomes a and b (all rows, presence = count > 0), S[a, a] = the families of a; boot_shared: the same
over the rows a bootstrap replicate draws (phy.boot_columns over the rows; a row drawn twice counts twice); content_distances: jaccard,
1 - S_ab / (S_aa + S_bb - S_ab), or overlap, 1 - S_ab / min(S_aa, S_bb) (Snel et al. 1999), in float64 from the exact integers;
content_tree: phy.neighbor_joining over them, with bootstrap support over the families as phy.tree labels it.  Tree and table list the
taxa in SORTED order of their names, so the files repeat from run to run.  The numpy functions are the definition; the device call
(device_shared_counts, device_boot_shared: include/sohit.h so_pan_shared) equals them integer for integer, and the replicates' trees
come from the existing so_phy_nj_splits.
"""
import math
import random
import sys

import numpy as np

TYPE_NAMES = ('Specific', 'Share', 'Core')
SPECIFIC, SHARE, CORE = 0, 1, 2
SIZE = 20           # genome orders of the rarefaction
_I32_MAX = 2 ** 31 - 1


# ---------------------------------------------------------------------------------------------------------
# host: text -> taxa and the member table
# ---------------------------------------------------------------------------------------------------------
def _lines(text):
    """the lines a text-mode file yields: split behind every '\\n', the last one without it when the text does not end in one"""
    parts = text.split('\n')
    return [p + '\n' for p in parts[:-1]] + ([parts[-1]] if parts[-1] else [])


def read_allow(path):
    """the -r file -> set of names, or None (no file, or an empty one: no filter)"""
    import os
    if not path or not os.path.isfile(path):
        return None
    with open(path, 'r') as f:
        allow = set(line.strip() for line in f)
    return allow or None


def taxa_of_fasta(fasta_text, allow=None):
    """the distinct taxa of the header lines, in order of first appearance"""
    seen = {}
    for line in _lines(fasta_text):
        if line.startswith('>'):
            tax = line[1:-1].split(' ')[0].split('|')[0]
            if allow and tax not in allow:
                continue
            seen.setdefault(tax, None)
    return list(seen)


def fasta_ids(fasta_text):
    """the record ids in file order: the header line without '>' and trailing blanks, up to the first white space ('' for a bare '>')"""
    out = []
    for line in _lines(fasta_text):
        if line.startswith('>'):
            words = line[1:].rstrip().split(None, 1)
            out.append(words[0] if words else '')
    return out


def group_lists(groups_text):
    """the members of every line of a groups file, as the script splits them"""
    return [line[:-1].split('\t') for line in _lines(groups_text)]


class MemberTable:
    """`row[m]`, `taxon[m]` (int32): the kept members; `n_rows` rows, the first `n_file_rows` of them lines of the groups file"""

    def __init__(self, row, taxon, n_rows, n_file_rows):
        self.row, self.taxon, self.n_rows, self.n_file_rows = row, taxon, n_rows, n_file_rows


def member_table_of(groups, ids, taxa, allow=None):
    """groups (lists of member ids) + the FASTA's record ids + the taxon order -> MemberTable"""
    where = {t: k for k, t in enumerate(taxa)}
    row, tx, visit = [], [], set()

    def code(member):
        tax = member.split('|')[0]
        if allow and tax not in allow:
            return -1
        if tax not in where:
            raise ValueError('pan_genome: member %r has a taxon that is not among the taxa of the FASTA file (pan_genome.py raises KeyError on such input)' % (member,))
        return where[tax]

    n = 0
    for group in groups:
        for member in group:
            t = code(member)
            if t >= 0:
                row.append(n), tx.append(t), visit.add(member)
        n += 1
    n_file = n
    for member in ids:
        if member in visit:
            continue
        t = code(member)
        if t >= 0:
            row.append(n), tx.append(t)
            n += 1
    return MemberTable(np.asarray(row, dtype=np.int32), np.asarray(tx, dtype=np.int32), n, n_file)


def member_table(fasta_text, groups_text, taxa, allow=None):
    """the text of the two files + the taxon order (taxa_of_fasta with the same `allow`, in any order) -> MemberTable"""
    return member_table_of(group_lists(groups_text), fasta_ids(fasta_text), taxa, allow)


# ---------------------------------------------------------------------------------------------------------
# thresholds: the script's float expressions, then the integers an integer count is compared with
# ---------------------------------------------------------------------------------------------------------
def thresholds(ts, tc, n):
    """-> (Ts, Tc) for n genomes, as Python evaluates the script's two expressions"""
    ts, tc = float(ts), float(tc)
    if ts != ts or tc != tc:
        raise ValueError('pan_genome: a threshold is not a number')
    return (ts < 1 and max(ts * n, 1) or ts), (tc < 1 and tc * n or tc)


def _floor32(x):
    return int(min(max(math.floor(x), -_I32_MAX), _I32_MAX)) if abs(x) != math.inf else (_I32_MAX if x > 0 else -_I32_MAX)


def _ceil32(x):
    return int(min(max(math.ceil(x), -_I32_MAX), _I32_MAX)) if abs(x) != math.inf else (_I32_MAX if x > 0 else -_I32_MAX)


def type_thresholds(ts, tc, n):
    """-> (spec_max, core_min): thr <= Ts is thr <= spec_max, thr < Tc is thr < core_min for every integer thr (cut to 32 bits: counts are
    far inside)"""
    Ts, Tc = thresholds(ts, tc, n)
    return _floor32(Ts), _ceil32(Tc)


def step_thresholds(ts, tc, n_taxa):
    """-> (S, C) int32[n_taxa]: at step i (j = i + 1 genomes) ys <= Ts - 1 is ys <= S[i] and ys >= Tc is ys >= C[i]; entry 0 is unused"""
    S, C = np.zeros(n_taxa, dtype=np.int32), np.zeros(n_taxa, dtype=np.int32)
    for i in range(1, n_taxa):
        Ts, Tc = thresholds(ts, tc, i + 1)
        S[i], C[i] = _floor32(Ts - 1), _ceil32(Tc)
    return S, C


def permutations(n_taxa, size=SIZE):
    """the genome orders: seed 42, `size` successive shuffles of one list -> int32[size, n_taxa]"""
    rng = random.Random(42)
    idx = list(range(n_taxa))
    out = np.zeros((size, n_taxa), dtype=np.int32)
    for p in range(size):
        rng.shuffle(idx)
        out[p] = idx
    return out


# ---------------------------------------------------------------------------------------------------------
# the definitions (numpy) the device call is held to
# ---------------------------------------------------------------------------------------------------------
def count_matrix(row, taxon, n_rows, n_taxa):
    """-> int32[n_rows, n_taxa]: how often every (row, taxon) pair occurs"""
    key = np.asarray(row, dtype=np.int64) * n_taxa + np.asarray(taxon, dtype=np.int64)
    return np.bincount(key, minlength=n_rows * n_taxa).astype(np.int32).reshape(n_rows, n_taxa)


def row_types(counts, n_file_rows, spec_max, core_min):
    """-> (type uint8[n_rows], (core, share, specific) counted over the FILE rows); the rows behind them are Specific"""
    thr = (np.asarray(counts) > 0).sum(1)
    typ = np.where(thr <= spec_max, SPECIFIC, np.where(thr < core_min, SHARE, CORE)).astype(np.uint8)
    typ[n_file_rows:] = SPECIFIC
    f = typ[:n_file_rows]
    return typ, (int((f == CORE).sum()), int((f == SHARE).sum()), int((f == SPECIFIC).sum()))


def rarefaction(counts, perm, S, C):
    """-> (core, spec, panz) int64[size, n_taxa - 1]: entry [p, i - 1] is step i of order p"""
    x = np.asarray(counts) > 0
    perm = np.asarray(perm)
    size, d = len(perm), x.shape[1]
    out = [np.zeros((size, max(d - 1, 0)), dtype=np.int64) for _ in range(3)]
    if size == 0 or d < 2:
        return tuple(out)
    ys = x[:, perm[:, 0]].astype(np.int32)
    for i in range(1, d):
        yn = x[:, perm[:, i]].astype(np.int32)
        out[1][:, i - 1] = ((ys <= S[i]) & (yn > 0)).sum(0)
        ys = ys + yn
        out[0][:, i - 1] = (ys >= C[i]).sum(0)
        out[2][:, i - 1] = (ys > 0).sum(0)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------
# the stage on the GPU (include/sohit.h so_pan_genome, csrc/pan.hip).  No fallback: without the library or a device this raises.
# ---------------------------------------------------------------------------------------------------------
class PanResult:
    """`counts` int32[n_rows, n_taxa] or None, `types` uint8[n_rows], `totals` (core, share, specific) over the file rows, `core` / `spec`
    / `panz` int64[size, n_taxa - 1], `stats` (tier, waits)"""

    def __init__(self, counts, types, totals, core, spec, panz, stats=None):
        self.counts, self.types, self.totals, self.core, self.spec, self.panz, self.stats = counts, types, totals, core, spec, panz, stats or {}


def device_pan_genome(row, taxon, n_rows, n_file_rows, n_taxa, spec_max, core_min, perm, S, C, want_counts=True, device=0, flags=0):
    """count_matrix(), row_types() and rarefaction() in one device call -> PanResult; a refusal raises RuntimeError with the library's message"""
    from . import _lib
    row32, tax32 = np.ascontiguousarray(row, dtype=np.int32), np.ascontiguousarray(taxon, dtype=np.int32)
    if len(row32) != len(tax32):
        raise ValueError('device_pan_genome: row and taxon differ in length')
    perm32 = np.ascontiguousarray(perm, dtype=np.int32).reshape(-1, n_taxa) if n_taxa else np.zeros((len(perm), 0), dtype=np.int32)
    S32, C32 = np.ascontiguousarray(S, dtype=np.int32), np.ascontiguousarray(C, dtype=np.int32)
    if len(S32) != n_taxa or len(C32) != n_taxa:
        raise ValueError('device_pan_genome: S and C hold one entry per taxon')
    size = len(perm32)
    with _lib.call('so_pan_genome', _lib.SoPanResult, 'so_pan_free', 'so_pan_last_error', int(device), len(row32), row32, tax32, int(n_rows), int(n_file_rows), int(n_taxa),
                   int(spec_max), int(core_min), size, perm32, S32, C32, 1 if want_counts else 0, int(flags)) as out:
        arr = _lib.result_array
        steps = max(n_taxa - 1, 0)
        curve = lambda p: arr(p, size * steps, np.int64).reshape(size, steps)
        return PanResult(arr(out.counts, n_rows * n_taxa, np.int32).reshape(n_rows, n_taxa) if want_counts else None, arr(out.type, n_rows, np.uint8),
                         (int(out.n_core), int(out.n_share), int(out.n_spec)), curve(out.core), curve(out.spec), curve(out.panz),
                         {'tier': int(out.tier), 'waits': int(out.waits)})


def pan_genome(table, n_taxa, ts=.05, tc=.95, size=SIZE, device_stage=False, want_counts=True, device=0):
    """MemberTable -> PanResult, by the numpy definitions or (device_stage) by the device call"""
    spec_max, core_min = type_thresholds(ts, tc, n_taxa)
    S, C = step_thresholds(ts, tc, n_taxa)
    perm = permutations(n_taxa, size)
    if device_stage:
        return device_pan_genome(table.row, table.taxon, table.n_rows, table.n_file_rows, n_taxa, spec_max, core_min, perm, S, C, want_counts, device)
    counts = count_matrix(table.row, table.taxon, table.n_rows, n_taxa)
    types, totals = row_types(counts, table.n_file_rows, spec_max, core_min)
    core, spec, panz = rarefaction(counts, perm, S, C)
    return PanResult(counts if want_counts else None, types, totals, core, spec, panz)


# ---------------------------------------------------------------------------------------------------------
# gene content: the families every pair of genomes shares, the distances made from them, the tree of the genomes.  The reference has no
# such product: these numpy functions are the definition, the device call (so_pan_shared) equals them integer for integer.
# ---------------------------------------------------------------------------------------------------------
METRICS = ('jaccard', 'overlap')
_NO_METRIC = "content_distances: the metric is 'jaccard' or 'overlap'"
_ROW_STEP = 1 << 16   # rows per float64 product: every partial count is an integer far below 2^53, so the sums are exact


def _weighted_shared(counts, weight=None):
    x = np.asarray(counts)
    if x.ndim != 2:
        raise ValueError('shared_counts: the count table has two dimensions')
    R, T = x.shape
    S = np.zeros((T, T), dtype=np.int64)
    for r0 in range(0, R, _ROW_STEP):
        P = (x[r0:r0 + _ROW_STEP] > 0).astype(np.float64)
        S += np.rint(P.T @ (P if weight is None else P * weight[r0:r0 + _ROW_STEP, None])).astype(np.int64)
    return S


def shared_counts(counts):
    """-> int64[T, T]: S[a, b] = the rows (file rows and the one-gene rows behind them) present in both a and b, presence = count > 0 (a
    member listed twice counts once); S[a, a] = the families of genome a.  S = P^T P in float64, exact"""
    return _weighted_shared(counts)


def boot_shared(counts, seed, b):
    """-> int64[T, T] of replicate b: shared_counts over the rows phy.boot_columns(seed, b, n_rows) -- a row drawn twice counts twice
    (the order of the draws does not matter: S = P^T diag(times drawn) P)"""
    from . import phy
    R = len(np.asarray(counts))
    return _weighted_shared(counts, np.bincount(phy.boot_columns(seed, b, R), minlength=R).astype(np.float64))


def _content(S, metric):
    """-> (D, argwhere of the zero denominators): the diagonal's denominator counts -- a genome without a family has no distance at all"""
    if metric not in METRICS:
        raise ValueError(_NO_METRIC)
    S = np.asarray(S, dtype=np.int64)
    if S.ndim != 2 or S.shape[0] != S.shape[1]:
        raise ValueError('content_distances: S is a square matrix')
    d = np.diagonal(S)
    den = (d[:, None] + d[None, :] - S) if metric == 'jaccard' else np.minimum(d[:, None], d[None, :])
    with np.errstate(divide='ignore', invalid='ignore'):
        D = 1. - S.astype(np.float64) / den.astype(np.float64)
    np.fill_diagonal(D, 0.)
    return D, np.argwhere(den == 0)


def content_distances(S, metric='jaccard', names=None):
    """-> float64[T, T] from the exact integers: jaccard 1 - S_ab / (S_aa + S_bb - S_ab); overlap 1 - S_ab / min(S_aa, S_bb), the
    gene-content distance of Snel et al. 1999; the diagonal is 0.  A pair whose denominator is 0 -- under jaccard two genomes without a
    family, under overlap one; a genome without a family has none to itself either -- raises phy.DistanceRefused"""
    from . import phy
    D, bad = _content(S, metric)
    if len(bad):
        off = bad[bad[:, 0] != bad[:, 1]]      # the first pair of two taxa; under jaccard a lone empty genome has only itself: any other names the pair
        a, b = (int(off[0][0]), int(off[0][1])) if len(off) else (int(bad[0][0]), 0 if bad[0][0] or len(D) == 1 else 1)
        who = lambda k: phy._label(names[k]) if names is not None else str(k)
        raise phy.DistanceRefused('content_distances: taxa %s and %s have no %s distance: its denominator is 0 (a genome without a family)' % (who(a), who(b), metric))
    return D


def boot_content_distances(S, metric='jaccard'):
    """-> (D float64[T, T], ok): content_distances() without its refusal.  ok is False where a denominator is 0: such a replicate is
    dropped, not refused (its D holds NaN or inf there; the diagonal is 0 all the same)"""
    D, bad = _content(S, metric)
    return D, not len(bad)


def _device_shared(who, row, taxon, n_rows, n_taxa, seed, b0, nb, device, stats=None, want=True, timed=False):
    """so_pan_shared -> int32[max(nb, 1), T, T] (None without `want`); nb = 0: all rows"""
    from . import _lib
    row32, tax32 = np.ascontiguousarray(row, dtype=np.int32), np.ascontiguousarray(taxon, dtype=np.int32)
    if len(row32) != len(tax32):
        raise ValueError('%s: row and taxon differ in length' % who)
    flags = (0 if want else 1) | (2 if timed else 0)
    with _lib.call('so_pan_shared', _lib.SoPanSharedResult, 'so_pan_shared_free', 'so_pan_last_error', int(device), len(row32), row32, tax32, int(n_rows), int(n_taxa),
                   int(seed) & (2 ** 64 - 1), int(b0), int(nb), flags) as res:
        if stats is not None:
            stats['waits'], stats['batches'], stats['ranges'], stats['bytes'] = int(res.waits), int(res.batches), int(res.ranges), int(res.bytes)
            if timed:
                stats['draw_ms'], stats['product_ms'] = float(res.draw_ms), float(res.product_ms)
        n, T = int(res.n_reps), int(n_taxa)
        return _lib.result_array(res.shared, n * T * T, np.int32).reshape(n, T, T) if want else None


def device_shared_counts(row, taxon, n_rows, n_taxa, device=0, stats=None):
    """shared_counts(count_matrix(row, taxon, n_rows, n_taxa)) in one device call (so_pan_shared), never through the count table ->
    int64[T, T]; a refusal raises RuntimeError with the library's message"""
    return _device_shared('device_shared_counts', row, taxon, n_rows, n_taxa, 0, 0, 0, device, stats)[0].astype(np.int64)


def device_boot_shared(row, taxon, n_rows, n_taxa, seed, b0, nb, device=0, stats=None):
    """boot_shared() of replicates b0 .. b0 + nb - 1 in one device call (so_pan_shared) -> int64[nb, T, T]"""
    if int(nb) < 1:
        raise ValueError('device_boot_shared: a replicate at least')
    return _device_shared('device_boot_shared', row, taxon, n_rows, n_taxa, seed, b0, nb, device, stats).astype(np.int64)


class TooFewTaxa(ValueError):
    """fewer than two taxa: no pair, no tree (pan_genome.py exits with code 2)"""


def content_tree(table, taxa, metric='jaccard', boot=0, seed=1, device_stage=False, device=0, stats=None):
    """MemberTable + the names of its taxon codes -> (Newick bytes, S int64[T, T], D float64[T, T]): the neighbour-joining tree
    (phy.neighbor_joining) of the gene-content distances.  Tree, S and D list the taxa in SORTED order of their names, whatever order the
    table codes them in.  boot > 0: every node a join makes carries the share of the valid bootstrap replicates that hold its split, as
    phy.tree labels them: replicate b draws the rows with replacement (boot_shared), a replicate with a zero denominator is dropped
    (boot_content_distances), the others give a topology (phy.nj_splits); no valid replicate: ValueError.  device_stage: S and the
    replicates' matrices by so_pan_shared, the replicates' trees by so_phy_nj_splits (no fallback); the distances divide exact integers
    on the host either way, so the bytes are the same.  stats: 'boot', 'boot_valid', 'calls' (device calls of the bootstrap)"""
    from . import phy
    if metric not in METRICS:
        raise ValueError(_NO_METRIC)
    boot, seed, T = int(boot), int(seed), len(taxa)
    if not 0 <= boot < 2 ** 31:
        raise ValueError('content_tree: boot lies in 0 .. 2^31 - 1')
    if T < 2:
        raise TooFewTaxa('content_tree: the gene-content tree and table need two taxa at least (there %s)' % ('is 1' if T == 1 else 'are none'))
    order = sorted(range(T), key=lambda k: taxa[k])
    names = [taxa[k] for k in order]
    rank = np.zeros(T, dtype=np.int32)
    rank[order] = np.arange(T, dtype=np.int32)
    tax = rank[np.asarray(table.taxon, dtype=np.int64)] if len(table.taxon) else np.zeros(0, dtype=np.int32)
    R = table.n_rows
    try:
        if device_stage:
            counts, S = None, device_shared_counts(table.row, tax, R, T, device)
        else:
            counts = count_matrix(table.row, tax, R, T)
            S = shared_counts(counts)
        D = content_distances(S, metric, names)
        if boot <= 0:
            return phy.neighbor_joining(D, names), S, D
        if R == 0:
            raise ValueError('content_tree: no row to draw from')
        ref = phy.tree_splits(D)
        ns, W = max(T - 3, 0), (T + 63) // 64
        if device_stage:   # a batch: what about 2^30 bytes of counts (int32 and int64) and distances hold
            step = phy.batch_size(boot, 20 * T * T)
            counts_of = lambda b0, nb: (device_boot_shared(table.row, tax, R, T, seed, b0, nb, device), 1)
            trees_of = lambda Ds, idx: phy.device_nj_splits(Ds, device)
        else:
            step = 1
            counts_of = lambda b, _: ([boot_shared(counts, seed, b)], 0)
            trees_of = lambda Ds, idx: phy.nj_splits(Ds[0])[None]
        ok, splits, calls = phy.replicate_trees(boot, step, counts_of, lambda Sb, k: boot_content_distances(Sb[k], metric), trees_of, ns, W)
        if stats is not None and device_stage:
            stats['calls'] = calls
    except RuntimeError as e:
        raise ValueError('content_tree: %s' % e)
    valid = int(ok.sum())
    if valid == 0:
        raise ValueError('content_tree: none of the %d replicates gives every pair of taxa a distance' % boot)
    if stats is not None:
        stats['boot'], stats['boot_valid'] = boot, valid
    return phy.neighbor_joining(D, names, phy.split_support(ref, splits, ok) / float(valid)), S, D


def content_table_text(names, S, D):
    """-> the text of the -d file: per pair a < b of the sorted taxa `taxon_a taxon_b families_a families_b shared distance`, tab-separated,
    the distance as repr(float)"""
    S, D = np.asarray(S).tolist(), np.asarray(D).tolist()
    out = []
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            out.append('%s\t%s\t%d\t%d\t%d\t%s\n' % (names[a], names[b], S[a][a], S[b][b], S[a][b], repr(float(D[a][b]))))
    return ''.join(out)


# ---------------------------------------------------------------------------------------------------------
# text
# ---------------------------------------------------------------------------------------------------------
def xy_text(core, spec, panz):
    """-> the text of <groups file>_xy.txt: per j = 2 .. N the orders one after the other"""
    core, spec, panz = np.asarray(core), np.asarray(spec), np.asarray(panz)
    size, steps = core.shape
    out = []
    for i in range(steps):
        for p in range(size):
            out.append('%d\t%d\t%d\t%d\n' % (i + 2, core[p, i], spec[p, i], panz[p, i]))
    return ''.join(out)


def number_line(totals, n_rows, n_file_rows, n_taxa):
    """the `# Number` line: the rows behind the file rows count as specific"""
    core, shar, spec = totals
    return '\t'.join(map(str, ['# Number', core, shar, spec + (n_rows - n_file_rows), n_taxa]))


def table_lines(taxa, types, counts):
    """the header line and one line per row of the family table"""
    out = ['\t'.join(['#family', 'type'] + list(taxa))]
    for k, (t, c) in enumerate(zip(np.asarray(types).tolist(), np.asarray(counts).tolist())):
        out.append('group_%09d\t%s' % (k, TYPE_NAMES[t]) + '\t' + '\t'.join(map(str, c)))
    return out


def report_lines(taxa, res, n_file_rows, xy_name):
    """what the script prints, the three fit blocks replaced by one line"""
    n_rows = len(res.types)
    return ['#' * 80, '# Statistics and profile of pan-genome:',
            '# The methods can be found in Hu X, et al. Trajectory and genomic determinants of fungal-pathogen speciation and host adaptation.',
            '#', '# statistic of core, shared and specific genes:', '\t'.join(['# Feature', 'core', 'shared', 'specific', 'taxon']),
            number_line(res.totals, n_rows, n_file_rows, len(taxa)), '#',
            '# the curve fits of core size, new genes and pan-genome size are not computed here: %s holds their whole input' % xy_name,
            '#', '# Type and frequency of each gene group in different species:', '#' * 80] + table_lines(taxa, res.types, res.counts)


# ---------------------------------------------------------------------------------------------------------
# the script
# ---------------------------------------------------------------------------------------------------------
def manual_print():
    print('Usage:')
    print('  python this_script.py -i foo.pep.fsa -g foo.mcl [-l .05] [-u .95] [-r taxa.txt] [-G T] [-t tree.nwk] [-d pairs.tsv] [-m jaccard|overlap] [-B replicates] [-S seed]')
    print('Parameters:')
    print(' -i: protein/gene fasta file; a header reads taxon|identifier')
    print(' -g: groups file, one protein/gene group per line, tab-separated')
    print(' -l: at most this share (below 1) or number of taxa: a specific family. Default 0.05')
    print(' -u: at least this share (below 1) or number of taxa: a core family. Default 0.95')
    print(' -r: a file of taxon names, one per line: only these take part')
    print(' -G: count table, types and rarefaction on the GPU [T|F]; with -t or -d also the shared-family counts and the bootstrap replicates. Default: F')
    print(' -t: write the gene-content tree of the genomes (neighbour joining, Newick, taxa in sorted order) to this file')
    print(' -d: write one line per pair of genomes to this file: taxon_a taxon_b families_a families_b shared distance (tab-separated, taxa in sorted order)')
    print(' -m: gene-content distance [jaccard|overlap]: 1 - shared / (families_a + families_b - shared), or 1 - shared / min(families_a, families_b). Default: jaccard')
    print(' -B: with -t, label the tree\'s nodes with their bootstrap support over this many replicates of the families. Default: 0 (no labels)')
    print(' -S: seed of the bootstrap\'s draws, 0 .. 2^64 - 1. Default: 1')


def write_content(table, taxa, tree_path='', dist_path='', metric='jaccard', boot=0, seed=1, device_stage=False, device=0, stats=None):
    """content_tree() to files: the tree (Newick and a newline) to `tree_path`, content_table_text() to `dist_path`, each when named;
    nothing is written before both are computed -> (sorted taxa, Newick bytes, S, D)"""
    newick, S, D = content_tree(table, taxa, metric, boot if tree_path else 0, seed, device_stage, device, stats)
    names = sorted(taxa)
    if tree_path:
        with open(tree_path, 'wb') as o:
            o.write(newick + b'\n')
    if dist_path:
        with open(dist_path, 'w') as o:
            o.write(content_table_text(names, S, D))
    return names, newick, S, D


def run(fasta_path, groups_path, ts=.05, tc=.95, allow_path=None, device_stage=False, taxa=None, content=None):
    """the script on two files -> the report lines; writes <groups_path>_xy.txt.  taxa: the column order (None: Python's set order of
    the names, as the script has it).  content: the keywords of write_content() (-t, -d, -m, -B, -S) -- the gene-content tree and table
    are computed before anything is written, so a refusal leaves no half output"""
    allow = read_allow(allow_path)
    with open(fasta_path, 'r') as f:
        fasta = f.read()
    with open(groups_path, 'r') as f:
        groups = f.read()
    if taxa is None:
        taxa = list(set(taxa_of_fasta(fasta, allow)))
    table = member_table(fasta, groups, taxa, allow)
    res = pan_genome(table, len(taxa), ts, tc, device_stage=device_stage)
    if content:
        write_content(table, taxa, device_stage=device_stage, **content)
    xy =groups_path + '_xy.txt'
    with open(xy, 'w') as o:
        o.write(xy_text(res.core, res.spec, res.panz))
    return report_lines(taxa, res, table.n_file_rows, xy)


def main(argv=None):
    from .fsearch import parse_flags
    argv = list(sys.argv if argv is None else argv)
    args = parse_flags(argv, {'-i': '', '-g': '', '-l': .05, '-u': .95, '-r': None, '-G': 'F', '-t': '', '-d': '', '-m': 'jaccard', '-B': '0', '-S': '1'})
    if args['-i'] == '' or args['-g'] == '':
        manual_print()
        raise SystemExit()
    try:
        ts, tc = float(args['-l']), float(args['-u'])
    except ValueError:
        manual_print()
        raise SystemExit()
    gpu = str(args['-G']).upper()[:1] == 'T'
    if args['-t'] == '' and args['-d'] == '' and (args['-B'], args['-S'], args['-m']) == ('0', '1', 'jaccard'):
        lines = run(args['-i'], args['-g'], ts, tc, args['-r'], gpu)
    else:
        from .phy import DistanceRefused
        from .rbh import _count_flag
        boot, seed = _count_flag(args['-B'], 2 ** 31 - 1), _count_flag(args['-S'], 2 ** 64 - 1)
        if boot is None or seed is None:
            sys.stderr.write('pan_genome: -B takes a whole number of replicates from 0 to 2^31 - 1, -S a seed from 0 to 2^64 - 1\n')
            return 2
        if args['-m'] not in METRICS:
            sys.stderr.write('pan_genome: -m names the gene-content distance, jaccard or overlap\n')
            return 2
        if boot > 0 and args['-t'] == '':
            sys.stderr.write('pan_genome: -B labels the tree that -t writes: name a tree file with -t\n')
            return 2
        content = dict(tree_path=args['-t'], dist_path=args['-d'], metric=args['-m'], boot=boot, seed=seed) if args['-t'] or args['-d'] else None
        try:
            lines = run(args['-i'], args['-g'], ts, tc, args['-r'], gpu, content=content)
        except (DistanceRefused, TooFewTaxa) as e:
            sys.stderr.write('pan_genome: %s\n' % e)
            return 2
    sys.stdout.write(''.join(l + '\n' for l in lines))
    sys.stdout.flush()
    return 0
