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
    import ctypes as C_
    from . import _lib
    L = _lib.load()
    row32, tax32 = np.ascontiguousarray(row, dtype=np.int32), np.ascontiguousarray(taxon, dtype=np.int32)
    if len(row32) != len(tax32):
        raise ValueError('device_pan_genome: row and taxon differ in length')
    perm32 = np.ascontiguousarray(perm, dtype=np.int32).reshape(-1, n_taxa) if n_taxa else np.zeros((len(perm), 0), dtype=np.int32)
    S32, C32 = np.ascontiguousarray(S, dtype=np.int32), np.ascontiguousarray(C, dtype=np.int32)
    if len(S32) != n_taxa or len(C32) != n_taxa:
        raise ValueError('device_pan_genome: S and C hold one entry per taxon')
    size = len(perm32)
    ptr = lambda a: C_.c_void_p(a.ctypes.data)
    out = _lib.SoPanResult()
    rc = L.so_pan_genome(int(device), len(row32), ptr(row32), ptr(tax32), int(n_rows), int(n_file_rows), int(n_taxa), int(spec_max), int(core_min), size,
                         ptr(perm32), ptr(S32), ptr(C32), 1 if want_counts else 0, int(flags), C_.byref(out))
    if rc != 0:
        raise RuntimeError(L.so_pan_last_error().decode())
    try:
        arr = _lib.result_array
        steps = max(n_taxa - 1, 0)
        curve = lambda p: arr(p, size * steps, np.int64).reshape(size, steps)
        return PanResult(arr(out.counts, n_rows * n_taxa, np.int32).reshape(n_rows, n_taxa) if want_counts else None, arr(out.type, n_rows, np.uint8),
                         (int(out.n_core), int(out.n_share), int(out.n_spec)), curve(out.core), curve(out.spec), curve(out.panz),
                         {'tier': int(out.tier), 'waits': int(out.waits)})
    finally:
        L.so_pan_free(C_.byref(out))


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
    print('  python this_script.py -i foo.pep.fsa -g foo.mcl [-l .05] [-u .95] [-r taxa.txt] [-G T]')
    print('Parameters:')
    print(' -i: protein/gene fasta file; a header reads taxon|identifier')
    print(' -g: groups file, one protein/gene group per line, tab-separated')
    print(' -l: at most this share (below 1) or number of taxa: a specific family. Default 0.05')
    print(' -u: at least this share (below 1) or number of taxa: a core family. Default 0.95')
    print(' -r: a file of taxon names, one per line: only these take part')
    print(' -G: count table, types and rarefaction on the GPU [T|F]. Default: F')


def run(fasta_path, groups_path, ts=.05, tc=.95, allow_path=None, device_stage=False, taxa=None):
    """the script on two files -> the report lines; writes <groups_path>_xy.txt.  taxa: the column order (None: Python's set order of
    the names, as the script has it)"""
    allow = read_allow(allow_path)
    with open(fasta_path, 'r') as f:
        fasta = f.read()
    with open(groups_path, 'r') as f:
        groups = f.read()
    if taxa is None:
        taxa = list(set(taxa_of_fasta(fasta, allow)))
    table = member_table(fasta, groups, taxa, allow)
    res = pan_genome(table, len(taxa), ts, tc, device_stage=device_stage)
    xy = groups_path + '_xy.txt'
    with open(xy, 'w') as o:
        o.write(xy_text(res.core, res.spec, res.panz))
    return report_lines(taxa, res, table.n_file_rows, xy)


def main(argv=None):
    from .fsearch import parse_flags
    argv = list(sys.argv if argv is None else argv)
    args = parse_flags(argv, {'-i': '', '-g': '', '-l': .05, '-u': .95, '-r': None, '-G': 'F'})
    if args['-i'] == '' or args['-g'] == '':
        manual_print()
        raise SystemExit()
    try:
        ts, tc = float(args['-l']), float(args['-u'])
    except ValueError:
        manual_print()
        raise SystemExit()
    lines = run(args['-i'], args['-g'], ts, tc, args['-r'], str(args['-G']).upper()[:1] == 'T')
    sys.stdout.write(''.join(l + '\n' for l in lines))
    sys.stdout.flush()
    return 0
