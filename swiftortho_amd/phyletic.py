"""phyletic -- phyletic profiles: the gene families that are gained and lost together across the genomes (phylogenetic profiling,
Pellegrini et al. 1999).  The pan-genome stage (swiftortho_amd/pan.py) reads the family-by-taxon presence matrix P per family (types,
curves) and forms P^T P, the families two GENOMES share; this is the product the other way round, P P^T over the FAMILIES, thresholded
to the sparse list of family pairs with near-identical presence patterns -- candidates for one pathway, one mobile element, one complex.

The reference has no such script: the numpy functions here are the definition, and the device call (device_linked_pairs: include/sohit.h
so_phyletic_pairs, csrc/phyletic.hip) equals linked_pairs() integer for integer.
  * Input: a pan.MemberTable (row, taxon, n_rows, n_file_rows) and T taxa, what pan.member_table() builds.
  * present[r] = the distinct taxa of row r (a member listed twice counts once, as in pan.shared_counts).
  * A row is ELIGIBLE iff r < n_file_rows and n_min <= present[r] <= n_max: the one-gene rows behind the file rows never are.  On the
    command line n_min = spec_max + 1 and n_max = core_min - 1 of pan.type_thresholds(-l, -u, T), so the eligible rows are exactly the
    rows pan_genome.py types Share -- core and specific families carry no signal.
  * Two eligible rows a < b with taxon sets A, B: k = |A & B|, u = present[a] + present[b] - k.  The pair is LINKED iff k >= k_min and
    k * den >= num * u, all integers: num / den is the Jaccard threshold (0 < num <= den < 2^20), equality passes, no float decides.
  * Result (Links): a[], b[], shared[] (int32) ordered by (a, b), present[n_rows], n_eligible.
jaccard() divides the exact integers in float64; enrichment() is the upper tail of the hypergeometric distribution, which says whether a
Jaccard of 1 between two families of 2 genomes means less than one between two families of 250.  Both are host arithmetic behind either
path, so `-G T` and `-G F` write the same bytes.
"""
import fractions
import functools
import math
import sys

import numpy as np

DEN_LIMIT = 1 << 20       # num <= den < 2^20: with k, u <= 4096 both sides of the test stay below 2^32
_ROW_STEP = 256           # rows of `a` per float32 product (every count is an integer up to 4096: exact)
HEADER = '#family_a\tfamily_b\ttaxa_a\ttaxa_b\tshared\tjaccard\tp'


class Links:
    """`a`, `b`, `shared` (int32, by (a, b)): the linked pairs of rows and the taxa they share; `present` int32[n_rows]; `n_eligible`"""

    def __init__(self, a, b, shared, present, n_eligible):
        self.a, self.b, self.shared, self.present, self.n_eligible = a, b, shared, present, n_eligible


# ---------------------------------------------------------------------------------------------------------
# the definition (numpy) the device call is held to
# ---------------------------------------------------------------------------------------------------------
def profile_bits(table, T):
    """-> bool[n_rows, T]: taxon t is present in row r"""
    x = np.zeros((int(table.n_rows), int(T)), dtype=bool)
    x[np.asarray(table.row, dtype=np.int64), np.asarray(table.taxon, dtype=np.int64)] = True
    return x


def eligible_rows(present, n_file_rows, n_min, n_max):
    """-> the eligible rows, ascending (int64)"""
    p = np.asarray(present)[:int(n_file_rows)]
    return np.flatnonzero((p >= n_min) & (p <= n_max))


def check_thresholds(n_min, k_min, num, den):
    """what the device call refuses of the thresholds, as ValueError"""
    if int(n_min) < 1:
        raise ValueError('linked_pairs: n_min is at least 1')
    if int(k_min) < 1:
        raise ValueError('linked_pairs: k_min is at least 1')
    if not 0 < int(num) <= int(den) < DEN_LIMIT:
        raise ValueError('linked_pairs: the threshold num / den needs 0 < num <= den < 2^20')


def linked_pairs(table, T, n_min, n_max, k_min, num, den):
    """THE DEFINITION -> Links.  The product runs in blocks of rows (as pan._weighted_shared does), so 3000 rows take about a second"""
    check_thresholds(n_min, k_min, num, den)
    bits = profile_bits(table, T)
    present = bits.sum(1).astype(np.int32)
    el = eligible_rows(present, table.n_file_rows, n_min, n_max)
    P = bits[el].astype(np.float32)
    n = present[el].astype(np.int64)
    col = np.arange(len(el))
    out_a, out_b, out_k = [], [], []
    for a0 in range(0, len(el), _ROW_STEP):
        k = np.rint(P[a0:a0 + _ROW_STEP] @ P.T).astype(np.int64)
        u = n[a0:a0 + _ROW_STEP, None] + n[None, :] - k
        ok = (k >= k_min) & (k * int(den) >= int(num) * u) & (col[None, :] > col[a0:a0 + _ROW_STEP, None])
        x, y = np.nonzero(ok)                      # row-major: by (a, b)
        out_a.append(el[a0 + x]), out_b.append(el[y]), out_k.append(k[x, y])
    cat = lambda parts: (np.concatenate(parts) if parts else np.zeros(0)).astype(np.int32)
    return Links(cat(out_a), cat(out_b), cat(out_k), present, len(el))


def jaccard(present, a, b, shared):
    """-> float64: k / u from the exact integers"""
    present, k = np.asarray(present, dtype=np.int64), np.asarray(shared, dtype=np.int64)
    u = present[np.asarray(a, dtype=np.int64)] + present[np.asarray(b, dtype=np.int64)] - k
    return k.astype(np.float64) / u.astype(np.float64)


@functools.lru_cache(maxsize=8)
def _log_factorials(T):
    return [math.lgamma(i + 1.) for i in range(T + 1)]


@functools.lru_cache(maxsize=None)
def _tail(T, lo, hi, k):
    lg = _log_factorials(T)
    choose = lambda n, r: lg[n] - lg[r] - lg[n - r]
    first = max(k, lo + hi - T)
    if first <= max(0, lo + hi - T):               # the whole support
        return 1.
    logs = [choose(lo, i) + choose(T - lo, hi - i) - choose(T, hi) for i in range(first, lo + 1)]
    if not logs:
        return 0.
    top = max(logs)                                # summed from the largest term: the others as fractions of it
    return min(1., math.exp(top) * math.fsum(math.exp(x - top) for x in logs))


def enrichment(T, na, nb, k):
    """-> P[X >= k], X hypergeometric: of T genomes na hold family a, the nb of family b are drawn, X of them hold a.  float64 from a
    table of math.lgamma; symmetric in (na, nb), cached per distinct (min, max, k); k <= 0 gives 1"""
    T, na, nb, k = int(T), int(na), int(nb), int(k)
    if not (0 <= na <= T and 0 <= nb <= T):
        raise ValueError('enrichment: a family holds 0 .. T genomes')
    return _tail(T, min(na, nb), max(na, nb), k)


# ---------------------------------------------------------------------------------------------------------
# the stage on the GPU (include/sohit.h so_phyletic_pairs, csrc/phyletic.hip).  No fallback: without the library or a device this raises.
# ---------------------------------------------------------------------------------------------------------
def device_linked_pairs(table, T, n_min, n_max, k_min, num, den, device=0, stats=None, want=True, timed=False):
    """linked_pairs() in one device call -> Links (a, b, shared None without `want`); a refusal raises RuntimeError with the library's
    message.  stats: waits, tiles, n_eligible, n_pairs, and with `timed` count_ms, emit_ms, sort_ms"""
    from . import _lib
    row32, tax32 = np.ascontiguousarray(table.row, dtype=np.int32), np.ascontiguousarray(table.taxon, dtype=np.int32)
    if len(row32) != len(tax32):
        raise ValueError('device_linked_pairs: row and taxon differ in length')
    flags = (0 if want else 1) | (2 if timed else 0)
    with _lib.call('so_phyletic_pairs', _lib.SoPhyleticResult, 'so_phyletic_free', 'so_phyletic_last_error', int(device), len(row32), row32, tax32, int(table.n_rows),
                   int(table.n_file_rows), int(T), int(n_min), int(n_max), int(k_min), int(num), int(den), flags) as res:
        if stats is not None:
            stats['waits'], stats['tiles'], stats['n_eligible'], stats['n_pairs'] = int(res.waits), int(res.tiles), int(res.n_eligible), int(res.n_pairs)
            if timed:
                stats['count_ms'], stats['emit_ms'], stats['sort_ms'] = float(res.count_ms), float(res.emit_ms), float(res.sort_ms)
        arr, n = _lib.result_array, int(res.n_pairs)
        pairs = (arr(res.a, n, np.int32), arr(res.b, n, np.int32), arr(res.shared, n, np.int32)) if want else (None, None, None)
        return Links(pairs[0], pairs[1], pairs[2], arr(res.present, int(res.n_rows), np.int32), int(res.n_eligible))


class BadThreshold(ValueError):
    """a -j or -k the stage does not take (phyletic_links.py exits with code 2)"""


def jaccard_fraction(text):
    """the -j value -> (num, den), exactly: '0.8', '4/5' and '1' are all read by fractions.Fraction"""
    try:
        f = fractions.Fraction(str(text).strip())
    except (ValueError, ZeroDivisionError):
        raise BadThreshold('-j takes a Jaccard threshold above 0 and up to 1, as a decimal or a fraction (it is %r)' % (text,))
    if not 0 < f <= 1:
        raise BadThreshold('-j takes a Jaccard threshold above 0 and up to 1 (it is %s)' % f)
    if f.denominator >= DEN_LIMIT:
        raise BadThreshold('-j as a fraction in lowest terms has a denominator below 2^20 (it is %s)' % f)
    return f.numerator, f.denominator


def family_links(table, taxa, ts=.05, tc=.95, jaccard='0.8', k_min=2, device_stage=False, device=0, stats=None):
    """MemberTable + its taxa -> Links of the families typed Share at (ts, tc) whose profiles reach the Jaccard threshold and share k_min
    taxa at least, by linked_pairs() or (device_stage) by the device call: what the script, the wrapper and the pipeline call"""
    from . import pan
    T = len(taxa)
    num, den = jaccard_fraction(jaccard)
    if int(k_min) != k_min or int(k_min) < 1 or int(k_min) > pan._I32_MAX:
        raise BadThreshold('-k takes a whole number of shared genomes, 1 at least (it is %r)' % (k_min,))
    spec_max, core_min = pan.type_thresholds(ts, tc, T)
    n_min, n_max = max(1, min(spec_max, pan._I32_MAX - 1) + 1), core_min - 1       # (a family of no genome links nothing: n_min stays above 0)
    if T < 1:                                      # no genome: no family holds one
        return Links(*(np.zeros(0, dtype=np.int32),) * 3, np.zeros(table.n_rows, dtype=np.int32), 0)
    if device_stage:
        return device_linked_pairs(table, T, n_min, n_max, int(k_min), num, den, device, stats)
    return linked_pairs(table, T, n_min, n_max, int(k_min), num, den)


# ---------------------------------------------------------------------------------------------------------
# text
# ---------------------------------------------------------------------------------------------------------
def _columns(links):
    present = np.asarray(links.present).tolist()
    a, b, k = (np.asarray(x).tolist() for x in (links.a, links.b, links.shared))
    jac = jaccard(links.present, links.a, links.b, links.shared).tolist()
    return a, b, k, present, jac


def links_text(links, T):
    """-> the text of standard output: the header, then per linked pair `family_a family_b taxa_a taxa_b shared jaccard p`, tab-separated,
    the families named as pan.table_lines names them, jaccard and p as repr(float)"""
    a, b, k, present, jac = _columns(links)
    out = [HEADER + '\n']
    for x, y, s, j in zip(a, b, k, jac):
        out.append('group_%09d\tgroup_%09d\t%d\t%d\t%d\t%s\t%s\n' % (x, y, present[x], present[y], s, repr(j), repr(enrichment(T, present[x], present[y], s))))
    return ''.join(out)


def xyz_text(links, T):
    """-> the text of the -x file: `family_a family_b jaccard` per pair, the three columns find_cluster reads"""
    a, b, _, _, jac = _columns(links)
    return ''.join('group_%09d\tgroup_%09d\t%s\n' % (x, y, repr(j)) for x, y, j in zip(a, b, jac))


# ---------------------------------------------------------------------------------------------------------
# the script
# ---------------------------------------------------------------------------------------------------------
def manual_print():
    print('Pairs of gene families that co-occur across the genomes (phyletic profiles)')
    print('Usage:')
    print('  python this_script.py -i foo.pep.fsa -g foo.clsr [-l .05] [-u .95] [-r taxa.txt] [-j 0.8] [-k 2] [-x foo.links.xyz] [-G T] > foo.links.tsv')
    print('Parameters:')
    print(' -i: protein/gene fasta file; a header reads taxon|identifier')
    print(' -g: groups file, one protein/gene family per line, tab-separated')
    print(' -l, -u: as scripts/pan_genome.py: the families it types Share take part. Defaults 0.05, 0.95')
    print(' -r: a file of taxon names, one per line: only these take part')
    print(' -j: Jaccard threshold of a linked pair, above 0 and up to 1, a decimal or a fraction (4/5). Default: 0.8')
    print(' -k: genomes a linked pair shares at least. Default: 2')
    print(' -x: also write `family_a family_b jaccard` per pair to this file, the input of bin/find_cluster.py')
    print(' -G: the family pairs on the GPU [T|F]. Default: F')


def run(fasta_path, groups_path, ts=.05, tc=.95, allow_path=None, jaccard='0.8', k_min=2, device_stage=False, device=0, stats=None):
    """the script on two files -> (Links, T); the taxa in sorted order, so the process repeats (popcounts do not depend on it)"""
    from . import pan
    allow = pan.read_allow(allow_path)
    with open(fasta_path, 'r') as f:
        fasta = f.read()
    with open(groups_path, 'r') as f:
        groups = f.read()
    taxa = sorted(pan.taxa_of_fasta(fasta, allow))
    table = pan.member_table(fasta, groups, taxa, allow)
    return family_links(table, taxa, ts, tc, jaccard, k_min, device_stage, device, stats), len(taxa)


def main(argv=None):
    from .fsearch import parse_flags
    from .rbh import _count_flag
    argv = list(sys.argv if argv is None else argv)
    args = parse_flags(argv, {'-i': '', '-g': '', '-l': .05, '-u': .95, '-r': None, '-j': '0.8', '-k': '2', '-x': '', '-G': 'F'})
    if args['-i'] == '' or args['-g'] == '':
        manual_print()
        raise SystemExit()
    try:
        ts, tc = float(args['-l']), float(args['-u'])
    except ValueError:
        manual_print()
        raise SystemExit()
    try:
        jaccard_fraction(args['-j'])
        k_min = _count_flag(args['-k'], 2 ** 31 - 1)
        if not k_min:
            raise BadThreshold('-k takes a whole number of shared genomes, 1 at least (it is %r)' % (args['-k'],))
        links, T = run(args['-i'], args['-g'], ts, tc, args['-r'], args['-j'], k_min, str(args['-G']).upper()[:1] == 'T')
    except (BadThreshold, RuntimeError) as e:      # RuntimeError: a refusal of the device call
        sys.stderr.write('phyletic_links: %s\n' % e)
        return 2
    text = links_text(links, T)
    if args['-x']:
        with open(args['-x'], 'w') as o:
            o.write(xyz_text(links, T))
    sys.stdout.write(text)
    sys.stdout.flush()
    return 0
