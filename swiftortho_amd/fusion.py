"""fusion -- gene-fusion links: the third genomic-context signal for functional linkage next to gene neighbourhood (operon.py) and
co-occurrence (phyletic.py) -- the "Rosetta stone" method of Marcotte et al. 1999 and Enright et al. 1999.  Two proteins A and B that are
not homologous to each other but align to different, non-overlapping parts of one composite protein C very probably work together.
It needs nothing beyond the hit table of the all-vs-all search: the query interval of every row (qst, qed), the subject span (sst, sed,
slen) and the table itself as the homology relation.

The reference has no such script: the numpy function here is the definition, and the device calls (device_fusion_links,
device_fusion_links_from_records: include/sohit.h so_fusion_*, csrc/fusion.hip) equal fusion_links() integer for integer.
  * Input: hit rows in file order, name codes q, s (find_orth.HitColumns / rbh), qst, qed, sst, sed (1-based, inclusive, as printed),
    slen, and tax[n_names] (rbh.name_taxa).  A RUN is a maximal stretch of consecutive rows of one query code, as in rbh.py; a query
    whose rows come in two runs is treated run by run.
  * Parameters: max_overlap >= 0 (0); the subject coverage num / den (7 / 10), an exact fraction with 0 <= num <= den < 2^20;
    same_taxon (on).
  * A row is ELIGIBLE iff s != q, (sed - sst + 1) * den >= num * slen (equality passes) and, with same_taxon, tax[s] != tax[q].
  * The REPRESENTATIVE of a run and a subject is the first eligible row of that subject in the run.
  * x and y are HOMOLOGOUS iff any row of the table, eligible or not and in any run, holds (q, s) == (x, y) or (y, x).
  * A LINK is a pair of representatives ra < rb of one run, a = s[ra], b = s[rb], with min(qed[ra], qed[rb]) - max(qst[ra], qst[rb]) + 1
    <= max_overlap, with same_taxon tax[a] == tax[b], and a, b not homologous.
  * Result (Links): row_a[], row_b[] ascending by (row_a, row_b) and the counters n_runs, n_eligible, n_reps, n_pairs (the sum over the
    runs of m (m - 1) / 2 for m representatives), n_disjoint (the pairs that passed the interval and the taxon test).
support() of an unordered pair {a, b} is the number of distinct composites linking it; it and the text are host work behind either path,
so `-G T` and `-G F` write the same bytes.
"""
import fractions
import sys

import numpy as np

DEN_LIMIT = 1 << 20       # num <= den < 2^20: with spans and lengths below 2^31 both sides of the coverage test stay below 2^51
_I32_MAX = 2 ** 31 - 1
_PAIR_STEP = 1 << 22      # pairs expanded at a time by the numpy definition
HEADER = '#composite\tgene_a\tgene_b\tqst_a\tqed_a\tqst_b\tqed_b\tqlen\tsupport'
COUNTERS = ('n_runs', 'n_eligible', 'n_reps', 'n_pairs', 'n_disjoint')


class Refused(ValueError):
    """input or a flag value the stage does not take (fusion_links.py exits with code 2)"""


class Table:
    """the columns the stage reads, int64 each, rows in file order; `names`: every distinct id (bytes, ascending), indexed by q and s;
    has_slen: every row carried columns 13 and 14 (else slen and qlen are 0 and only a coverage of 0 is served)"""

    def __init__(self, names, q, s, qst, qed, sst, sed, slen, qlen, has_slen=True):
        self.names, self.q, self.s, self.qst, self.qed, self.sst, self.sed, self.slen, self.qlen = names, q, s, qst, qed, sst, sed, slen, qlen
        self.has_slen = has_slen

    def __len__(self):
        return len(self.q)


class Links:
    """`row_a`, `row_b` (int32, ascending by (row_a, row_b)); `link` int64[n, 8]: q, a, b, qst_a, qed_a, qst_b, qed_b, qlen per link;
    the counters of COUNTERS"""

    def __init__(self, row_a, row_b, link, n_runs, n_eligible, n_reps, n_pairs, n_disjoint):
        self.row_a, self.row_b, self.link = row_a, row_b, link
        self.n_runs, self.n_eligible, self.n_reps, self.n_pairs, self.n_disjoint = int(n_runs), int(n_eligible), int(n_reps), int(n_pairs), int(n_disjoint)

    def __len__(self):
        return len(self.row_a)

    def counters(self):
        return {k: getattr(self, k) for k in COUNTERS}


# ---------------------------------------------------------------------------------------------------------
# the definition (numpy) the device calls are held to
# ---------------------------------------------------------------------------------------------------------
def check_parameters(max_overlap, num, den):
    """what the device call refuses of the parameters, as Refused"""
    if not 0 <= int(max_overlap) <= _I32_MAX:
        raise Refused('fusion_links: max_overlap lies in 0 .. 2^31 - 1 (it is %d)' % int(max_overlap))
    if not (0 <= int(num) <= int(den) < DEN_LIMIT and int(den) >= 1):
        raise Refused('fusion_links: the subject coverage num / den needs 0 <= num <= den < 2^20, den above 0 (they are %d and %d)' % (int(num), int(den)))


def check_rows(t, n_names, tax, n_taxa=None):
    """what the device call refuses of the rows, as Refused"""
    bad = (t.qst < 1) | (t.qed < t.qst) | (t.sst < 1) | (t.sed < t.sst) | (t.slen < 0)
    if bad.any():
        raise Refused('fusion_links: a row with qst < 1, qed < qst, sst < 1, sed < sst or slen < 0 (row %d)' % int(np.flatnonzero(bad)[0]))
    if len(t) and (min(t.q.min(), t.s.min()) < 0 or max(t.q.max(), t.s.max()) >= n_names):
        raise Refused('fusion_links: a name code lies outside 0 .. n_names - 1')
    if n_taxa is not None and len(tax) and (tax.min() < 0 or tax.max() >= n_taxa):
        raise Refused('fusion_links: a name has a taxon outside 0 .. n_taxa - 1')


def _as_table(t):
    f = lambda a: np.asarray(a, dtype=np.int64)
    return Table(t.names, f(t.q), f(t.s), f(t.qst), f(t.qed), f(t.sst), f(t.sed), f(t.slen), f(t.qlen), t.has_slen)


def link_columns(t, row_a, row_b):
    """-> int64[n, 8]: q, a, b, qst_a, qed_a, qst_b, qed_b, qlen of every link, from the table's columns"""
    ra, rb = np.asarray(row_a, dtype=np.int64), np.asarray(row_b, dtype=np.int64)
    f = lambda c, r: np.asarray(c, dtype=np.int64)[r]
    return np.stack([f(t.q, ra), f(t.s, ra), f(t.s, rb), f(t.qst, ra), f(t.qed, ra), f(t.qst, rb), f(t.qed, rb), f(t.qlen, ra)], axis=1).reshape(len(ra), 8)


def fusion_links(table, tax, max_overlap=0, num=7, den=10, same_taxon=True):
    """THE DEFINITION -> Links.  Every run's pairs of representatives are expanded, _PAIR_STEP at a time"""
    from .rbh import _runs
    check_parameters(max_overlap, num, den)
    t = _as_table(table)
    tax = np.asarray(tax, dtype=np.int64)
    M = max(len(tax), 1)
    check_rows(t, len(tax), tax)
    n = len(t)
    empty = np.zeros(0, dtype=np.int32)
    if n == 0:
        return Links(empty, empty, np.zeros((0, 8), dtype=np.int64), 0, 0, 0, 0, 0)
    run = _runs(t.q)
    n_runs = int(run[-1]) + 1
    elig = (t.s != t.q) & ((t.sed - t.sst + 1) * int(den) >= int(num) * t.slen)
    if same_taxon:
        elig &= tax[t.s] != tax[t.q]
    erows = np.flatnonzero(elig)
    # representatives: the first eligible row of every (run, subject); np.unique names the first occurrence
    reps = np.sort(erows[np.unique(run[erows] * M + t.s[erows], return_index=True)[1]])
    rrun = run[reps]
    first = np.searchsorted(rrun, rrun, side='left')          # the slot of the run's first representative
    local = np.arange(len(reps)) - first                      # representatives of the run before this one
    n_pairs = int(local.sum())                                # (below 2^61: fewer than 2^31 rows)
    homolog = np.unique(t.q * M + t.s)
    has = lambda k: homolog[np.minimum(np.searchsorted(homolog, k), len(homolog) - 1)] == k
    out, n_disjoint = [], 0
    cum = np.concatenate([[0], np.cumsum(local)])
    j0 = 0
    while j0 < len(reps):                                     # slots j0 .. j1 - 1 as the later member, all their earlier ones
        j1 = int(np.searchsorted(cum, cum[j0] + _PAIR_STEP, side='right'))
        j1 = max(j1 - 1, j0 + 1)
        cnt = local[j0:j1]
        jb = np.repeat(np.arange(j0, j1), cnt)
        ia = first[jb] + (np.arange(int(cnt.sum())) - np.repeat(cum[j0:j1] - cum[j0], cnt))
        ra, rb = reps[ia], reps[jb]
        ok = np.minimum(t.qed[ra], t.qed[rb]) - np.maximum(t.qst[ra], t.qst[rb]) + 1 <= int(max_overlap)
        a, b = t.s[ra], t.s[rb]
        if same_taxon:
            ok &= tax[a] == tax[b]
        n_disjoint += int(ok.sum())
        ra, rb, a, b = ra[ok], rb[ok], a[ok], b[ok]
        ok = ~(has(a * M + b) | has(b * M + a))
        out.append((ra[ok] << 32) | rb[ok])
        j0 = j1
    key = np.sort(np.concatenate(out)) if out else np.zeros(0, dtype=np.int64)
    row_a, row_b = (key >> 32).astype(np.int32), (key & 0xFFFFFFFF).astype(np.int32)
    return Links(row_a, row_b, link_columns(t, row_a, row_b), n_runs, len(erows), len(reps), n_pairs, n_disjoint)


def literal_links(table, tax, max_overlap=0, num=7, den=10, same_taxon=True, deviate=None):
    """the definition once more, as a Python loop over dicts and sets -> (sorted list of (row_a, row_b), dict of the counters).
    deviate names ONE departure, for the tests that show a designed input catches it: 'overlap' (the bound off by one), 'one_way'
    (homology looked up as (a, b) only), 'last' (the last eligible row of a subject stands for it), 'first_row' (the first row of a
    subject stands for it, eligible or not)"""
    col = lambda a: np.asarray(a).tolist()
    q, s, qst, qed, sst, sed, slen = (col(getattr(table, k)) for k in ('q', 's', 'qst', 'qed', 'sst', 'sed', 'slen'))
    tx = col(tax)
    n = len(q)
    homolog = set(zip(q, s))
    links, c = [], dict.fromkeys(COUNTERS, 0)
    i = 0
    while i < n:
        j = i
        while j < n and q[j] == q[i]:
            j += 1
        c['n_runs'] += 1
        rep = {}                                   # subject -> its representative row, in order of first entry
        for r in range(i, j):
            ok = s[r] != q[r] and (sed[r] - sst[r] + 1) * den >= num * slen[r] and (not same_taxon or tx[s[r]] != tx[q[r]])
            c['n_eligible'] += ok
            if deviate == 'first_row':
                if s[r] not in rep:
                    rep[s[r]] = r if ok else None
            elif ok and (s[r] not in rep or deviate == 'last'):
                rep[s[r]] = r
        rows = sorted(r for r in rep.values() if r is not None)
        c['n_reps'] += len(rows)
        c['n_pairs'] += len(rows) * (len(rows) - 1) // 2
        for x, ra in enumerate(rows):
            for rb in rows[x + 1:]:
                a, b = s[ra], s[rb]
                over = min(qed[ra], qed[rb]) - max(qst[ra], qst[rb]) + 1
                if over > max_overlap + (1 if deviate == 'overlap' else 0) or (same_taxon and tx[a] != tx[b]):
                    continue
                c['n_disjoint'] += 1
                if (a, b) in homolog or ((b, a) in homolog and deviate != 'one_way'):
                    continue
                links.append((ra, rb))
        i = j
    return sorted(links), c


def support(links):
    """-> int64[n]: per link the number of distinct composites that link its unordered pair {a, b}"""
    L = np.asarray(links.link, dtype=np.int64).reshape(-1, 8)
    if len(L) == 0:
        return np.zeros(0, dtype=np.int64)
    lo, hi = np.minimum(L[:, 1], L[:, 2]), np.maximum(L[:, 1], L[:, 2])
    trip = np.unique(np.stack([lo, hi, L[:, 0]], axis=1), axis=0)          # distinct (pair, composite)
    pairs, count = np.unique(trip[:, :2], axis=0, return_counts=True)
    where = {(x, y): k for (x, y), k in zip(pairs.tolist(), count.tolist())}
    return np.asarray([where[p] for p in zip(lo.tolist(), hi.tolist())], dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------
# the stage on the GPU (include/sohit.h so_fusion_*, csrc/fusion.hip).  No fallback: without the library or a device these raise.
# ---------------------------------------------------------------------------------------------------------
def _flags(same_taxon, timed):
    return (1 if same_taxon else 0) | (2 if timed else 0)


def _links_of(res, stats, timed):
    from . import _lib
    if stats is not None:
        stats['waits'] = int(res.waits)
        if timed:
            for k in ('prep_ms', 'keys_ms', 'count_ms', 'count_again_ms', 'emit_ms', 'sort_ms'):
                stats[k] = float(getattr(res, k))
    arr, n = _lib.result_array, int(res.n_links)
    return Links(arr(res.row_a, n, np.int32), arr(res.row_b, n, np.int32), arr(res.link, 8 * n, np.int64).reshape(n, 8),
                 res.n_runs, res.n_eligible, res.n_reps, res.n_pairs, res.n_disjoint)


def _int32(who, a):
    a64 = np.asarray(a, dtype=np.int64)
    if len(a64) and (a64.min() < -2 ** 31 or a64.max() > _I32_MAX):
        raise RuntimeError('%s: a value does not fit 32 bits' % who)
    return np.ascontiguousarray(a64, dtype=np.int32)


def device_fusion_links(table, tax, max_overlap=0, num=7, den=10, same_taxon=True, n_taxa=None, device=0, stats=None, timed=False):
    """fusion_links() in one device call on host columns (so_fusion_cols) -> Links; a refusal raises RuntimeError with the library's message"""
    from . import _lib
    who = 'so_fusion_cols'
    if len(table) >= 1 << 31:
        raise RuntimeError('%s: 2^31 rows and more are not supported' % who)
    cols = [_int32(who, getattr(table, k)) for k in ('q', 's', 'qst', 'qed', 'sst', 'sed', 'slen', 'qlen')]
    tax32 = _int32(who, tax)
    nt = int(tax32.max()) + 1 if n_taxa is None and len(tax32) else int(n_taxa or 0)
    with _lib.call(who, _lib.SoFusionResult, 'so_fusion_free', 'so_fusion_last_error', int(device), len(table), *cols, len(tax32), tax32, nt, int(max_overlap),
                   int(num), int(den), _flags(same_taxon, timed)) as res:
        return _links_of(res, stats, timed)


def device_fusion_links_from_records(dev, query_ids, subject_ids, max_overlap=0, num=7, den=10, same_taxon=True, sep='|', stats=None, timed=False):
    """fusion_links() of the records `dev` holds -- a fsearch.DeviceHits, an nr.ExpandedHits or a CUDA uint8 torch tensor of so_hit records
    -- without the download (so_fusion_records) -> (names, Links)"""
    import ctypes as C
    from . import _lib, find_orth, rbh
    d_ptr, n, device, keep = find_orth.records_on_device(dev, 'fusion')
    names, qmap, smap = find_orth._record_maps(query_ids, subject_ids)
    tax, taxa = rbh.name_taxa(names, sep)
    tax32 = np.ascontiguousarray(tax, dtype=np.int32)
    with _lib.call('so_fusion_records', _lib.SoFusionResult, 'so_fusion_free', 'so_fusion_last_error', int(device), C.c_void_p(d_ptr), n, qmap, len(qmap), smap, len(smap),
                   len(names), tax32, len(taxa), int(max_overlap), int(num), int(den), _flags(same_taxon, timed)) as res:
        links = _links_of(res, stats, timed)
    del keep
    return names, links


# ---------------------------------------------------------------------------------------------------------
# text
# ---------------------------------------------------------------------------------------------------------
def _whole(field):
    """a field of the table -> its whole number in int32 range, or Refused"""
    f = field.strip()
    d = f[1:] if f[:1] in (b'-', b'+') else f
    if not (d.isdigit() and len(d) <= 10) or not -2 ** 31 <= int(f) <= _I32_MAX:
        raise Refused('a field that is not a whole number in int32 range: %r' % field.decode('latin-1'))
    return int(f)


def read_table(data):
    """tab-separated rows (bytes of a 12-column blast -m8 or 16-column find_hit file) -> Table: columns 1, 2 (ids), 7 .. 10 and, where every
    row has them, 13 and 14 (qlen, slen).  The module's own reader: find_orth.HitColumns carries neither the subject span nor slen"""
    from .find_orth import _codes
    data = data.replace(b'\r\n', b'\n').replace(b'\r', b'\n')
    qn, sn, num = [], [], [[] for _ in range(6)]
    wide = True
    for k, line in enumerate(data.split(b'\n')):
        if not line:
            continue
        f = line.split(b'\t')
        if len(f) < 12:
            raise Refused('line %d has %d columns: a hit table has 12 at least' % (k + 1, len(f)))
        qn.append(f[0]), sn.append(f[1])
        for c, j in enumerate((6, 7, 8, 9)):
            num[c].append(_whole(f[j]))
        if len(f) >= 14:
            num[4].append(_whole(f[13])), num[5].append(_whole(f[12]))
        else:
            wide = False
            num[4].append(0), num[5].append(0)
    arr = lambda v: np.asarray(v, dtype=np.int64)
    if not qn:
        z = np.zeros(0, dtype=np.int64)
        return Table(np.zeros(0, dtype='S1'), z, z, z, z, z, z, z, z, True)
    names, q, s = _codes(np.asarray(qn, dtype=np.bytes_), np.asarray(sn, dtype=np.bytes_))
    slen, qlen = (arr(num[4]), arr(num[5])) if wide else (np.zeros(len(q), dtype=np.int64),) * 2
    return Table(names, q, s, arr(num[0]), arr(num[1]), arr(num[2]), arr(num[3]), slen, qlen, wide)


def _lines(names, links):
    nm = [x.decode('utf-8', 'replace') for x in np.asarray(names).tolist()]
    return nm, np.asarray(links.link, dtype=np.int64).reshape(-1, 8).tolist(), support(links).tolist()


def links_text(names, links):
    """-> the text of standard output: the header, then per link in (row_a, row_b) order `composite gene_a gene_b qst_a qed_a qst_b qed_b
    qlen support`, tab-separated"""
    nm, rows, sup = _lines(names, links)
    out = [HEADER + '\n']
    for (c, a, b, qa0, qa1, qb0, qb1, ql), k in zip(rows, sup):
        out.append('%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\n' % (nm[c], nm[a], nm[b], qa0, qa1, qb0, qb1, ql, k))
    return ''.join(out)


def xyz_text(names, links):
    """-> the text of the -x file: `gene_a gene_b support` per unordered pair, in the pair's name order (name codes ascend with the ids):
    the three columns find_cluster reads"""
    nm, rows, sup = _lines(names, links)
    pairs = sorted({(min(r[1], r[2]), max(r[1], r[2]), k) for r, k in zip(rows, sup)})
    return ''.join('%s\t%s\t%d\n' % (nm[a], nm[b], k) for a, b, k in pairs)


# ---------------------------------------------------------------------------------------------------------
# the script
# ---------------------------------------------------------------------------------------------------------
def coverage_fraction(text):
    """the -c value -> (num, den), exactly: '0.7', '7/10' and '1' are all read by fractions.Fraction"""
    try:
        f = fractions.Fraction(str(text).strip())
    except (ValueError, ZeroDivisionError):
        raise Refused('-c takes a subject coverage from 0 to 1, as a decimal or a fraction (it is %r)' % (text,))
    if not 0 <= f <= 1:
        raise Refused('-c takes a subject coverage from 0 to 1 (it is %s)' % f)
    if f.denominator >= DEN_LIMIT:
        raise Refused('-c as a fraction in lowest terms has a denominator below 2^20 (it is %s)' % f)
    return f.numerator, f.denominator


def overlap_value(text):
    t = str(text).strip()
    if not (t.isdigit() and t.isascii() and int(t) <= _I32_MAX):
        raise Refused('-o takes a whole number of residues from 0 to 2^31 - 1 (it is %r)' % (text,))
    return int(t)


def truth_value(flag, text):
    t = str(text).strip().upper()
    if t not in ('T', 'F'):
        raise Refused('%s takes T or F (it is %r)' % (flag, text))
    return t == 'T'


def table_links(table, coverage='0.7', max_overlap=0, same_taxon=True, sep='|', device_stage=False, device=0, stats=None):
    """Table -> Links by fusion_links() or (device_stage) by the device call: what the script and the wrapper call"""
    from .rbh import name_taxa
    num, den = coverage_fraction(coverage)
    max_overlap = overlap_value(max_overlap)
    if not table.has_slen and num != 0:
        raise Refused('the table has 12-column rows, which carry no subject length: the coverage test needs columns 13 and 14 (only -c 0 is served)')
    tax, taxa = name_taxa(table.names, sep)
    if device_stage:
        return device_fusion_links(table, tax, max_overlap, num, den, same_taxon, len(taxa), device, stats)
    return fusion_links(table, tax, max_overlap, num, den, same_taxon)


def run(sc_path, coverage='0.7', max_overlap=0, same_taxon=True, device_stage=False, device=0, stats=None):
    """the script on a hit table -> (Table, Links)"""
    with open(sc_path, 'rb') as f:
        table = read_table(f.read())
    return table, table_links(table, coverage, max_overlap, same_taxon, '|', device_stage, device, stats)


def manual_print():
    print('Pairs of proteins that align side by side on one composite protein and are not homologous to each other (gene fusion, "Rosetta stone")')
    print('Usage:')
    print('  python this_script.py -i foo.sc [-c 0.7] [-o 0] [-s T|F] [-x foo.fusion.xyz] [-G T] > foo.fusion.tsv')
    print('Parameters:')
    print(' -i: the hit table of an all-vs-all search: bin/find_hit.py .sc file (16 columns), or blast -m8 (12 columns, with -c 0 only)')
    print(' -c: share of a component its alignment covers at least, from 0 to 1, a decimal or a fraction (7/10). Default: 0.7')
    print(' -o: residues the two alignments may share on the composite. Default: 0')
    print(' -s: the two components are of one taxon, which is not the composite\'s [T|F]. Default: T')
    print(' -x: also write `gene_a gene_b support` per pair of components to this file, the input of bin/find_cluster.py')
    print(' -G: the links on the GPU [T|F]. Default: F')


def main(argv=None):
    from .fsearch import parse_flags
    argv = list(sys.argv if argv is None else argv)
    args = parse_flags(argv, {'-i': '', '-c': '0.7', '-o': '0', '-s': 'T', '-x': '', '-G': 'F'})
    if args['-i'] == '':
        manual_print()
        raise SystemExit()
    try:
        coverage_fraction(args['-c'])
        same = truth_value('-s', args['-s'])
        gpu = truth_value('-G', args['-G'])
        table, links = run(args['-i'], args['-c'], overlap_value(args['-o']), same, gpu)
    except (Refused, RuntimeError) as e:           # RuntimeError: a refusal of the device call
        sys.stderr.write('fusion_links: %s\n' % e)
        return 2
    text = links_text(table.names, links)
    if args['-x']:
        with open(args['-x'], 'w') as o:
            o.write(xyz_text(table.names, links))
    sys.stdout.write(text)
    sys.stdout.flush()
    return 0
