"""rbh -- counterpart of SwiftOrtho's scripts/get_rbh.py and of the first half of scripts/rbh2phy.py: from the hits of an all-vs-all
search to the reciprocal best hits between taxa and to the core-gene families built from them; same ids, same order.

Like find_orth, the stage is COLUMNAR (nothing here is a transcription of the scripts, which walk the text twice with dictionaries):
it works on find_orth.HitColumns -- from the search's records (columns_from_records) or from a .sc file (columns_from_text) -- and
name codes ascend in the ids' string order, so "the smaller id first" is an integer comparison.

What the scripts define, quirks included (pinned by the goldens: tools/refharness/make_rbh_goldens.py runs the REAL scripts):
  * run: consecutive rows of one query id; taxon: the id up to the first separator (the whole id when it has none);
  * winner: per run and subject taxon other than the query's, the FIRST row holding the largest score (get_rbh.py replaces on strict
    `<`, rbh2phy.py sorts the run stably by -score: the same rule; 0.0 and -0.0 are equal).  Winners are listed by the first row of
    their (run, taxon) group;
  * get_rbh.py: every winner proposes (smaller id, larger id); the pair is printed at every EVEN-numbered proposal of its key, where
    that proposal stands (its add / print-and-remove set): proposed once -> nothing, four times -> twice;
  * rbh2phy.py: the taxa of the FASTA headers, ordered by gene count (descending, ties by first appearance), are the slots; the
    reference taxon R is -r, or slot 0's.  Pass 1 (runs of R's genes): fwd[gene][taxon] = the winner's subject, a later run
    overwriting taxon by taxon; genes enter the table at their first run with a winner.  Pass 2 (runs of other genes): the winner
    among R's genes, if it is in the table and fwd[it][taxon of q] == q, flags that cell.  Assembly: slot 0 of every entry is preset
    to (the gene itself, flagged) WHATEVER slot R has, a forward hit in slot 0's taxon overwrites the id and keeps the flag; a group
    is the flagged ids in slot order, kept when len / number of taxa >= 0.9.  So with -r naming another taxon than the largest, the
    gene is missing from its own group and slot 0's member need not be reciprocal: reproduced, not repaired;
  * a hit taxon that is not in the FASTA makes rbh2phy.py raise KeyError as soon as its table uses it; here core_table() refuses
    (ValueError) whenever the table has a gene at all and some hit taxon is absent from the FASTA;
  * a NaN score is outside the definition (Python's `<` and sort disagree on it): the numpy functions and the device call hand such
    input to the literal host loops below, which walk the rows the way each script does.
"""
import sys

import numpy as np

from . import find_orth


# ---------------------------------------------------------------------------------------------------------
# taxa
# ---------------------------------------------------------------------------------------------------------
def name_taxa(names, sep='|'):
    """taxon code of every name + the distinct taxa (bytes, ascending); an id without the separator is its own taxon"""
    if len(names) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype='S1')
    head = np.char.partition(names, sep.encode('utf-8'))[:, 0]
    taxa, inv = np.unique(head, return_inverse=True)
    return inv.astype(np.int64), taxa


def fasta_taxa(fasta_bytes, sep='|'):
    """the taxa of a FASTA file in slot order: a header is any line that starts with '>', its taxon the line without its first and
    last character up to the first separator; ordered by gene count descending, ties by first appearance (a stable sort)"""
    data = fasta_bytes.replace(b'\r\n', b'\n').replace(b'\r', b'\n')
    count = {}
    sepb = sep.encode('utf-8')
    for line in data.splitlines(True):
        if line.startswith(b'>'):
            t = line[1:-1].split(sepb)[0]
            count[t] = count.get(t, 0) + 1
    return [t for t, _ in sorted(count.items(), key=lambda x: x[1], reverse=True)]


# ---------------------------------------------------------------------------------------------------------
# winners
# ---------------------------------------------------------------------------------------------------------
def _runs(q):
    return np.cumsum(np.concatenate([[0], q[1:] != q[:-1]]).astype(np.int64)) if len(q) else np.zeros(0, dtype=np.int64)


def winners(cols, tax, n_taxa):
    """-> (query codes, subject codes) of the winner list, and the number of runs (numpy; k_rbh_run_wave / k_rbh_seg_max on the GPU)"""
    q, s, sco = np.asarray(cols.q, dtype=np.int64), np.asarray(cols.s, dtype=np.int64), np.asarray(cols.score, dtype=np.float64)
    empty = np.zeros(0, dtype=np.int64)
    if len(q) == 0:
        return empty, empty, 0
    run = _runs(q)
    nrun = int(run[-1]) + 1
    rows = np.flatnonzero(tax[q] != tax[s])
    if len(rows) == 0:
        return empty, empty, nrun
    key = run[rows] * max(n_taxa, 1) + tax[s[rows]]
    # groups ascending by key; inside one the largest score first, equal scores (0.0 and -0.0 too) by row
    order = np.lexsort((rows, -sco[rows], key))
    head = np.flatnonzero(np.concatenate([[True], key[order][1:] != key[order][:-1]]))
    win = rows[order[head]]
    first = rows[np.unique(key, return_index=True)[1]]    # (ascending by key as well)
    o = np.argsort(first, kind='stable')
    return q[win[o]], s[win[o]], nrun


def _literal_winners(cols, tax, by_sort):
    """the scripts' own walks, for scores numpy cannot rank (NaN): by_sort False -- get_rbh.py: a row replaces its taxon's best when
    best < score; True -- rbh2phy.py: the run sorted by -score (Python's sort), the first row of every taxon.  -> (wq, ws, runs)"""
    q, s, sco = np.asarray(cols.q).tolist(), np.asarray(cols.s).tolist(), np.asarray(cols.score, dtype=np.float64).tolist()
    tx = np.asarray(tax).tolist()
    wq, ws, nrun = [], [], 0
    i, n = 0, len(q)
    while i < n:
        j = i
        while j < n and q[j] == q[i]:
            j += 1
        nrun += 1
        rows = list(range(i, j))
        if by_sort:
            rows.sort(key=lambda r: -sco[r])
        best = {}
        for r in rows:
            t = tx[s[r]]
            if t == tx[q[i]]:
                continue
            if t not in best or (not by_sort and sco[best[t]] < sco[r]):
                best[t] = r
        for r in best.values():
            wq.append(q[i]), ws.append(s[r])
        i = j
    return np.asarray(wq, dtype=np.int64), np.asarray(ws, dtype=np.int64), nrun


def _winner_list(cols, tax, n_taxa, by_sort):
    if len(cols.score) and np.isnan(np.asarray(cols.score, dtype=np.float64)).any():
        return _literal_winners(cols, tax, by_sort)
    return winners(cols, tax, n_taxa)


# ---------------------------------------------------------------------------------------------------------
# reciprocal best hits
# ---------------------------------------------------------------------------------------------------------
def pairs_from_winners(wq, ws, n_names):
    """the winner list -> (a, b): the pairs get_rbh.py prints, in its order"""
    if len(wq) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    a, b = np.minimum(wq, ws), np.maximum(wq, ws)
    key = a * max(n_names, 1) + b
    order = np.argsort(key, kind='stable')
    sk = key[order]
    start = np.maximum.accumulate(np.where(np.concatenate([[True], sk[1:] != sk[:-1]]), np.arange(len(sk)), 0))
    occ = np.empty(len(sk), dtype=np.int64)
    occ[order] = np.arange(len(sk)) - start
    even = np.flatnonzero(occ & 1)
    return a[even], b[even]


def reciprocal_best_hits(cols, sep='|'):
    """HitColumns -> (a, b): name codes of the reciprocal best hits in print order (numpy; the definition so_rbh_* are held to)"""
    tax, taxa = name_taxa(cols.names, sep)
    wq, ws, _ = _winner_list(cols, tax, len(taxa), False)
    return pairs_from_winners(wq, ws, len(cols.names))


def rbh_lines(names, a, b):
    """-> the bytes get_rbh.py writes: one `a\\tb\\n` per pair"""
    nm = names.tolist()
    return b''.join(nm[x] + b'\t' + nm[y] + b'\n' for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist()))


# ---------------------------------------------------------------------------------------------------------
# core table
# ---------------------------------------------------------------------------------------------------------
class CoreTable:
    """`slots`: the FASTA's taxa in slot order (bytes); `reference`: R (bytes); `genes[n_core]`: R's genes in table order (name codes);
    `fwd[n_core, n_slots]`: the forward winner per gene and slot, or -1; `rec[n_core, n_slots]`: 1 where a best hit back confirms it.
    A device call also leaves `pairs` (the reciprocal best hits of the same call) and `stats` (its counters)."""

    def __init__(self, slots, reference, genes, fwd, rec):
        self.slots, self.reference = slots, reference
        self.genes, self.fwd, self.rec = genes, fwd, rec
        self.pairs, self.stats = None, {}

    @classmethod
    def empty(cls, slots, reference):
        ns = len(slots)
        return cls(slots, reference, np.zeros(0, dtype=np.int64), np.zeros((0, ns), dtype=np.int64), np.zeros((0, ns), dtype=np.uint8))


def _slot_codes(names, fasta_bytes, reference, sep):
    """-> (slot of every name [unknown taxa numbered behind the FASTA's], slots, R as bytes, R's slot or -1, number of unknown taxa)"""
    slots = fasta_taxa(fasta_bytes, sep)
    ref = reference.encode('utf-8') if isinstance(reference, str) else bytes(reference)
    if ref == b'':
        if not slots:
            raise ValueError('core_table: the FASTA file has no header line: no reference taxon')
        ref = slots[0]
    tax, taxa = name_taxa(names, sep)
    where = {t: k for k, t in enumerate(slots)}
    extra = [t for t in taxa.tolist() if t not in where]
    for t in extra:
        where[t] = len(where)
    code = np.asarray([where[t] for t in taxa.tolist()], dtype=np.int64)
    return (code[tax] if len(tax) else tax), slots, ref, where.get(ref, -1), len(extra)


_ABSENT = 'core_table: a hit taxon is not among the taxa of the FASTA file (rbh2phy.py raises KeyError on such input)'


def core_table(cols, fasta_bytes, reference='', sep='|'):
    """HitColumns + the FASTA the search read -> CoreTable (numpy; the definition so_rbh_* are held to)"""
    slot, slots, ref, R, n_extra = _slot_codes(cols.names, fasta_bytes, reference, sep)
    T = len(slots) + n_extra
    if R < 0:
        return CoreTable.empty(slots, ref)
    wq, ws, _ = _winner_list(cols, slot, T, True)
    p1 = np.flatnonzero(slot[wq] == R) if len(wq) else np.zeros(0, dtype=np.int64)
    if len(p1) == 0:
        return CoreTable.empty(slots, ref)
    if n_extra:
        raise ValueError(_ABSENT)
    ug, first = np.unique(wq[p1], return_index=True)
    genes = ug[np.argsort(first, kind='stable')]
    gidx = np.full(max(len(cols.names), 1), -1, dtype=np.int64)
    gidx[genes] = np.arange(len(genes))
    last = np.full(len(genes) * T, -1, dtype=np.int64)
    np.maximum.at(last, gidx[wq[p1]] * T + slot[ws[p1]], p1)          # the last run wins, taxon by taxon
    fwd = np.where(last >= 0, ws[np.maximum(last, 0)], -1)
    rec = np.zeros(len(genes) * T, dtype=np.uint8)
    p2 = np.flatnonzero((slot[wq] != R) & (slot[ws] == R) & (gidx[ws] >= 0))
    cell = gidx[ws[p2]] * T + slot[wq[p2]]
    rec[cell[fwd[cell] == wq[p2]]] = 1
    return CoreTable(slots, ref, genes, fwd.reshape(len(genes), T), rec.reshape(len(genes), T))


def core_groups(names, table):
    """the host assembly of rbh2phy.py: CoreTable -> the kept groups, each a list of ids (bytes) in slot order"""
    nm = names.tolist()
    nt = len(table.slots)
    out = []
    for g, fwd, rec in zip(np.asarray(table.genes).tolist(), np.asarray(table.fwd).tolist(), np.asarray(table.rec).tolist()):
        ids, flag = [-1] * nt, [0] * nt
        ids[0], flag[0] = g, 1                      # slot 0, whatever slot the reference taxon has
        for t in range(nt):
            if fwd[t] >= 0:
                ids[t] = fwd[t]                     # (slot 0: the id is overwritten, the flag stays)
            if rec[t]:
                flag[t] = 1
        grp = [nm[i] for i, f in zip(ids, flag) if f == 1]
        if len(grp) * 1. / nt >= .9:
            out.append(grp)
    return out


# ---------------------------------------------------------------------------------------------------------
# the stage on the GPU (include/sohit.h so_rbh_*, csrc/rbh.hip).  No fallback: without the library or a device these raise.
# ---------------------------------------------------------------------------------------------------------
def _rbh_call(fn, head, n_names, tax, n_taxa, ref_taxon):
    """-> (a, b, genes, fwd, rec, stats) of one so_rbh_<fn> call; a refusal raises RuntimeError with the library's message"""
    import ctypes as C
    from . import _lib
    L = _lib.load()
    tax32 = np.ascontiguousarray(tax, dtype=np.int32)
    out = _lib.SoRbhResult()
    rc = getattr(L, 'so_rbh_' + fn)(*(head + [int(n_names), C.c_void_p(tax32.ctypes.data), int(n_taxa), int(ref_taxon), 0, C.byref(out)]))
    if rc != 0:
        raise RuntimeError(L.so_rbh_last_error().decode())
    try:
        arr = _lib.result_array
        nc, nt = int(out.n_core), int(n_taxa)
        stats = {k: int(getattr(out, k)) for k in ('n_runs', 'n_winners', 'n_runs_long', 'n_rows_long', 'waits')}
        return (arr(out.rbh_a, out.n_rbh, np.int64), arr(out.rbh_b, out.n_rbh, np.int64), arr(out.core_gene, nc, np.int64),
                arr(out.core_fwd, nc * nt, np.int64).reshape(nc, nt), arr(out.core_rec, nc * nt, np.uint8).reshape(nc, nt), stats)
    finally:
        L.so_rbh_free(C.byref(out))


def _cols_head(cols, device):
    import ctypes as C
    n, q32, s32 = find_orth.code_columns32(cols, 'so_rbh_cols')
    sco = np.ascontiguousarray(cols.score, dtype=np.float64)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    return [int(device), n, ptr(q32), ptr(s32), ptr(sco)], (q32, s32, sco)


def _records_head(dev, query_ids, subject_ids):
    """-> (names, head arguments of so_rbh_records, what must stay alive during the call)"""
    import ctypes as C
    d_ptr, n, device, dev = find_orth.records_on_device(dev, 'rbh')
    names, qmap, smap = find_orth._record_maps(query_ids, subject_ids)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    return names, [int(device), C.c_void_p(d_ptr), n, ptr(qmap), len(qmap), ptr(smap), len(smap)], (dev, qmap, smap)


def _is_nan_refusal(e):
    return 'NaN' in str(e)


def device_reciprocal_best_hits(cols, sep='|', device=0):
    """reciprocal_best_hits() on the GPU from host columns (so_rbh_cols): the same pairs in the same order"""
    tax, taxa = name_taxa(cols.names, sep)
    head, keep = _cols_head(cols, device)
    try:
        a, b = _rbh_call('cols', head, len(cols.names), tax, len(taxa), -1)[:2]
    except RuntimeError as e:
        if not _is_nan_refusal(e):
            raise
        return reciprocal_best_hits(cols, sep)   # (the literal loop: the call does not define a NaN's rank)
    del keep
    return a, b


def _table_from_call(res, slots, ref, n_extra):
    a, b, genes, fwd, rec, stats = res
    if len(genes) and n_extra:
        raise ValueError(_ABSENT)
    ns = len(slots)
    t = CoreTable(slots, ref, genes, fwd[:, :ns], rec[:, :ns]) if len(genes) else CoreTable.empty(slots, ref)
    t.pairs, t.stats = (a, b), stats
    return t


def device_core_table(cols, fasta_bytes, reference='', sep='|', device=0):
    """core_table() on the GPU from host columns (so_rbh_cols) -> CoreTable, with `.pairs` = the reciprocal best hits of the same call"""
    slot, slots, ref, R, n_extra = _slot_codes(cols.names, fasta_bytes, reference, sep)
    head, keep = _cols_head(cols, device)
    try:
        res = _rbh_call('cols', head, len(cols.names), slot, len(slots) + n_extra, R)
    except RuntimeError as e:
        if not _is_nan_refusal(e):
            raise
        t = core_table(cols, fasta_bytes, reference, sep)
        t.pairs = reciprocal_best_hits(cols, sep)
        return t
    del keep
    return _table_from_call(res, slots, ref, n_extra)


def device_reciprocal_best_hits_from_records(dev, query_ids, subject_ids, sep='|'):
    """reciprocal_best_hits() of columns_from_records() without the download: `dev` is a fsearch.DeviceHits, an nr.ExpandedHits or a CUDA
    uint8 torch tensor of so_hit records -> (names, a, b)"""
    names, head, keep = _records_head(dev, query_ids, subject_ids)
    tax, taxa = name_taxa(names, sep)
    a, b = _rbh_call('records', head, len(names), tax, len(taxa), -1)[:2]
    del keep
    return names, a, b


def device_core_table_from_records(dev, query_ids, subject_ids, fasta_bytes, reference='', sep='|'):
    """core_table() of the records `dev` holds (see device_reciprocal_best_hits_from_records), in ONE device call with the pairs
    -> (names, CoreTable with `.pairs`)"""
    names, head, keep = _records_head(dev, query_ids, subject_ids)
    slot, slots, ref, R, n_extra = _slot_codes(names, fasta_bytes, reference, sep)
    res = _rbh_call('records', head, len(names), slot, len(slots) + n_extra, R)
    del keep
    return names, _table_from_call(res, slots, ref, n_extra)


# ---------------------------------------------------------------------------------------------------------
# the two scripts
# ---------------------------------------------------------------------------------------------------------
def fasta_records(fasta_bytes):
    """id (the header up to the first white space) -> (header line without '>', sequence on one line), for every record"""
    out = {}
    for rec in fasta_bytes.replace(b'\r\n', b'\n').replace(b'\r', b'\n').split(b'\n>'):
        rec = rec[1:] if rec.startswith(b'>') else rec
        lines = rec.split(b'\n')
        if not lines[0].strip():
            continue
        key = lines[0].split()[0]
        if key not in out:
            out[key] = (lines[0], b''.join(l.strip() for l in lines[1:]))
    return out


def _gpu_flag(v):
    return str(v).upper()[:1] == 'T'


def _count_flag(v, most):
    """the value of a flag that takes a whole number in 0 .. most, or None"""
    v = str(v).strip()
    return int(v) if v.isdigit() and v.isascii() and int(v) <= most else None


def main_get_rbh(argv=None):
    from .fsearch import parse_flags
    argv = list(sys.argv if argv is None else argv)
    gpu = _gpu_flag(parse_flags(argv, {'-G': 'F'})['-G'])
    pos = [a for k, a in enumerate(argv[1:], 1) if not a.startswith('-G') and argv[k - 1] != '-G']
    if not pos:
        print('python this.py foo.blast8 [-G T]')
        raise SystemExit()
    with open(pos[0], 'rb') as f:
        cols = find_orth.columns_from_text(f.read())
    a, b = device_reciprocal_best_hits(cols) if gpu else reciprocal_best_hits(cols)
    sys.stdout.buffer.write(rbh_lines(cols.names, a, b))
    sys.stdout.buffer.flush()
    return 0


def main_rbh2phy(argv=None):
    import os
    from .fsearch import parse_flags
    argv = list(sys.argv if argv is None else argv)
    args = parse_flags(argv, {'-i': '', '-f': '', '-r': '', '-G': 'F', '-o': '', '-A': 'F', '-g': '1', '-t': '', '-m': 'p', '-B': '0', '-S': '1', '-K': 'F', '-k': ''})
    if args['-i'] == '' or args['-f'] == '':
        print('Usage:\n  python this.py -i foo.sc -f foo.fsa [-r taxon] [-G T] [-o groups.tsv] [-A T [-g share] [-t tree.nwk] [-m p|poisson|kimura|logdet] [-B replicates] [-S seed] [-K T [-k gcf.tsv]]]')
        print(' -i: blast -m8 or find_hit .sc file; ids are taxon|gene\n -f: the FASTA file the search read\n -r: reference taxon (default: the taxon with most genes)')
        print(' -G: the winner list and the table on the GPU [T|F]. Default: F\n -o: also write one tab-separated line of ids per group')
        print(' -A: join the families into the core-gene supermatrix from the CIGARs of the rows (find_hit.py -C T) and print it as FASTA [T|F]. Default: F')
        print(' -g: with -A T, keep the columns whose share of gaps is at most this. Default: 1 (every column)')
        print(' -t: with -A T, write the neighbour-joining tree of the taxa to this file\n -m: distance of the tree [p|poisson|kimura|logdet]. Default: p')
        print('     kimura: -log(1 - p - p*p/5); logdet: the paralinear distance from the 20 x 20 residue-pair table of every pair of taxa (with -G T: on the GPU)')
        print(' -B: with -t, label the tree\'s nodes with their bootstrap support over this many replicates (with -G T: on the GPU). Default: 0 (no labels)')
        print(' -S: seed of the bootstrap\'s column draws, 0 .. 2^64 - 1. Default: 1')
        print(' -K: with -t, label the tree\'s nodes with their gene concordance factors: the share of the core families able to decide a branch whose own')
        print('     neighbour-joining tree holds it (with -G T: on the GPU; -m p|poisson|kimura; with -B the label is boot/gcf) [T|F]. Default: F')
        print(' -k: with -K T, write join, taxa_in_clade, decisive, concordant, gcf and the clade\'s taxa per branch to this file')
        raise SystemExit()
    boot, seed = _count_flag(args['-B'], 2 ** 31 - 1), _count_flag(args['-S'], 2 ** 64 - 1)
    if boot is None or seed is None:
        sys.stderr.write('rbh2phy: -B takes a whole number of replicates from 0 to 2^31 - 1, -S a seed from 0 to 2^64 - 1\n')
        return 2
    if boot > 0 and args['-t'] == '':
        sys.stderr.write('rbh2phy: -B labels the tree that -t writes: name a tree file with -t (and join the families with -A T)\n')
        return 2
    gcf = _gpu_flag(args['-K'])
    if gcf and args['-t'] == '':
        sys.stderr.write('rbh2phy: -K labels the tree that -t writes: name a tree file with -t (and join the families with -A T)\n')
        return 2
    if args['-k'] != '' and not gcf:
        sys.stderr.write('rbh2phy: -k writes the table of the gene concordance factors: ask for them with -K T\n')
        return 2
    if gcf and args['-m'] == 'logdet':
        sys.stderr.write('rbh2phy: -K T takes -m p, poisson or kimura: a single family\'s block is where logdet has no distance\n')
        return 2
    with open(args['-i'], 'rb') as f:
        sc = f.read()
    cols = find_orth.columns_from_text(sc)
    with open(args['-f'], 'rb') as f:
        fasta = f.read()
    table = device_core_table(cols, fasta, args['-r']) if _gpu_flag(args['-G']) else core_table(cols, fasta, args['-r'])
    if _gpu_flag(args['-A']):
        from . import phy
        try:
            share = float(args['-g'])
            sm = phy.run_align(sc, fasta, cols, table, share, args['-m'], args['-t'], _gpu_flag(args['-G']), boot=boot, seed=seed,
                               **({'concordance': True, 'gcf_path': args['-k']} if gcf else {}))
        except (phy.MissingCigar, phy.DistanceRefused, phy.ConcordanceRefused) as e:
            sys.stderr.write('rbh2phy: %s\n' % e)
            return 2
        except ValueError as e:
            sys.stderr.write('rbh2phy: %s\n' % e)
            return 1
        sys.stderr.write('rbh2phy: %d core families of reference taxon %s joined into %d columns (%d kept) for %d taxa\n'
                         % (len(sm.col_off) - 1, table.reference.decode('utf-8', 'replace'), len(sm.gaps), len(sm.keep), len(sm.taxa)))
        return 0
    groups = core_groups(cols.names, table)
    recs = fasta_records(fasta)
    d = '%s_alns_tmp' % args['-i']
    os.makedirs(d, exist_ok=True)
    for k, grp in enumerate(groups):
        with open(os.path.join(d, '%d.fsa' % k), 'wb') as o:
            for g in grp:
                head, seq = recs[g]
                o.write(b'>' + head + b'\n' + seq + b'\n')
    if args['-o']:
        with open(args['-o'], 'wb') as o:
            o.write(b''.join(b'\t'.join(grp) + b'\n' for grp in groups))
    sys.stderr.write('rbh2phy: %d core families of reference taxon %s written to %s/ ; aligning them (famsa | mafft | muscle) and joining '
                     'the alignments is not part of this port\n' % (len(groups), table.reference.decode('utf-8', 'replace'), d))
    return 0
