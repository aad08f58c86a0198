"""search -> orthology relations without the text round trip (SURVEY.md 8f-1 / BASELINE config 5).

The reference pipeline writes the 16-column .sc file and bin/find_orth.py parses it back.  Here the hit records the
search produced (fixed-width so_hit structs, `Hits.array()`; on several GPUs the records gathered over RCCL) are handed
to the columnar find_orth stage directly; the .sc file is still written when asked for (it is the drop-in artefact), but
nothing reads it.  `orthology_from_search()` is what `bin/find_hit.py ... && bin/find_orth.py -i x.sc` computes.
`groups_from_search()` goes one stage further, to what `bin/find_cluster.py -i x.orth -a mcl` (or `-a apc`) prints: the relation tables
the device computed are clustered as columns (find_cluster.groups_from_tables, apc_from_tables), so no relation text lies between the
stages either.
`collapse=True` on either function is the reference's recommended route (scripts/run_all_fast.py: nr_flt -> find_hit -> nr2full -> ...)
in the same process: identical sequences are searched once (nr.collapse_tables), the records of the collapsed search are multiplied back
in HBM (nr.device_expand, so_nr_expand) in nr2full's order, and the device stages of find_orth read the expanded records where they lie."""
import os
import time


def _collapse(data, t):
    """collapse=True, the host half: -> (CollapseTables, the bytes to search, the ids of the full file)"""
    from . import nr
    t0 = time.time()
    tables = nr.collapse_tables(data)
    t['collapse'] = time.time() - t0
    return tables, tables.fasta, tables.ids


def _check_collapsed(s, tables):
    if s.num_queries != len(tables.off) - 1 or s.num_refs != len(tables.off) - 1:
        raise ValueError('collapse=True: the search reads %d records in the collapsed file, the member table holds %d (a record without residues?)'
                         % (s.num_queries, len(tables.off) - 1))


def _search_records(s, tables, sc_path, t, t0):
    """search_device, the .sc file when asked for, and with `tables` (collapse=True) the expansion on the device
    -> (the records the relation stage reads, the object to close after it or None, t0)"""
    import numpy as np
    from . import fsearch, nr
    dev = s.search_device()
    t['search'] = time.time() - t0
    t0 = time.time()
    if sc_path:
        raw = dev.tensor().cpu().numpy() if len(dev) else np.zeros(0, dtype=np.uint8)
        arr, n = fsearch.hits_from_bytes(s, raw)
        if tables is None:
            s._chk(s.L.so_write_sc(s.h, arr, n, os.fsencode(sc_path), b'w'))
        else:
            # the cold path: the collapsed rows as text, multiplied out by the text nr2full(); nothing reads the file
            import tempfile
            fd, tmp = tempfile.mkstemp(suffix='.sc', dir=os.path.dirname(os.path.abspath(sc_path)))
            os.close(fd)
            try:
                s._chk(s.L.so_write_sc(s.h, arr, n, os.fsencode(tmp), b'w'))
                with open(tmp, 'r') as f, open(sc_path, 'w') as o:
                    for l in nr.nr2full(f):
                        o.write(l + '\n')
            finally:
                os.remove(tmp)
        t['write_sc'] = time.time() - t0
        t0 = time.time()
    if tables is None:
        return dev, None, t0
    exp = nr.device_expand(dev, tables)
    t['expand'] = time.time() - t0
    t['rows_collapsed'] = len(dev)
    return exp, exp, time.time()


def orthology_from_search(fasta_path, sc_path=None, coverage=.5, identity=0., norm='no', sep='|', device=0, device_stage=False, collapse=False, **search_kw):
    """self-search of one proteome on the GPU, then IP / OT / CO relations from the hit RECORDS.
    device_stage=True: the records stay in HBM (search_device) and the candidate stage of find_orth runs on them there
    (find_orth.relations_from_device); they are downloaded only when `sc_path` asks for the file.
    device_stage='relations': the relation tables are computed on the device as well (find_orth.device_relation_tables_from_records)
    and the host only writes the text.
    collapse=True (needs a true device_stage): exact duplicates are searched once and multiplied back on the device -- the lines are those
    of find_orth on the .sc file nr.search_collapsed() writes, byte for byte, and `sc_path` receives that file's bytes (through the text
    nr2full(), the cold path).  The timing dict then also holds 'collapse', 'expand', 'rows_collapsed'; 'rows' counts the expanded records.
    Files nr.collapse_tables() refuses (an empty, repeated or ';;;'-holding id) raise its ValueError: the script chain serves them.
    -> (relation lines as bytes, dict of stage wall times in seconds; with device_stage also 'orth_candidates', or 'orth_relations')"""
    from . import find_orth, fsearch
    if collapse and not device_stage:
        raise ValueError("orthology_from_search: collapse=True expands the records on the device: device_stage must be True or 'relations'")
    t = {}
    t0 = time.time()
    data = open(fasta_path, 'rb').read()
    tables = None
    if collapse:
        tables, data, ids = _collapse(data, t)
    else:
        ids = find_orth.fasta_ids(data)
    s = fsearch.Searcher(device=device, **search_kw)
    try:
        s.load_ref_bytes(data)
        s.load_queries_bytes(data)
        t['load'] = time.time() - t0 - t.get('collapse', 0.)
        t0 = time.time()
        if device_stage:
            return _device_stage(s, ids, sc_path, coverage, identity, norm, sep, t, t0, relations=device_stage == 'relations', tables=tables)
        hits = s.search()
        t['search'] = time.time() - t0
        t0 = time.time()
        rec = hits.array()
        if sc_path:
            hits.write(sc_path, 'w')
            t['write_sc'] = time.time() - t0
            t0 = time.time()
        hits.close()
    finally:
        s.close()
    lines = find_orth.relations_from_records(rec, ids, ids, coverage, identity, norm, sep)
    t['find_orth'] = time.time() - t0
    t['rows'] = len(rec)
    return lines, t


def _device_stage(s, ids, sc_path, coverage, identity, norm, sep, t, t0, relations=False, tables=None):
    """orthology_from_search() from the search on, with the records left on the device (the caller closes the searcher)"""
    from . import find_orth
    if tables is not None:
        _check_collapsed(s, tables)
    dev, owned, t0 = _search_records(s, tables, sc_path, t, t0)
    try:
        if relations:
            names, rel = find_orth.device_relation_tables_from_records(dev, ids, ids, coverage, identity, norm, sep)
            t['orth_relations'] = time.time() - t0
            lines = find_orth.lines_from_tables(names, rel)
        else:
            names, tax, taxa, cand = find_orth._device_records(dev, ids, ids, coverage, identity, norm, sep)
            t['orth_candidates'] = time.time() - t0
            lines = find_orth.relations_from_candidates(names, tax, taxa, cand)
        t['find_orth'] = time.time() - t0
        t['rows'] = len(dev)
    finally:
        if owned is not None:
            owned.close()
    return lines, t


def core_genes_from_search(fasta_path, reference='', device=0, collapse=False, sep='|', sc_path=None, **search_kw):
    """one process from a FASTA file to the reciprocal best hits between its taxa and the core-gene families of `reference` (default:
    the taxon with most genes): self-search on the GPU, then ONE device call on the records where they lie (rbh.device_core_table_from_records,
    so_rbh_records) -- what `bin/find_hit.py ... && scripts/get_rbh.py x.sc` prints and the groups `scripts/rbh2phy.py -i x.sc -f x.fsa
    [-r reference]` writes, with no .sc text in between (`sc_path` still receives the file when named; nothing reads it).
    collapse=True: exact duplicates are searched once and the records multiplied back on the device, as in orthology_from_search.
    -> (pairs as a list of (id, id) bytes in print order, groups as lists of ids (bytes), dict of stage wall times in seconds: load, search,
    [write_sc,] rbh, and the counts rows, pairs, groups, core_genes)"""
    from . import find_orth, fsearch, rbh
    t = {}
    t0 = time.time()
    full = open(fasta_path, 'rb').read()
    data, tables = full, None
    if collapse:
        tables, data, ids = _collapse(full, t)
    else:
        ids = find_orth.fasta_ids(full)
    s = fsearch.Searcher(device=device, **search_kw)
    try:
        s.load_ref_bytes(data)
        s.load_queries_bytes(data)
        t['load'] = time.time() - t0 - t.get('collapse', 0.)
        t0 = time.time()
        if tables is not None:
            _check_collapsed(s, tables)
        dev, owned, t0 = _search_records(s, tables, sc_path, t, t0)
        try:
            names, table = rbh.device_core_table_from_records(dev, ids, ids, full, reference, sep)
            t['rbh'] = time.time() - t0
            t['rows'] = len(dev)
        finally:
            if owned is not None:
                owned.close()
    finally:
        s.close()
    nm = names.tolist()
    pairs = [(nm[a], nm[b]) for a, b in zip(table.pairs[0].tolist(), table.pairs[1].tolist())]
    groups = rbh.core_groups(names, table)
    t['pairs'], t['groups'], t['core_genes'] = len(pairs), len(groups), len(table.genes)
    return pairs, groups, t


def groups_from_search(fasta_path, inflation=1.5, coverage=.5, identity=0., norm='no', sep='|', device=0, device_stage='all', orth_path=None, sc_path=None,
                       algorithm='mcl', damp=0.5, collapse=False, **search_kw):
    """one process from a FASTA file to ortholog groups: self-search on the GPU, the relation tables on the device from the records in
    HBM (find_orth.device_relation_tables_from_records), the groups from those tables (find_cluster.groups_from_tables) -- what
    `bin/find_hit.py ... && bin/find_orth.py -i x.sc > x.orth && bin/find_cluster.py -i x.orth -a mcl -I <inflation>` prints, one
    group per line.  `device_stage`: find_cluster's (False | True | 'matrix' | 'all').  `algorithm='apc'`: the groups of
    `bin/find_cluster.py -i x.orth -a apc -d <damp>` instead (find_cluster.apc_from_tables; any true `device_stage` = its one device call
    from the rows to the exemplar labels); any other name raises ValueError before anything is loaded.  The .sc and the .orth file are
    written only when `sc_path` / `orth_path` name them; nothing reads them.  collapse=True: exact duplicates are searched once and the
    records multiplied back on the device, as in orthology_from_search (the dict then also holds collapse, expand, rows_collapsed).
    -> (groups as lists of ids, dict of stage wall times in seconds: load, search, [write_sc,] orth_relations, [write_orth,] cluster,
    and the counts rows, relations, groups)"""
    if algorithm not in ('mcl', 'apc'):
        raise ValueError("groups_from_search: unknown algorithm %r ('mcl' and 'apc' are provided)" % (algorithm,))
    from . import find_cluster, find_orth, fsearch
    t = {}
    t0 = time.time()
    data = open(fasta_path, 'rb').read()
    members = None
    if collapse:
        members, data, ids = _collapse(data, t)
    else:
        ids = find_orth.fasta_ids(data)
    s = fsearch.Searcher(device=device, **search_kw)
    try:
        s.load_ref_bytes(data)
        s.load_queries_bytes(data)
        t['load'] = time.time() - t0 - t.get('collapse', 0.)
        t0 = time.time()
        if members is not None:
            _check_collapsed(s, members)
        dev, owned, t0 = _search_records(s, members, sc_path, t, t0)
        try:
            names, tables = find_orth.device_relation_tables_from_records(dev, ids, ids, coverage, identity, norm, sep)
            t['orth_relations'] = time.time() - t0
            t['rows'] = len(dev)
        finally:
            if owned is not None:
                owned.close()
    finally:
        s.close()
    t0 = time.time()
    if orth_path:
        with open(orth_path, 'wb') as f:
            f.write(b''.join(l + b'\n' for l in find_orth.lines_from_tables(names, tables)))
        t['write_orth'] = time.time() - t0
        t0 = time.time()
    if algorithm == 'apc':
        groups = find_cluster.apc_from_tables(names, tables, damp, device_stage=bool(device_stage))
    else:
        groups = find_cluster.groups_from_tables(names, tables, inflation, device_stage)
    t['cluster'] = time.time() - t0
    t['relations'] = len(tables.ip_a) + len(tables.ot_a) + len(tables.co_a)
    t['groups'] = len(groups)
    return groups, t


def pan_genome_from_search(fasta_path, ts=.05, tc=.95, taxa=None, pan_device=True, **groups_from_search_kw):
    """one process from a FASTA file to the pan-genome statistics of its ortholog groups: groups_from_search(fasta_path,
    **groups_from_search_kw), then the pan-genome stage (swiftortho_amd.pan) on those groups -- what `scripts/pan_genome.py -i x.fsa -g
    x.clsr -l ts -u tc` computes on the groups file of the same search, with no groups text in between.  `taxa`: the column order
    (None: the taxa of the header lines by first appearance; the script has Python's set order).  pan_device: the count of taxa per
    family, the types and the rarefaction in one device call (pan.device_pan_genome), else by the numpy definitions.
    -> (taxa, type per row (uint8: 0 Specific, 1 Share, 2 Core; the file rows first, then one row per ungrouped gene), (core, share,
    specific) counted over the group rows, (core, spec, panz) int64[20, taxa - 1], the dict of groups_from_search with pan_host (ids and
    taxa coded on the host) and pan (the stage) added, in seconds)"""
    from . import pan
    groups, t = groups_from_search(fasta_path, **groups_from_search_kw)
    t0 = time.time()
    with open(fasta_path, 'r') as f:
        text = f.read()
    if taxa is None:
        taxa = pan.taxa_of_fasta(text)
    table = pan.member_table_of(groups, pan.fasta_ids(text), taxa)
    t['pan_host'] = time.time() - t0
    t0 = time.time()
    res = pan.pan_genome(table, len(taxa), ts, tc, device_stage=pan_device, want_counts=False, device=groups_from_search_kw.get('device', 0))
    t['pan'] = time.time() - t0
    return list(taxa), res.types, res.totals, (res.core, res.spec, res.panz), t


def family_links_from_search(fasta_path, jaccard='0.8', k_min=2, ts=.05, tc=.95, pan_device=True, **groups_from_search_kw):
    """one process from a FASTA file to the phyletic profiles of its ortholog groups: groups_from_search(fasta_path,
    **groups_from_search_kw), then phyletic.family_links on those groups -- what `scripts/phyletic_links.py -i x.fsa -g x.clsr -l ts -u tc
    -j jaccard -k k_min` computes on the groups file of the same search, with no groups text in between.  pan_device: the family pairs
    in one device call (phyletic.device_linked_pairs, so_phyletic_pairs), else by the numpy definition.
    -> (taxa in sorted order, phyletic.Links -- the linked pairs of group rows by (a, b), the genomes they share, the genomes of every row --,
    the dict of groups_from_search with pan_host (ids and taxa coded on the host) and links (the stage) added, in seconds)"""
    from . import pan, phyletic
    groups, t = groups_from_search(fasta_path, **groups_from_search_kw)
    t0 = time.time()
    with open(fasta_path, 'r') as f:
        text = f.read()
    taxa = sorted(pan.taxa_of_fasta(text))
    table = pan.member_table_of(groups, pan.fasta_ids(text), taxa)
    t['pan_host'] = time.time() - t0
    t0 = time.time()
    links = phyletic.family_links(table, taxa, ts, tc, jaccard, k_min, device_stage=pan_device, device=groups_from_search_kw.get('device', 0))
    t['links'] = time.time() - t0
    return taxa, links, t


def fusion_links_from_search(fasta_path, coverage='0.7', max_overlap=0, same_taxon=True, device=0, collapse=False, sep='|', sc_path=None, device_stage=True,
                             **search_kw):
    """one process from a FASTA file to its gene-fusion links: self-search on the GPU, then ONE device call on the records where they lie
    (fusion.device_fusion_links_from_records, so_fusion_records) -- what `bin/find_hit.py ... && scripts/fusion_links.py -i x.sc -c coverage
    -o max_overlap -s T|F` prints, with no .sc text in between (`sc_path` still receives the file when named; nothing reads it).
    collapse=True: exact duplicates are searched once and the records multiplied back on the device, as in core_genes_from_search.
    device_stage=False: the records are downloaded and the numpy definition runs on them (no collapse then).
    -> (names (bytes, ascending), fusion.Links -- fusion.links_text(names, links) is the script's output --, dict of stage wall times in
    seconds: load, search, [write_sc,] fusion, and the counts rows, links)"""
    from . import find_orth, fsearch, fusion, rbh
    if collapse and not device_stage:
        raise ValueError('fusion_links_from_search: collapse=True expands the records on the device: device_stage must be True')
    num, den = fusion.coverage_fraction(coverage)
    max_overlap = fusion.overlap_value(max_overlap)
    t = {}
    t0 = time.time()
    full = open(fasta_path, 'rb').read()
    data, tables = full, None
    if collapse:
        tables, data, ids = _collapse(full, t)
    else:
        ids = find_orth.fasta_ids(full)
    s = fsearch.Searcher(device=device, **search_kw)
    try:
        s.load_ref_bytes(data)
        s.load_queries_bytes(data)
        t['load'] = time.time() - t0 - t.get('collapse', 0.)
        t0 = time.time()
        if device_stage:
            if tables is not None:
                _check_collapsed(s, tables)
            dev, owned, t0 = _search_records(s, tables, sc_path, t, t0)
            try:
                names, links = fusion.device_fusion_links_from_records(dev, ids, ids, max_overlap, num, den, same_taxon, sep)
                t['rows'] = len(dev)
            finally:
                if owned is not None:
                    owned.close()
        else:
            hits = s.search()
            t['search'] = time.time() - t0
            t0 = time.time()
            rec = hits.array()
            if sc_path:
                hits.write(sc_path, 'w')
                t['write_sc'] = time.time() - t0
                t0 = time.time()
            hits.close()
            names, qmap, smap = find_orth._record_maps(ids, ids)
            col = lambda k: rec[k].astype('int64')
            table = fusion.Table(names, qmap[col('qidx')].astype('int64'), smap[col('sidx')].astype('int64'), col('qst'), col('qed'), col('sst'), col('sed'), col('slen'),
                                 col('qlen'))
            links = fusion.fusion_links(table, rbh.name_taxa(names, sep)[0], max_overlap, num, den, same_taxon)
            t['rows'] = len(rec)
        t['fusion'] = time.time() - t0
    finally:
        s.close()
    t['links'] = len(links)
    return names, links, t


def species_tree_from_search(fasta_path, reference='', gap_share=1.0, model='p', device_stage=True, device=0, sep='|', boot=0, boot_seed=1, concordance=False, **search_kw):
    """one process from a FASTA file to the species tree of its taxa: self-search on the GPU with a CIGAR on every row, the core-gene
    table of `reference` (default: the taxon with most genes), the core-gene supermatrix from the rows' own alignments (swiftortho_amd.phy:
    no aligner runs), the distances over its kept columns (`gap_share`, `model` 'p', 'poisson', 'kimura' or 'logdet' -- the last from the substitution counts, device_stage: so_phy_subst) and neighbour joining -- what
    `bin/find_hit.py -C T ... && scripts/rbh2phy.py -A T -t x.nwk` write.  device_stage: the table, the picked rows, the matrix and the
    pair counts on the GPU (so_rbh_cols, so_phy_rows, so_phy_build), else by the numpy definitions; the records and the CIGARs are the host
    copies either way.  boot > 0: the tree's nodes carry their bootstrap support over `boot` replicates of the kept columns drawn from
    `boot_seed` (phy.bootstrap; device_stage: so_phy_boot); the dict holds boot and boot_valid, the replicates asked for and kept (0, 0 without).
    concordance: the nodes carry their gene concordance factors (phy.gene_concordance; device_stage: so_phy_gene; with boot > 0 the label is
    boot/gcf); the dict then holds 'gcf', what phy.tree leaves under that key (the printed tree's splits, decisive, concordant, ok, n_present).
    -> (Newick bytes, phy.Supermatrix, dict of stage wall times in seconds: load, search, rbh, supermatrix, tree, and the counts rows,
    families, columns, kept)"""
    from . import find_orth, fsearch, phy, rbh
    t = {}
    t0 = time.time()
    full = open(fasta_path, 'rb').read()
    ids = find_orth.fasta_ids(full)
    s = fsearch.Searcher(device=device, **search_kw)
    try:
        s.load_ref_bytes(full)
        s.load_queries_bytes(full)
        t['load'] = time.time() - t0
        t0 = time.time()
        hits = s.search(cigar=True)
        try:
            rec = hits.array()
            t['search'] = time.time() - t0
            t0 = time.time()
            cols = find_orth.columns_from_records(rec, ids, ids)
            table = rbh.device_core_table(cols, full, reference, sep, device) if device_stage else rbh.core_table(cols, full, reference, sep)
            t['rbh'] = time.time() - t0
            t0 = time.time()
            ops, off = hits.cigar_buffer()
            rows = phy.RecordRows(cols, rec['qst'], rec['sst'], ops, off)
            sm = phy.supermatrix(cols.names, table, rbh.fasta_records(full), rows, gap_share, device_stage, device=device)
            t['supermatrix'] = time.time() - t0
        finally:
            hits.close()
    finally:
        s.close()
    t0 = time.time()
    boot_stats = {}
    newick = phy.tree(sm, model, boot, boot_seed, device_stage, device, boot_stats, **({'concordance': True} if concordance else {}))
    t['tree'] = time.time() - t0
    if concordance:
        t['gcf'] = boot_stats['gcf']
    t['boot'], t['boot_valid'] = boot_stats.get('boot', 0), boot_stats.get('boot_valid', 0)
    t['rows'], t['families'], t['columns'], t['kept'] = len(rec), len(sm.col_off) - 1, len(sm.gaps), len(sm.keep)
    return newick, sm, t


def gene_content_tree_from_search(fasta_path, metric='jaccard', boot=0, boot_seed=1, pan_device=True, **groups_from_search_kw):
    """one process from a FASTA file to the gene-content tree of its genomes: groups_from_search(fasta_path, **groups_from_search_kw),
    then pan.content_tree on those groups -- what `scripts/pan_genome.py -i x.fsa -g x.clsr -t x.nwk -d x.tsv -m metric -B boot -S
    boot_seed` writes on the groups file of the same search, with no groups text in between.  pan_device: the shared-family counts and
    the bootstrap replicates on the device (pan.device_shared_counts, so_pan_shared; the replicates' trees by so_phy_nj_splits), else by
    the numpy definitions.
    -> (taxa in sorted order, Newick bytes, S int64[T, T] (the families every pair shares), D float64[T, T], the dict of
    groups_from_search with pan_host (ids and taxa coded on the host) and content (the stage) added, in seconds)"""
    from . import pan
    groups, t = groups_from_search(fasta_path, **groups_from_search_kw)
    t0 = time.time()
    with open(fasta_path, 'r') as f:
        text = f.read()
    taxa = pan.taxa_of_fasta(text)
    table = pan.member_table_of(groups, pan.fasta_ids(text), taxa)
    t['pan_host'] = time.time() - t0
    t0 = time.time()
    newick, S, D = pan.content_tree(table, taxa, metric, boot, boot_seed, device_stage=pan_device, device=groups_from_search_kw.get('device', 0))
    t['content'] = time.time() - t0
    return sorted(taxa), newick, S, D, t
