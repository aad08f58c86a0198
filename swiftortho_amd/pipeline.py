"""search -> orthology relations without the text round trip (SURVEY.md 8f-1 / BASELINE config 5).

The reference pipeline writes the 16-column .sc file and bin/find_orth.py parses it back.  Here the hit records the
search produced (fixed-width so_hit structs, `Hits.array()`; on several GPUs the records gathered over RCCL) are handed
to the columnar find_orth stage directly; the .sc file is still written when asked for (it is the drop-in artefact), but
nothing reads it.  `orthology_from_search()` is what `bin/find_hit.py ... && bin/find_orth.py -i x.sc` computes.
`groups_from_search()` goes one stage further, to what `bin/find_cluster.py -i x.orth -a mcl` (or `-a apc`) prints: the relation tables
the device computed are clustered as columns (find_cluster.groups_from_tables, apc_from_tables), so no relation text lies between the
stages either."""
import os
import time


def orthology_from_search(fasta_path, sc_path=None, coverage=.5, identity=0., norm='no', sep='|', device=0, device_stage=False, **search_kw):
    """self-search of one proteome on the GPU, then IP / OT / CO relations from the hit RECORDS.
    device_stage=True: the records stay in HBM (search_device) and the candidate stage of find_orth runs on them there
    (find_orth.relations_from_device); they are downloaded only when `sc_path` asks for the file.
    device_stage='relations': the relation tables are computed on the device as well (find_orth.device_relation_tables_from_records)
    and the host only writes the text.
    -> (relation lines as bytes, dict of stage wall times in seconds; with device_stage also 'orth_candidates', or 'orth_relations')"""
    from . import find_orth, fsearch
    t = {}
    t0 = time.time()
    data = open(fasta_path, 'rb').read()
    ids = find_orth.fasta_ids(data)
    s = fsearch.Searcher(device=device, **search_kw)
    try:
        s.load_ref_bytes(data)
        s.load_queries_bytes(data)
        t['load'] = time.time() - t0
        t0 = time.time()
        if device_stage:
            return _device_stage(s, ids, sc_path, coverage, identity, norm, sep, t, t0, relations=device_stage == 'relations')
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


def _device_stage(s, ids, sc_path, coverage, identity, norm, sep, t, t0, relations=False):
    """orthology_from_search() from the search on, with the records left on the device (the caller closes the searcher)"""
    import numpy as np
    from . import find_orth, fsearch
    dev = s.search_device()
    t['search'] = time.time() - t0
    t0 = time.time()
    if sc_path:
        raw = dev.tensor().cpu().numpy() if len(dev) else np.zeros(0, dtype=np.uint8)
        arr, n = fsearch.hits_from_bytes(s, raw)
        s._chk(s.L.so_write_sc(s.h, arr, n, os.fsencode(sc_path), b'w'))
        t['write_sc'] = time.time() - t0
        t0 = time.time()
    if relations:
        names, tables = find_orth.device_relation_tables_from_records(dev, ids, ids, coverage, identity, norm, sep)
        t['orth_relations'] = time.time() - t0
        lines = find_orth.lines_from_tables(names, tables)
    else:
        names, tax, taxa, cand = find_orth._device_records(dev, ids, ids, coverage, identity, norm, sep)
        t['orth_candidates'] = time.time() - t0
        lines = find_orth.relations_from_candidates(names, tax, taxa, cand)
    t['find_orth'] = time.time() - t0
    t['rows'] = len(dev)
    return lines, t


def groups_from_search(fasta_path, inflation=1.5, coverage=.5, identity=0., norm='no', sep='|', device=0, device_stage='all', orth_path=None, sc_path=None,
                       algorithm='mcl', damp=0.5, **search_kw):
    """one process from a FASTA file to ortholog groups: self-search on the GPU, the relation tables on the device from the records in
    HBM (find_orth.device_relation_tables_from_records), the groups from those tables (find_cluster.groups_from_tables) -- what
    `bin/find_hit.py ... && bin/find_orth.py -i x.sc > x.orth && bin/find_cluster.py -i x.orth -a mcl -I <inflation>` prints, one
    group per line.  `device_stage`: find_cluster's (False | True | 'matrix' | 'all').  `algorithm='apc'`: the groups of
    `bin/find_cluster.py -i x.orth -a apc -d <damp>` instead (find_cluster.apc_from_tables; any true `device_stage` = its one device call
    from the rows to the exemplar labels); any other name raises ValueError before anything is loaded.  The .sc and the .orth file are
    written only when `sc_path` / `orth_path` name them; nothing reads them.
    -> (groups as lists of ids, dict of stage wall times in seconds: load, search, [write_sc,] orth_relations, [write_orth,] cluster,
    and the counts rows, relations, groups)"""
    if algorithm not in ('mcl', 'apc'):
        raise ValueError("groups_from_search: unknown algorithm %r ('mcl' and 'apc' are provided)" % (algorithm,))
    import numpy as np
    from . import find_cluster, find_orth, fsearch
    t = {}
    t0 = time.time()
    data = open(fasta_path, 'rb').read()
    ids = find_orth.fasta_ids(data)
    s = fsearch.Searcher(device=device, **search_kw)
    try:
        s.load_ref_bytes(data)
        s.load_queries_bytes(data)
        t['load'] = time.time() - t0
        t0 = time.time()
        dev = s.search_device()
        t['search'] = time.time() - t0
        t0 = time.time()
        if sc_path:
            raw = dev.tensor().cpu().numpy() if len(dev) else np.zeros(0, dtype=np.uint8)
            arr, n = fsearch.hits_from_bytes(s, raw)
            s._chk(s.L.so_write_sc(s.h, arr, n, os.fsencode(sc_path), b'w'))
            t['write_sc'] = time.time() - t0
            t0 = time.time()
        names, tables = find_orth.device_relation_tables_from_records(dev, ids, ids, coverage, identity, norm, sep)
        t['orth_relations'] = time.time() - t0
        t['rows'] = len(dev)
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
