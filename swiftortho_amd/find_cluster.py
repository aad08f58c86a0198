"""find_cluster -- counterpart of SwiftOrtho's bin/find_cluster.py for `-a mcl` and `-a apc`: from the orthology
relations file (find_orth output) to ortholog groups, one tab-separated group per line, same flags,
same stdout.

Last stage of BASELINE config 5 (find_hit -> find_orth -> find_cluster -a mcl -I 1.5); a SURVEY.md 8f
"next" row.  The Markov-cluster iteration -- the one data-parallel part of this stage: column normalisation,
sparse x sparse expansion, inflation, pruning on float32 CSR matrices -- runs on the GPU (libsohit `so_mcl`,
csrc/mcl.hip) with scipy's arithmetic order, because the pruning decisions, and therefore the groups, depend
on it; the graph bookkeeping around it (best-neighbour components, batching, the read-out) is host code.  With `-G T`
(`cnc(device_stage=True)`) the first half of that bookkeeping -- best-neighbour components, level-2 groups, the rows to keep --
runs on the GPU too (libsohit `so_cnc_groups`, csrc/cnc.hip), pinned number for number to `group_numbers()`; default off, same output.
With `-G M` (`cnc(device_stage='matrix')`) every batch also goes from its rows to its surviving pairs in one device call (libsohit
`so_mcl_rows`, csrc/mcl.hip): the matrix is assembled, iterated and read out on the GPU, pinned bit for bit to `block_matrix_arrays()` and
`surviving_pair_columns()`; default off, same output.
With `-G A` (`cnc(device_stage='all')`) the front of cnc between the tokeniser and the batches is one device call as well (libsohit
`so_cnc_plan`, csrc/cnc.hip): genes numbered by first appearance, the component stage, the kept rows, their `sort -n` order and the
batch cuts, pinned field for field to `row_plan()`; the rest is `-G M`; default off, same output.  `cnc_columns()` is cnc behind its
tokeniser and `groups_from_tables()` feeds it find_orth's relation tables, so that `pipeline.groups_from_search()` goes from a FASTA
file to the groups in one process without relation text.
So does the affinity-propagation loop of `-a apc` (libsohit `so_apc`, csrc/apc.hip), with the reference's own
arithmetic order.  With `-a apc -G A` (`apc(device_stage=True)`) the rows go from their id codes to the exemplar labels in one device call
(libsohit `so_apc_rows`, the same file): gene numbers, preference, the entry layout and the loop, pinned field for field to
`apc_entry_columns()` and bit for bit to `so_apc`; `apc_columns()` is apc behind its tokeniser and `apc_from_tables()` feeds it find_orth's
relation tables; the read-out stays on the host; default off, same output.  There is no CPU path for either loop: without the HIP library `-a mcl` and `-a apc` fail.
`-a apc` has to be named on the command line: a command without `-a` is still refused (exit code 2), as are `-a sap`
(it needs pysapc), `-a apc` with a batch size `-b` of 0 or below (the reference's in-place float32 variant) and every
other spelling that starts with `ap` (the reference then runs without preference entries).

Reference behaviour reproduced (bin/find_cluster.py, `cnc` 1470-1673, `mcl_xyz` 1425-1467, `mcl`
652-689, `normalize` 636-646), including its accidents, because they decide which genes appear:
  * rows `TYPE a b score` (or `a b score`); only rows with a <= b are used;
  * level 1: every gene is linked to its best-scoring neighbour(s) (ties all kept); connected
    components of that graph are numbered in discovery order;
  * level 2: components joined by any edge are merged -- but an edge is only seen when BOTH of its
    level-1 component numbers are non-zero (`if X and Y`), so component 0 never merges;
  * an edge is kept when both ends carry the same level-2 number and that number is non-zero
    (`if cx and cy and cx == cy`): everything in level-2 group 0 is dropped from the output, and all
    genes outside any level-2 group share the number -1 and are clustered together as one block;
  * the kept edges, sorted like `LC_ALL=C sort -n`, go through MCL in batches cut at group changes
    once more than 10^7 edges have accumulated;
  * MCL on a (D+1)x(D+1) float32 matrix with self-loops = the largest incident weight: column
    normalisation, squaring, inflation, pruning below 1e-5, at most 100 rounds, convergence test every
    5th round against the normalised matrix of that round; groups = connected components of the
    entries > 1e-5 -- read, as the reference does, by zipping the coordinates of the non-zero entries
    with the raw data array (which still holds the pruned zeros when the round limit was hit).

And for `-a apc` (`fc2mat` 767-858, `apclust_blk` 404-513 with its passes 309-401, `main` 1705-1723):
  * rows with a > b are skipped before the genes are numbered; a gene is numbered by its first appearance even when
    the row's weight then fails to parse (`float(w)`, then `float(w.split('rm')[0])`, else the row is dropped): such a
    gene is a group of its own; a row of neither three nor four fields raises;
  * every kept row gives the entries (a, b, w) and (b, a, w); repeated pairs and self pairs are entries of their own;
    after all rows one preference entry (g, g, -20 x number of distinct `id.split('|')[0]`) per gene; gene numbers,
    scores, responsibilities and availabilities are stored as float32, the arithmetic on them is float64;
  * the two largest values of a row (R + A) are never reset between rounds: they start at 0 (the first at gene 0) and run
    on over all rounds, and a displaced maximum is not demoted to second place;
  * the responsibility of the diagonal enters the availabilities unrounded, the column sums add the rounded ones in
    entry order;
  * the convergence counter is handed to `get_change` by value, so the loop always runs its 100 rounds;
  * a gene's exemplar is the first entry of its row that reaches the row's maximum of R + A; groups = connected
    components of the gene -> exemplar graph, genes in number order;
  * `-p` and `-t` are parsed and never used; the batch size `-b` (> 0) cannot change a result;
  * the reference writes and removes `<input>.npy`; no file is written here.
"""
import sys

import numpy as np

DEFAULTS = {'-i': '', '-d': '0.5', '-p': '-10000', '-I': '1.5', '-a': 'apc', '-t': '2', '-b': '25000000', '-G': 'F'}


def manual_print(prog='find_cluster.py'):
    print('Usage:')
    print('    python %s -i foo.xyz -d 0.5' % prog)
    print('Parameters:')
    print('  -i: tab-delimited file which contain 3 columns')
    print('  -d: damp for apc')
    print('  -p: parameter of preference for apc')
    print('  -I: inflation parameter for mcl')
    print('  -a: algorithm (mcl or apc)')
    print('  -t: cpu number')
    print('  -b: batch size for apc (above 0; no effect on the result)')
    print('  -G: stages of mcl on the GPU beside the loop [A|T|M|F]: T = the component stage, M = that and every batch from its rows to')
    print('      its surviving pairs (matrix assembly and read-out), A = M and the whole row plan in front of the batches (gene numbers,')
    print('      kept rows, their order). Default: F (same output).  With -a apc: A = the rows go from their id codes to the exemplar labels')
    print('      in one device call (numbering, entry layout, loop); T, M and F have no effect')


class _Graph:
    """undirected graph with networkx's iteration order: nodes in insertion order, components in order of their first node"""

    def __init__(self):
        self.adj = {}

    def add_edge(self, u, v):
        if u not in self.adj:
            self.adj[u] = {}
        if v not in self.adj:
            self.adj[v] = {}
        self.adj[u][v] = 1
        self.adj[v][u] = 1

    @classmethod
    def from_pairs(cls, pairs):
        """the graph after `add_edge(u, v)` for every (u, v) of `pairs` in order, built column-wise: a node's place is its first
        appearance in the sequence u0, v0, u1, v1, ...; its neighbour dict holds the other ends of its edges in that same order
        (a repeated edge keeps its first place, as a repeated assignment does)"""
        g = cls()
        if isinstance(pairs, tuple) and len(pairs) == 2 and isinstance(pairs[0], np.ndarray):
            e = np.stack(pairs, axis=1)        # (u column, v column)
        else:
            e = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        if not len(e):
            return g
        src = e.reshape(-1)                    # u0, v0, u1, v1, ...
        dst = e[:, ::-1].reshape(-1)           # v0, u0, v1, u1, ...
        order = np.argsort(src, kind='stable')
        s_sorted = src[order]
        starts = np.flatnonzero(np.r_[True, s_sorted[1:] != s_sorted[:-1]])
        ends = np.r_[starts[1:], len(src)]
        first = order[starts]                  # a node's first position in the sequence
        d_sorted = dst[order].tolist()
        nodes = s_sorted[starts].tolist()
        for k in np.argsort(first, kind='stable').tolist():
            g.adj[nodes[k]] = dict.fromkeys(d_sorted[starts[k]:ends[k]], 1)
        return g

    def components(self):
        seen = set()
        for s in self.adj:
            if s in seen:
                continue
            comp, frontier = {s}, [s]
            seen.add(s)
            while frontier:
                nxt = []
                for u in frontier:
                    for v in self.adj[u]:
                        if v not in seen:
                            seen.add(v)
                            comp.add(v)
                            nxt.append(v)
                frontier = nxt
            yield comp


def _rows(lines):
    for i in lines:
        j = i[:-1].split('\t')
        if len(j) == 4:
            x, y, z = j[1:4]
        else:
            x, y, z = j[:3]
        if x > y:
            continue
        yield x, y, z


def block_matrix(edge_lines):
    """The matrix mcl_xyz (find_cluster.py:1425-1467) hands to the Markov loop, built columnar: genes numbered by first appearance over
    ALL lines of the batch, rows with x <= y only, (x, y) and (y, x) carry the weight of the pair's LAST line, the diagonal the largest
    incident weight, weights in float32, explicit zeros not stored; (D + 1) x (D + 1) with an empty last row, canonical CSR (columns
    ascending).  -> (gene names by number, indptr int64, indices int32, data float32)"""
    cols = [l.split('\t', 3)[:3] for l in edge_lines]
    xs = np.array([c[0] for c in cols], dtype=object)
    ys = np.array([c[1] for c in cols], dtype=object)
    inter = np.empty(2 * len(cols), dtype=object)
    inter[0::2], inter[1::2] = xs, ys
    names = list(dict.fromkeys(inter.tolist()))            # numbering in order of first appearance
    number = {g: k for k, g in enumerate(names)}
    dmx = len(names) + 1
    use = np.array([c[0] <= c[1] for c in cols], dtype=bool)
    X = np.fromiter((number[g] for g in xs[use].tolist()), dtype=np.int64, count=int(use.sum()))
    Y = np.fromiter((number[g] for g in ys[use].tolist()), dtype=np.int64, count=int(use.sum()))
    Z = np.array([float(c[2]) for c, u in zip(cols, use.tolist()) if u], dtype=np.float64).astype(np.float32)
    return names, *_matrix_from_numbers(X, Y, Z, dmx)


def block_matrix_arrays(gx, gy, z, gene_names):
    """block_matrix for rows that are already columns: gx / gy = gene numbers (any integer labelling) of the batch's rows in batch order
    (every row has x <= y), z = their weights (float64); genes are renumbered by first appearance over the batch (x before y)."""
    seq = np.empty(2 * len(gx), dtype=np.int64)
    seq[0::2], seq[1::2] = gx, gy
    vals, first = np.unique(seq, return_index=True)
    order = np.argsort(first, kind='stable')
    rank = np.empty(len(vals), dtype=np.int64)
    rank[order] = np.arange(len(vals))
    X, Y = rank[np.searchsorted(vals, gx)], rank[np.searchsorted(vals, gy)]
    names = [gene_names[g] for g in vals[order].tolist()]
    return names, *_matrix_from_numbers(X, Y, np.asarray(z, dtype=np.float64).astype(np.float32), len(names) + 1)


def _matrix_from_numbers(X, Y, Z, dmx):
    if np.any(X == Y):
        return _block_matrix_sequential(X, Y, Z, dmx)   # self loops overwrite the diagonal in line order: rare, done one by one
    # off-diagonal: the last line of a pair wins
    key = X * dmx + Y
    last = len(key) - 1 - np.unique(key[::-1], return_index=True)[1]
    px, py, pz = X[last], Y[last], Z[last]
    # diagonal: the largest weight seen at either end (a zero start: weights <= 0 never set it)
    diag = np.zeros(dmx, dtype=np.float32)
    np.maximum.at(diag, X, Z)
    np.maximum.at(diag, Y, Z)
    dn = np.flatnonzero(diag > 0)
    r = np.concatenate([px, py, dn])
    c = np.concatenate([py, px, dn])
    v = np.concatenate([pz, pz, diag[dn]])
    keep = v != 0
    r, c, v = r[keep], c[keep], v[keep]
    o = np.lexsort((c, r))
    r, c, v = r[o], c[o], v[o]
    indptr = np.zeros(dmx + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=dmx), out=indptr[1:])
    return indptr, c.astype(np.int32), v.astype(np.float32)


def _block_matrix_sequential(X, Y, Z, dmx):
    cell = {}
    zero = np.float32(0)
    for a, b, z in zip(X.tolist(), Y.tolist(), Z):
        cell[(a, b)] = z
        cell[(b, a)] = z
        if cell.get((a, a), zero) < z:
            cell[(a, a)] = z
        if cell.get((b, b), zero) < z:
            cell[(b, b)] = z
    keys = sorted(k for k, v in cell.items() if v != 0)
    r = np.array([k[0] for k in keys], dtype=np.int64)
    indptr = np.zeros(dmx + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=dmx), out=indptr[1:])
    return indptr, np.array([k[1] for k in keys], dtype=np.int32), np.array([cell[k] for k in keys], dtype=np.float32)


def device_mcl(indptr, indices, data, inflation, device=0, rounds=100, check=5, prune=1e-5, rtol=1e-5, atol=1e-8, info=None):
    """the Markov loop on the GPU (libsohit so_mcl, csrc/mcl.hip) -> the final matrix as (indptr, indices, data) in the reference's
    storage order, stored zeros included.  `rounds`, `check`, `prune`, `rtol`, `atol`: the reference's own values by default (at most
    100 rounds, convergence test every 5th, pruning below 1e-5); `info`: a dict that receives `rounds` (rounds begun) and `converged`
    (0 / 1).  No CPU path: raises when the HIP library or a device is missing."""
    import ctypes as C
    from . import _lib
    L = _lib.load()
    res = _lib.SoMclResult()
    ip = np.ascontiguousarray(indptr, dtype=np.int64)
    ix = np.ascontiguousarray(indices, dtype=np.int32)
    dv = np.ascontiguousarray(data, dtype=np.float32)
    rc = L.so_mcl(device, len(ip) - 1, ip.ctypes.data, ix.ctypes.data if len(ix) else None, dv.ctypes.data if len(dv) else None, float(inflation), int(rounds), int(check),
                  float(prune), float(rtol), float(atol), C.byref(res))
    if rc != 0:
        raise RuntimeError(L.so_mcl_last_error().decode())
    try:
        n, nnz = int(res.n), int(res.nnz)
        if isinstance(info, dict):
            info.update(rounds=int(res.rounds), converged=int(res.converged))
        out_ip = _lib.result_array(res.indptr, n + 1)
        out_ix = _lib.result_array(res.indices, nnz)
        out_dv = _lib.result_array(res.data, nnz)
    finally:
        L.so_mcl_free(C.byref(res))
    return out_ip, out_ix, out_dv


def device_mcl_rows(gx, gy, z, n_labels, inflation, device=0, rounds=100, check=5, prune=1e-5, rtol=1e-5, atol=1e-8, want_matrix=False, info=None):
    """one batch from its rows to its surviving pairs on the GPU (libsohit so_mcl_rows, csrc/mcl.hip): block_matrix_arrays, the loop of
    device_mcl and surviving_pair_columns without the matrix ever existing on the host.  gx / gy: gene labels in 0 .. n_labels - 1 of the
    batch's rows in batch order, z: their float64 weights.  -> (gene, pair_r, pair_c), all int64: gene[k] = the label of matrix row k, the
    pairs in read-out order over matrix rows; with `want_matrix` also (indptr, indices, data), the matrix as it entered the loop.
    `rounds` = 0 skips the loop.  `info`: a dict that receives `rounds` and `converged`.  A NaN weight, a row with x == y, a label outside
    its range and a batch that holds both (a, b) and (b, a) are refused (RuntimeError).  No CPU path: raises when the HIP library or a
    device is missing."""
    import ctypes as C
    from . import _lib
    L = _lib.load()
    res = _lib.SoMclRowsResult()
    xi = np.ascontiguousarray(gx, dtype=np.int64)
    yi = np.ascontiguousarray(gy, dtype=np.int64)
    zv = np.ascontiguousarray(z, dtype=np.float64)
    if not (len(xi) == len(yi) == len(zv)):
        raise ValueError('device_mcl_rows: gx, gy and z differ in length')
    nr = len(xi)
    rc = L.so_mcl_rows(device, int(n_labels), nr, xi.ctypes.data if nr else None, yi.ctypes.data if nr else None, zv.ctypes.data if nr else None, float(inflation),
                       int(rounds), int(check), float(prune), float(rtol), float(atol), 1 if want_matrix else 0, C.byref(res))
    if rc != 0:
        raise RuntimeError(L.so_mcl_last_error().decode())
    try:
        d, npair, nnz = int(res.n_genes), int(res.n_pairs), int(res.nnz)
        if isinstance(info, dict):
            info.update(rounds=int(res.rounds), converged=int(res.converged))
        arr = _lib.result_array
        out = (arr(res.gene, d), arr(res.pair_r, npair), arr(res.pair_c, npair))
        if want_matrix:
            out += (arr(res.indptr, d + 2), arr(res.indices, nnz), arr(res.data, nnz))
    finally:
        L.so_mcl_rows_free(C.byref(res))
    return out


def device_readout(indptr, indices, data, prune=1e-5, device=0):
    """surviving_pair_columns on the GPU (libsohit so_mcl_readout: the read-out kernels of device_mcl_rows alone, on a host matrix)"""
    import ctypes as C
    from . import _lib
    L = _lib.load()
    res = _lib.SoMclRowsResult()
    ip = np.ascontiguousarray(indptr, dtype=np.int64)
    ix = np.ascontiguousarray(indices, dtype=np.int32)
    dv = np.ascontiguousarray(data, dtype=np.float32)
    if len(ip) < 1 or len(ix) != len(dv):
        raise ValueError('device_readout: not a CSR matrix')
    rc = L.so_mcl_readout(device, len(ip) - 1, ip.ctypes.data, ix.ctypes.data if len(ix) else None, dv.ctypes.data if len(dv) else None, float(prune), C.byref(res))
    if rc != 0:
        raise RuntimeError(L.so_mcl_last_error().decode())
    try:
        npair = int(res.n_pairs)
        r = _lib.result_array(res.pair_r, npair)
        c = _lib.result_array(res.pair_c, npair)
    finally:
        L.so_mcl_rows_free(C.byref(res))
    return r, c


def surviving_pairs(indptr, indices, data, prune=1e-5):
    """The reference's read-out of the final matrix (find_cluster.py:686-689): the coordinates of the entries that are not zero, paired
    IN ORDER with the raw data array -- which still holds the pruned zeros when the loop ran out of rounds, so the pairing can be
    shifted -- and kept where that value exceeds the threshold."""
    r, c = surviving_pair_columns(indptr, indices, data, prune)
    return list(zip(r.tolist(), c.tolist()))


def surviving_pair_columns(indptr, indices, data, prune=1e-5):
    """surviving_pairs as two arrays"""
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    nz = data != 0
    r, c = rows[nz], indices[nz]
    keep = data[:len(r)] > np.float32(prune)
    return r[keep].astype(np.int64), c[keep].astype(np.int64)


def mcl_block(edge_lines, inflation, mcl=device_mcl):
    """one batch of edges -> groups (lists of gene ids) in the reference's order"""
    names, indptr, indices, data = block_matrix(edge_lines)
    g = _Graph.from_pairs(surviving_pair_columns(*mcl(indptr, indices, data, inflation)))
    for comp in g.components():
        yield [names[e] for e in comp]


def mcl_block_arrays(gx, gy, z, gene_names, inflation, mcl=device_mcl):
    """mcl_block for a batch given as columns (see block_matrix_arrays)"""
    if len(gx) == 0:
        return
    names, indptr, indices, data = block_matrix_arrays(gx, gy, z, gene_names)
    g = _Graph.from_pairs(surviving_pair_columns(*mcl(indptr, indices, data, inflation)))
    for comp in g.components():
        yield [names[e] for e in comp]


def _device_block(gx, gy, z, n_labels, inflation):
    """cnc's batch with `device_stage='matrix'`: (device_mcl_rows is looked up per call)"""
    return device_mcl_rows(gx, gy, z, n_labels, inflation)


def mcl_block_rows(gx, gy, z, gene_names, inflation, mcl=device_mcl, block=_device_block):
    """mcl_block_arrays with the batch handed to `block` as rows: (gx, gy, z, number of labels, inflation) -> (gene labels in matrix
    order, pair_r, pair_c).  What the device call refuses -- a NaN weight, a self pair -- is a batch for mcl_block_arrays and `mcl`."""
    if len(gx) == 0:
        return
    if np.isnan(z).any() or np.any(gx == gy):
        yield from mcl_block_arrays(gx, gy, z, gene_names, inflation, mcl)
        return
    gene, pair_r, pair_c = block(gx, gy, z, len(gene_names), inflation)
    names = [gene_names[g] for g in np.asarray(gene).tolist()]
    g = _Graph.from_pairs((np.asarray(pair_r, dtype=np.int64), np.asarray(pair_c, dtype=np.int64)))
    for comp in g.components():
        yield [names[e] for e in comp]


def _component_labels(n, u, v):
    """connected components of an undirected graph on nodes 0 .. n-1: label = smallest node of the component (min-label propagation
    with pointer jumping)"""
    lab = np.arange(n, dtype=np.int64)
    if len(u) == 0:
        return lab
    while True:
        new = lab.copy()
        m = np.minimum(lab[u], lab[v])
        np.minimum.at(new, u, m)
        np.minimum.at(new, v, m)
        while True:
            nn = new[new]
            if np.array_equal(nn, new):
                break
            new = nn
        if np.array_equal(new, lab):
            return lab
        lab = new


def _numbered_components(pairs_u, pairs_v):
    """what `for flag, comp in enumerate(connected_components(G))` assigns after `G.add_edge(u, v)` for the pairs in order: nodes are
    known in order of first appearance (u before v), components are numbered in order of their first node.
    -> (node values in insertion order, component number of each of them)"""
    seq = np.empty(2 * len(pairs_u), dtype=np.int64)
    seq[0::2], seq[1::2] = pairs_u, pairs_v
    vals, first = np.unique(seq, return_index=True)
    order = np.argsort(first, kind='stable')
    nodes = vals[order]                                  # insertion order
    rank = np.empty(len(vals), dtype=np.int64)
    rank[order] = np.arange(len(vals))
    iu, iv = rank[np.searchsorted(vals, pairs_u)], rank[np.searchsorted(vals, pairs_v)]
    lab = _component_labels(len(nodes), iu, iv)
    roots = np.unique(lab)                               # ascending first node = discovery order
    return nodes, np.searchsorted(roots, lab)


def _edge_columns_native(data):
    """relation rows of a byte buffer through libsohit's tokeniser (so_tsv_*): -> (ids sorted bytewise, code of x, code of y, weight,
    weight text) of every row, or None when the library is missing, the input is tiny or a row is not what the fast path handles (the
    Python loop then decides, and raises what the reference would raise)"""
    import os
    n = data.count(b'\n')
    if n < int(os.environ.get('SOHIT_TSV_MIN', '4096')) or os.environ.get('SOHIT_TSV_NATIVE', '1') == '0':
        return None
    try:
        from . import _lib
        L = _lib.load()
    except Exception:
        return None
    import ctypes as C
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    buf = np.frombuffer(data, dtype=np.uint8)
    ls = np.empty(n + 1, dtype=np.int64)
    if L.so_tsv_lines(ptr(buf), len(data), ptr(ls), n + 1) != n:
        return None
    cols = np.array([0, 1, 2, 3, 2, 3], dtype=np.int32)
    numeric = np.array([0, 0, 0, 0, 1, 1], dtype=np.uint8)
    ntab = np.empty(n, dtype=np.int32)
    beg = np.empty((6, n), dtype=np.int64)
    ln = np.empty((6, n), dtype=np.int32)
    val = np.empty((6, n), dtype=np.float64)
    st = np.empty((6, n), dtype=np.uint8)
    if L.so_tsv_scan(ptr(buf), len(data), ptr(ls), n, 6, ptr(cols), ptr(numeric), ptr(ntab), ptr(beg), ptr(ln), ptr(val), ptr(st)) != 0:
        return None
    if np.any(ntab < 2):
        return None
    four = ntab == 3                                # `len(j) == 4`: a relation type in front of (x, y, weight)
    pick = lambda a, b: np.ascontiguousarray(np.where(four, a, b))
    xb, xl = pick(beg[1], beg[0]), pick(ln[1], ln[0])
    yb, yl = pick(beg[2], beg[1]), pick(ln[2], ln[1])
    zb, zl = pick(beg[3], beg[2]), pick(ln[3], ln[2])
    z, zs = pick(val[5], val[4]), pick(st[5], st[4])
    cx = np.empty(n, dtype=np.int64)
    cy = np.empty(n, dtype=np.int64)
    nb = np.empty(2 * n, dtype=np.int64)
    nlen = np.empty(2 * n, dtype=np.int32)
    nd = L.so_tsv_codes(ptr(buf), n, ptr(xb), ptr(xl), ptr(yb), ptr(yl), ptr(cx), ptr(cy), ptr(nb), ptr(nlen), 2 * n)
    if nd <= 0:
        return None
    use = cx <= cy                                  # `if x > y: continue` (ids compare like their bytes)
    if np.any(zs[use] != 0):
        return None                                 # a weight only Python's float() can judge
    names = [data[b:b + l].decode('utf-8') for b, l in zip(nb[:nd].tolist(), nlen[:nd].tolist())]
    u = np.flatnonzero(use)
    zb, zl = zb[u], zl[u]
    ztext = lambda i: data[int(zb[i]):int(zb[i]) + int(zl[i])]
    return names, cx[u], cy[u], z[u], ztext


def _text_bytes(lines):
    """an open file or a byte string as the bytes the reference's line loop sees; None for an iterable of lines"""
    if hasattr(lines, 'read'):
        data = lines.buffer.read() if hasattr(lines, 'buffer') else lines.read()
    elif isinstance(lines, (bytes, bytearray)):
        data = bytes(lines)
    else:
        return None
    if isinstance(data, str):
        data = data.encode('utf-8')
    data = data.replace(b'\r\n', b'\n').replace(b'\r', b'\n')   # the reference reads in text mode (universal newlines)
    if data and not data.endswith(b'\n'):
        data = data[:-1] + b'\n'                                # ... and cuts the last character of every line, newline or not
    return data


def _edge_columns(lines):
    """relation rows ('[type\\t]x\\ty\\tweight\\n') -> (ids sorted bytewise, code of x, code of y, weight, weight text of row i) for the
    rows with x <= y, in file order"""
    data = _text_bytes(lines)
    if data is not None:
        cols = _edge_columns_native(data)
        if cols is not None:
            return cols
        lines = data.decode('utf-8').splitlines(True)
    rows = [r for r in _rows(lines)]
    xs, ys, zs = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    both = np.array([g.encode('utf-8') for g in xs + ys], dtype=np.bytes_) if rows else np.zeros(0, dtype='S1')
    names, inv = np.unique(both, return_inverse=True)
    inv = inv.astype(np.int64)
    z = np.array([float(t) for t in zs], dtype=np.float64)
    return [g.decode('utf-8') for g in names.tolist()], inv[:len(rows)], inv[len(rows):], z, (lambda i: zs[i].encode('utf-8'))


def group_numbers(X, Y, Z, n):
    """The component stage of cnc (1470-1590) -- the DEFINITION the device stage (so_cnc_groups, csrc/cnc.hip) is pinned to.  X, Y: gene
    numbers of the rows with x <= y in file order, genes numbered 0 .. n-1 by first appearance (x of a row before its y), Z: their float64
    weights.  -> (comp1, grp), int64[n]: a gene's level-1 component number and its level-2 group number (-1: in no level-2 group)."""
    nrow = len(X)
    if nrow == 0:                                         # (cnc never gets here without a row)
        return np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    # level 1: every gene linked to its best-scoring neighbour(s); the dictionary is emptied last gene first, a gene's ties in file order
    best = np.full(n, -np.inf)
    np.maximum.at(best, X, Z)
    np.maximum.at(best, Y, Z)
    a = np.concatenate([X, Y])
    b = np.concatenate([Y, X])
    ridx = np.concatenate([np.arange(nrow) * 2, np.arange(nrow) * 2 + 1])   # (x, y) of a row before its (y, x)
    tie = np.concatenate([Z, Z]) == best[a]
    a, b, ridx = a[tie], b[tie], ridx[tie]
    o = np.lexsort((ridx, -a))
    genes1, comp1_of_node = _numbered_components(a[o], b[o])
    comp1 = np.zeros(n, dtype=np.int64)
    comp1[genes1] = comp1_of_node
    # level 2: components joined by an edge -- seen only when BOTH component numbers are non-zero
    cX, cY = comp1[X], comp1[Y]
    m = (cX != 0) & (cY != 0)
    k0, k1 = np.minimum(cX[m], cY[m]), np.maximum(cX[m], cY[m])
    nc = int(comp1.max()) + 2
    key = k0 * nc + k1
    _, first = np.unique(key, return_index=True)
    first.sort()
    nodes2, comp2_of_node = _numbered_components(k0[first], k1[first])
    group_of_comp = np.full(nc, -1, dtype=np.int64)
    group_of_comp[nodes2] = comp2_of_node
    grp = group_of_comp[comp1]
    return comp1, grp


def device_group_numbers(X, Y, Z, n, device=0, info=None):
    """group_numbers on the GPU (libsohit so_cnc_groups, csrc/cnc.hip) -> (comp1 int64[n], grp int64[n], keep bool[rows]); keep[i] =
    grp[X[i]] == grp[Y[i]] != 0, the rows cnc hands on.  `info`: a dict that receives n_comp1, n_grp, n_keep, sweeps1 and sweeps2 (the
    label sweeps of the two levels, the confirming one included).  A NaN weight, a gene number outside 0 .. n-1 and a gene without a
    row are refused.  No CPU path: raises when the HIP library or a device is missing."""
    import ctypes as C
    from . import _lib
    L = _lib.load()
    res = _lib.SoCncResult()
    xi = np.ascontiguousarray(X, dtype=np.int64)
    yi = np.ascontiguousarray(Y, dtype=np.int64)
    zv = np.ascontiguousarray(Z, dtype=np.float64)
    if not (len(xi) == len(yi) == len(zv)):
        raise ValueError('device_group_numbers: X, Y and Z differ in length')
    for v in (xi, yi):
        if len(v) and (int(v.min()) < -2 ** 31 or int(v.max()) >= 2 ** 31):
            raise RuntimeError('so_cnc_groups: a gene number does not fit 32 bits')
    xi, yi = xi.astype(np.int32), yi.astype(np.int32)
    nr = len(xi)
    rc = L.so_cnc_groups(device, int(n), nr, xi.ctypes.data if nr else None, yi.ctypes.data if nr else None, zv.ctypes.data if nr else None, C.byref(res))
    if rc != 0:
        raise RuntimeError(L.so_cnc_last_error().decode())
    try:
        d = int(res.n_genes)
        if isinstance(info, dict):
            info.update(n_comp1=int(res.n_comp1), n_grp=int(res.n_grp), n_keep=int(res.n_keep), sweeps1=int(res.sweeps1), sweeps2=int(res.sweeps2))
        comp1 = _lib.result_array(res.comp1, d)
        grp = _lib.result_array(res.grp, d)
        keep = _lib.result_array(res.keep, nr, bool)
    finally:
        L.so_cnc_free(C.byref(res))
    return comp1, grp, keep


def _device_stage(X, Y, Z, n):
    """cnc's component stage with `device_stage=True`: a NaN weight has no place in the device's integer order, and numpy's answer to
    it is what the bytes hang on: such an input keeps the numpy stage"""
    if np.isnan(Z).any():
        return group_numbers(X, Y, Z, n)
    return device_group_numbers(X, Y, Z, n)


class RowPlan:
    """What cnc knows of its rows before the batches (row_plan() is the definition, device_row_plan() the same from the GPU); all int64.
    gene_code[n_genes]: the id codes in order of first appearance (the x of a row before its y); X, Y[rows]: the rows' gene numbers;
    comp1, grp[n_genes]: as group_numbers() gives them; order[n_keep]: the kept rows (grp[X] == grp[Y] != 0) sorted by (grp as a signed
    number, cx, cy), rows with an equal triple in file order; cut: the positions p >= 1 of `order` whose grp differs from that of p - 1;
    tied: the positions p >= 1 whose (grp, cx, cy) equals that of p - 1."""
    FIELDS = ('gene_code', 'X', 'Y', 'comp1', 'grp', 'order', 'cut', 'tied')

    def __init__(self, gene_code, X, Y, comp1, grp, order, cut, tied):
        self.gene_code, self.X, self.Y, self.comp1, self.grp, self.order, self.cut, self.tied = gene_code, X, Y, comp1, grp, order, cut, tied

    @classmethod
    def empty(cls):
        return cls(*[np.zeros(0, dtype=np.int64) for _ in cls.FIELDS])


def row_plan(cx, cy, Z, n_codes, groups=None):
    """The front of cnc between the rows and the batches -- the DEFINITION the device plan (so_cnc_plan, csrc/cnc.hip) is pinned to.
    cx, cy: id codes of the rows with x <= y in file order (code order = the byte order of the ids), Z: their float64 weights, n_codes:
    the number of codes (it may exceed the number that occur).  `groups`: the component stage, (X, Y, Z, n) -> (comp1, grp) or
    (comp1, grp, keep flag per row); group_numbers by default.  -> RowPlan"""
    cx, cy = np.asarray(cx, dtype=np.int64), np.asarray(cy, dtype=np.int64)
    nrow = len(cx)
    if nrow == 0:
        return RowPlan.empty()
    # genes numbered by first appearance (x of a row before its y)
    seq = np.empty(2 * nrow, dtype=np.int64)
    seq[0::2], seq[1::2] = cx, cy
    vals, first = np.unique(seq, return_index=True)
    gene_code = vals[np.argsort(first, kind='stable')]
    number_of_code = np.zeros(int(n_codes), dtype=np.int64)
    number_of_code[gene_code] = np.arange(len(vals))
    X, Y = number_of_code[cx], number_of_code[cy]
    res = (groups if groups is not None else group_numbers)(X, Y, Z, len(vals))
    comp1, grp = np.asarray(res[0], dtype=np.int64), np.asarray(res[1], dtype=np.int64)
    # edges inside one level-2 group whose number is non-zero (-1, the pool of unmerged components, included)
    gx, gy = grp[X], grp[Y]
    keep = np.flatnonzero(res[2]) if len(res) > 2 else np.flatnonzero((gx != 0) & (gy != 0) & (gx == gy))
    # LC_ALL=C sort -n of the lines 'group\tx\ty\tweight': the leading number, then the whole line bytewise = (x, y, weight text)
    # bytewise (ids hold no byte below the tab, so a shorter id sorts before its extensions, like its code does)
    kg, kx, ky = gx[keep], cx[keep], cy[keep]
    o = np.lexsort((ky, kx, kg))
    sg, sx, sy = kg[o], kx[o], ky[o]
    new_grp = sg[1:] != sg[:-1]
    cut = np.flatnonzero(new_grp) + 1
    tied = np.flatnonzero(~new_grp & (sx[1:] == sx[:-1]) & (sy[1:] == sy[:-1])) + 1
    return RowPlan(gene_code, X, Y, comp1, grp, keep[o], cut, tied)


def device_row_plan(cx, cy, Z, n_codes, device=0, info=None, two_pass=False):
    """row_plan on the GPU (libsohit so_cnc_plan, csrc/cnc.hip): one device call from the code columns to every field of RowPlan.
    `two_pass`: the order by two stable sort passes, (cx, cy) then the group, also where one 64-bit key would do.  `info`: a dict that
    receives n_genes, n_comp1, n_grp, n_keep, sweeps1, sweeps2, sort_passes and waits (host waits of the call).  A NaN weight, a code
    outside 0 .. n_codes - 1 and a row with cx > cy are refused (RuntimeError).  No CPU path: raises when the HIP library or a device
    is missing."""
    import ctypes as C
    from . import _lib
    L = _lib.load()
    res = _lib.SoCncPlanResult()
    xi = np.ascontiguousarray(cx, dtype=np.int64)
    yi = np.ascontiguousarray(cy, dtype=np.int64)
    zv = np.ascontiguousarray(Z, dtype=np.float64)
    if not (len(xi) == len(yi) == len(zv)):
        raise ValueError('device_row_plan: cx, cy and Z differ in length')
    for v in (xi, yi):
        if len(v) and (int(v.min()) < -2 ** 31 or int(v.max()) >= 2 ** 31):
            raise RuntimeError('so_cnc_plan: a code does not fit 32 bits')
    xi, yi = xi.astype(np.int32), yi.astype(np.int32)
    nr = len(xi)
    rc = L.so_cnc_plan(device, int(n_codes), nr, xi.ctypes.data if nr else None, yi.ctypes.data if nr else None, zv.ctypes.data if nr else None,
                       1 if two_pass else 0, C.byref(res))
    if rc != 0:
        raise RuntimeError(L.so_cnc_last_error().decode())
    try:
        if isinstance(info, dict):
            info.update({k: int(getattr(res, k)) for k in ('n_genes', 'n_comp1', 'n_grp', 'n_keep', 'sweeps1', 'sweeps2', 'sort_passes', 'waits')})
        col = lambda p, n: _lib.result_array(p, n, np.int64)
        d, k = int(res.n_genes), int(res.n_keep)
        plan = RowPlan(col(res.gene_code, d), col(res.x, nr), col(res.y, nr), col(res.comp1, d), col(res.grp, d), col(res.order, k),
                       col(res.cut, int(res.n_cut)), col(res.tied, int(res.n_tied)))
    finally:
        L.so_cnc_plan_free(C.byref(res))
    return plan


def _device_plan(cx, cy, Z, n_codes):
    """cnc's plan with `device_stage='all'`: an input with a NaN weight keeps the numpy plan, as _device_stage keeps the numpy stage"""
    if np.isnan(Z).any():
        return row_plan(cx, cy, Z, n_codes)
    return device_row_plan(cx, cy, Z, n_codes)


def cnc(lines, inflation=1.5, chk=10 ** 7, mcl=device_mcl, groups=None, device_stage=False, block=None):
    """cnc (1470-1673): relation rows -> groups (lists of gene ids), in the reference's output order.  `lines`: an open file, bytes or an
    iterable of lines.  `mcl`: the Markov loop on a CSR block (the device implementation; the tests pass the scipy oracle to check this host
    bookkeeping on CPU).  `groups`: the component stage, (X, Y, Z, n) -> (comp1, grp) or (comp1, grp, keep flag per row): group_numbers by
    default, the device stage (device_group_numbers; the numpy one when a weight is NaN) with `device_stage=True`.
    `device_stage='matrix'`: the device stage, and every batch goes from its rows to its surviving pairs in one device call (`block`:
    (gx, gy, z, number of labels, inflation) -> (gene labels in matrix order, pair_r, pair_c); device_mcl_rows by default, the tests plug in
    a numpy restatement) -- but for a batch with a NaN weight or a self pair, which keeps the host matrix and `mcl`.
    `device_stage='all'`: as 'matrix', and the whole plan in front of the batches -- gene numbers, component stage, kept rows, their order,
    the cuts -- comes from one device call (device_row_plan; the numpy plan when a weight is NaN or `groups` is given).
    The reference keeps Python dictionaries and networkx graphs and moves the edges between its stages as sorted text files; here the
    rows are columns from the start (ids coded by their byte order, which is also the order `sort` compares them in), genes are integers
    numbered by first appearance (the insertion order of the reference's best-neighbour dictionary), and each of its orders --
    `popitem()` = last gene first, a graph's node order = first appearance in the `add_edge` sequence, components numbered by their
    first node, `LC_ALL=C sort -n` of the group-tagged edge lines -- is reproduced as index arithmetic (row_plan)."""
    names, cx, cy, Z, ztext = _edge_columns(lines)
    return cnc_columns(names, cx, cy, Z, ztext, inflation, chk, mcl, groups, device_stage, block)


def cnc_columns(names, cx, cy, Z, ztext, inflation=1.5, chk=10 ** 7, mcl=device_mcl, groups=None, device_stage=False, block=None, plan=None):
    """cnc behind its tokeniser: rows that are columns already -> groups.  names: the ids by code (code order = their byte order); cx, cy:
    the codes of the rows with x <= y in file order; Z: their float64 weights; ztext(i): the weight of row i as the bytes a file would
    hold (asked for only where one pair occurs twice in a group: those lines are ordered by that text).  `plan`: (cx, cy, Z, number of
    codes) -> RowPlan, instead of what `groups` and `device_stage` select.  The other arguments: see cnc."""
    if len(cx) == 0:
        return []
    if plan is not None:
        P = plan(cx, cy, Z, len(names))
    elif device_stage == 'all' and groups is None:
        P = _device_plan(cx, cy, Z, len(names))
    else:
        P = row_plan(cx, cy, Z, len(names), groups if groups is not None else (_device_stage if device_stage else group_numbers))
    X, Y = P.X, P.Y
    if len(P.order) == 0:
        return []
    gene_names = [names[c] for c in P.gene_code.tolist()]
    rows_sorted = P.order.copy()
    if len(P.tied):                                       # the same pair twice in a group: its lines are ordered by the weight's text
        first = np.concatenate([[True], np.diff(P.tied) > 1])
        last = np.concatenate([first[1:], [True]])
        for s0, e0 in zip((P.tied[first] - 1).tolist(), (P.tied[last] + 1).tolist()):
            seg = rows_sorted[s0:e0].tolist()
            seg.sort(key=lambda r: ztext(int(r)) + b'\n')
            rows_sorted[s0:e0] = seg
    # batches: a new one starts where the group changes once the running batch holds more than chk rows
    if device_stage in ('matrix', 'all') or block is not None:
        batch = lambda r: mcl_block_rows(X[r], Y[r], Z[r], gene_names, inflation, mcl, block if block is not None else _device_block)
    else:
        batch = lambda r: mcl_block_arrays(X[r], Y[r], Z[r], gene_names, inflation, mcl)
    out, start = [], 0
    for c in P.cut.tolist():
        if c - start > chk:
            out.extend(batch(rows_sorted[start:c]))
            start = c
    out.extend(batch(rows_sorted[start:]))
    return out


def groups_from_tables(names, tables, inflation=1.5, device_stage=False, chk=10 ** 7, mcl=device_mcl, block=None, groups=None, plan=None):
    """find_orth's RelationTables -> ortholog groups (lists of ids, str) without the relation text: what cnc() returns for the lines
    find_orth.lines_from_tables() writes.  names: the ids by code as find_orth numbers them (np.unique: byte order); rows = the IP, OT and
    CO sections in output order, kept where a <= b; a weight is the table's value (repr round-trips: the number the tokeniser would read
    back) and its text, needed for tied runs only, repr(v).  `device_stage`, `chk`, `mcl`, `block`, `groups`, `plan`: see cnc_columns
    (a NaN value takes the numpy plan)."""
    a = np.concatenate([np.asarray(getattr(tables, k + '_a'), dtype=np.int64) for k in ('ip', 'ot', 'co')])
    b = np.concatenate([np.asarray(getattr(tables, k + '_b'), dtype=np.int64) for k in ('ip', 'ot', 'co')])
    v = np.concatenate([np.asarray(getattr(tables, k + '_v'), dtype=np.float64) for k in ('ip', 'ot', 'co')])
    use = a <= b
    cx, cy, Z = a[use], b[use], v[use]
    ids = [t.decode('utf-8') if isinstance(t, bytes) else str(t) for t in (names.tolist() if hasattr(names, 'tolist') else names)]
    return cnc_columns(ids, cx, cy, Z, (lambda i: repr(float(Z[i])).encode()), inflation, chk, mcl, groups, device_stage, block, plan)


def _apc_rows_python(lines):
    """fc2mat's line loop (find_cluster.py:779-808), literally: -> (ids by number, x numbers, y numbers, weights) of the kept rows"""
    number, xs, ys, zs = {}, [], [], []
    for i in lines:
        j = i[:-1].split('\t')
        if len(j) == 4:
            x, y, z = j[1:4]
        else:
            x, y, z = j          # (neither three nor four fields: raises, as the reference does)
        if x > y:
            continue
        if x not in number:
            number[x] = len(number)
        if y not in number:
            number[y] = len(number)
        try:
            w = float(z)
        except Exception:
            try:
                w = float(z.split('rm')[0])
            except Exception:
                continue         # (its genes stay numbered)
        xs.append(number[x]), ys.append(number[y]), zs.append(w)
    return list(number), np.array(xs, dtype=np.int64), np.array(ys, dtype=np.int64), np.array(zs, dtype=np.float64)


def _rows_have_three_or_four_fields(data):
    """every line of `data` holds two or three tabs (the tokeniser's fast path reads the first columns of a longer row, where the
    reference raises)"""
    tabs = np.frombuffer(data, dtype=np.uint8) == 9
    ends = np.flatnonzero(np.frombuffer(data, dtype=np.uint8) == 10)
    per_line = np.diff(np.concatenate([[0], np.cumsum(tabs)[ends]]))
    return bool(np.all((per_line == 2) | (per_line == 3)))


def _taxon_codes(ids):
    """ids by code -> (int32 code of `id.split('|')[0]` per id, number of distinct prefixes)"""
    number = {}
    tax = np.fromiter((number.setdefault(g.split('|')[0], len(number)) for g in ids), dtype=np.int32, count=len(ids))
    return tax, len(number)


def apc_entry_columns(cx, cy, Z, n_codes, taxon_of_code):
    """The column half of fc2mat (find_cluster.py:767-858) -- the DEFINITION the device stage (so_apc_rows, csrc/apc.hip) is pinned to.
    cx, cy: id codes of the rows with x <= y in file order (codes 0 .. n_codes - 1 in the byte order of the ids; codes may be unused),
    Z: their float64 weights, taxon_of_code[c]: an int32 code of `id.split('|')[0]`.  Genes are numbered by first appearance in cx0, cy0,
    cx1, cy1, ...; entry 2r = (X_r, Y_r, f32(z_r)), entry 2r + 1 = (Y_r, X_r, f32(z_r)), entry 2R + g = (g, g, f32(-20.0 * n_taxa_used)),
    n_taxa_used = the distinct taxon codes of the numbered genes (a taxon carried by unused codes alone does not count); f32 rounds once,
    to nearest even (overflow: an infinity; denormals kept; a NaN stays a NaN).
    -> (gene_code int64[n_genes], row int32, col int32, score float32, n_genes, n_taxa_used)"""
    cx, cy = np.asarray(cx, dtype=np.int64), np.asarray(cy, dtype=np.int64)
    Z = np.asarray(Z, dtype=np.float64)
    tax = np.asarray(taxon_of_code, dtype=np.int32)
    nrow = len(cx)
    seq = np.empty(2 * nrow, dtype=np.int64)
    seq[0::2], seq[1::2] = cx, cy
    vals, first = np.unique(seq, return_index=True)
    gene_code = vals[np.argsort(first, kind='stable')]
    n = len(gene_code)
    number_of_code = np.zeros(int(n_codes), dtype=np.int64)
    number_of_code[gene_code] = np.arange(n)
    X, Y = number_of_code[cx], number_of_code[cy]
    n_taxa_used = len(np.unique(tax[gene_code]))
    m = 2 * nrow
    row = np.empty(m + n, dtype=np.int32)
    col = np.empty(m + n, dtype=np.int32)
    score = np.empty(m + n, dtype=np.float32)
    row[0:m:2], row[1:m:2], col[0:m:2], col[1:m:2] = X, Y, Y, X
    with np.errstate(over='ignore'):
        score[0:m:2] = score[1:m:2] = Z.astype(np.float32)
    row[m:] = col[m:] = np.arange(n)
    score[m:] = np.float32(n_taxa_used * -20.)
    return gene_code, row, col, score, n, n_taxa_used


def _apc_input(lines):
    """the rows of `-a apc` as far as the tokeniser takes them: ('columns', ids by code, cx, cy, z) for plain input, ('rows', ids by
    number, X, Y, Z) from the literal loop for anything the fast path does not take (a weight only Python can judge, a row of another
    shape, a tiny input, a kept row without a weight)"""
    data = _text_bytes(lines)
    cols = None
    if data is not None:
        if _rows_have_three_or_four_fields(data):
            cols = _edge_columns_native(data)
        lines = data.decode('utf-8').splitlines(True)
    if cols is not None:
        return ('columns',) + tuple(cols[:4])
    return ('rows',) + _apc_rows_python(lines)


def _apc_entries_of_rows(names, X, Y, Z):
    """the entry list of rows the literal loop numbered: -> (ids by number, row int32, col int32, score float32, number of genes)"""
    n = len(names)
    pref = len(set(g.split('|')[0] for g in names)) * -20.
    row = np.empty(2 * len(X) + n, dtype=np.int32)
    col = np.empty(2 * len(X) + n, dtype=np.int32)
    score = np.empty(2 * len(X) + n, dtype=np.float32)
    m = 2 * len(X)
    row[0:m:2], row[1:m:2], col[0:m:2], col[1:m:2] = X, Y, Y, X
    score[0:m:2] = score[1:m:2] = Z.astype(np.float32)
    row[m:] = col[m:] = np.arange(n)
    score[m:] = np.float32(pref)
    return names, row, col, score, n


def apc_entries(lines):
    """The entry list fc2mat (find_cluster.py:767-858) writes for `-a apc`: genes numbered by first appearance over the rows with
    x <= y (x before y); per kept row (X, Y, w) then (Y, X, w); after all rows one preference entry (g, g, -20 * number of distinct
    `id.split('|')[0]`) per gene.  `lines`: an open file, bytes or an iterable of lines.  Plain input goes through libsohit's
    tokeniser, the taxon codes and apc_entry_columns; anything the tokeniser does not take (a weight only Python can judge, a row of
    another shape, a tiny input) through the literal loop.
    -> (ids by number, row int32, col int32, score float32, number of genes)"""
    inp = _apc_input(lines)
    if inp[0] == 'rows':
        return _apc_entries_of_rows(*inp[1:])
    ids, cx, cy, z = inp[1:]
    gene_code, row, col, score, n, _ = apc_entry_columns(cx, cy, z, len(ids), _taxon_codes(ids)[0])
    return [ids[c] for c in gene_code.tolist()], row, col, score, n


def device_apc(row, col, score, n_genes, damp, rounds=100, device=0):
    """the affinity-propagation loop on the GPU (libsohit so_apc, csrc/apc.hip) over the entries (row, col, score) in the reference's
    order -> (labels int64[n_genes], r float32, a float32 in entry order) after `rounds` rounds.  No CPU path: raises when the HIP
    library or a device is missing."""
    import ctypes as C
    from . import _lib
    L = _lib.load()
    res = _lib.SoApcResult()
    ri = np.ascontiguousarray(row, dtype=np.int32)
    ci = np.ascontiguousarray(col, dtype=np.int32)
    sv = np.ascontiguousarray(score, dtype=np.float32)
    if not (len(ri) == len(ci) == len(sv)):
        raise ValueError('device_apc: row, col and score differ in length')
    n = len(ri)
    rc = L.so_apc(device, int(n_genes), n, ri.ctypes.data if n else None, ci.ctypes.data if n else None, sv.ctypes.data if n else None, float(damp), int(rounds),
                  C.byref(res))
    if rc != 0:
        raise RuntimeError(L.so_apc_last_error().decode())
    try:
        d = int(res.n_genes)
        labels = _lib.result_array(res.labels, d)
        r = _lib.result_array(res.r, n)
        a = _lib.result_array(res.a, n)
    finally:
        L.so_apc_free(C.byref(res))
    return labels, r, a


def device_apc_rows(cx, cy, z, n_codes, taxon_of_code, damp, rounds=100, device=0, want_entries=False, info=None):
    """`-a apc` from id-coded rows to exemplar labels in one device call (libsohit so_apc_rows, csrc/apc.hip): apc_entry_columns and the
    loop of device_apc without the entry list ever existing on the host.  cx <= cy: id codes in 0 .. n_codes - 1 of the rows in file
    order, z: their float64 weights, taxon_of_code: an int32 taxon code per id code.  -> (gene_code int64[n_genes], labels
    int64[n_genes]); with `want_entries` also (row int32, col int32, score float32, r float32, a float32) in entry order -- R and A stay
    on the device otherwise.  `info`: a dict that receives n_genes, n_entries, n_taxa_used, rounds and waits (host waits of the call).
    A code or a taxon code out of range and a row with cx > cy are refused (RuntimeError).  No CPU path: raises when the HIP library or
    a device is missing."""
    import ctypes as C
    from . import _lib
    L = _lib.load()
    res = _lib.SoApcRowsResult()
    xi = np.ascontiguousarray(cx, dtype=np.int64)
    yi = np.ascontiguousarray(cy, dtype=np.int64)
    zv = np.ascontiguousarray(z, dtype=np.float64)
    tx = np.ascontiguousarray(taxon_of_code, dtype=np.int64)
    if not (len(xi) == len(yi) == len(zv)):
        raise ValueError('device_apc_rows: cx, cy and z differ in length')
    if len(tx) != int(n_codes) and int(n_codes) >= 0:
        raise ValueError('device_apc_rows: taxon_of_code does not hold one taxon per code')
    for v in (xi, yi, tx):
        if len(v) and (int(v.min()) < -2 ** 31 or int(v.max()) >= 2 ** 31):
            raise RuntimeError('so_apc_rows: a code does not fit 32 bits')
    xi, yi, tx = xi.astype(np.int32), yi.astype(np.int32), tx.astype(np.int32)
    nr = len(xi)
    n_taxa = int(tx.max()) + 1 if len(tx) else 0
    rc = L.so_apc_rows(device, int(n_codes), nr, xi.ctypes.data if nr else None, yi.ctypes.data if nr else None, zv.ctypes.data if nr else None,
                       tx.ctypes.data if len(tx) else None, n_taxa, float(damp), int(rounds), 1 if want_entries else 0, C.byref(res))
    if rc != 0:
        raise RuntimeError(L.so_apc_last_error().decode())
    try:
        d, n = int(res.n_genes), int(res.n_entries)
        if isinstance(info, dict):
            info.update({k: int(getattr(res, k)) for k in ('n_genes', 'n_entries', 'n_taxa_used', 'rounds', 'waits')})
        col = _lib.result_array
        out = (col(res.gene_code, d).astype(np.int64), col(res.labels, d))
        if want_entries:
            out += (col(res.row, n), col(res.col, n), col(res.score, n), col(res.r, n), col(res.a, n))
    finally:
        L.so_apc_rows_free(C.byref(res))
    return out


def _device_loop(row, col, score, n_genes, damp):
    """the command's loop: (device_apc is looked up per call)"""
    return device_apc(row, col, score, n_genes, damp)


def _device_rows(cx, cy, z, n_codes, taxon_of_code, damp):
    """the command's device stage: (device_apc_rows is looked up per call)"""
    return device_apc_rows(cx, cy, z, n_codes, taxon_of_code, damp)


def _exemplar_groups(names, labels):
    """the read-out of `-a apc`: the connected components of the graph after `add_edge(g, exemplar of g)` for the genes in number order
    (host code: the member order inside a group is Python's set order)"""
    n = len(names)
    g = _Graph.from_pairs((np.arange(n, dtype=np.int64), np.asarray(labels, dtype=np.int64)))
    return [[names[e] for e in comp] for comp in g.components()]


def apc_columns(names, cx, cy, Z, damp=0.5, device_stage=False, loop=device_apc, rows=device_apc_rows):
    """apc behind its tokeniser: rows that are columns already -> groups.  names: the ids by code (code order = their byte order); cx, cy:
    the codes of the rows with x <= y in file order; Z: their float64 weights.  With `device_stage` the rows go to the labels in one
    device call, `rows`: (cx, cy, Z, number of codes, taxon_of_code, damp) -> (gene_code, labels, ...) (device_apc_rows; the tests plug
    in a numpy restatement); otherwise through apc_entry_columns and `loop` (see apc).  Both end in the same read-out on the host."""
    if len(cx) == 0:
        return []
    tax, _ = _taxon_codes(names)
    if device_stage:
        res = rows(cx, cy, Z, len(names), tax, damp)
        gene_code, labels = np.asarray(res[0], dtype=np.int64), res[1]
    else:
        gene_code, row, col, score, n, _ = apc_entry_columns(cx, cy, Z, len(names), tax)
        labels = loop(row, col, score, n, damp)[0]
    return _exemplar_groups([names[c] for c in gene_code.tolist()], labels)


def apc_from_tables(names, tables, damp=0.5, device_stage=False, loop=device_apc, rows=device_apc_rows):
    """find_orth's RelationTables -> the groups of `-a apc` (lists of ids, str) without the relation text: what apc() returns for the lines
    find_orth.lines_from_tables() writes -- the counterpart of groups_from_tables.  names: the ids by code as find_orth numbers them
    (np.unique: byte order); rows = the IP, OT and CO sections in output order, kept where a <= b; a weight is the table's value (repr
    round-trips: the number the tokeniser would read back).  `device_stage`, `loop`, `rows`: see apc_columns."""
    a = np.concatenate([np.asarray(getattr(tables, k + '_a'), dtype=np.int64) for k in ('ip', 'ot', 'co')])
    b = np.concatenate([np.asarray(getattr(tables, k + '_b'), dtype=np.int64) for k in ('ip', 'ot', 'co')])
    v = np.concatenate([np.asarray(getattr(tables, k + '_v'), dtype=np.float64) for k in ('ip', 'ot', 'co')])
    use = a <= b
    ids = [t.decode('utf-8') if isinstance(t, bytes) else str(t) for t in (names.tolist() if hasattr(names, 'tolist') else names)]
    return apc_columns(ids, a[use], b[use], v[use], damp, device_stage, loop, rows)


def apc(lines, damp=0.5, loop=device_apc, device_stage=False, rows=device_apc_rows):
    """`-a apc` (fc2mat, apclust_blk, main 1705-1723): relation rows -> groups (lists of gene ids) in the reference's output order: the
    connected components of the graph after `add_edge(g, exemplar of g)` for the genes in number order.  `loop`: the affinity-propagation
    loop over the entry list (the device implementation; the tests pass the literal numpy oracle to check this host bookkeeping on CPU).
    `device_stage`: the rows go from their id codes to the labels in one device call (`rows`, see apc_columns) -- but for input that
    only the literal loop can judge (a weight Python alone parses, a row of another shape, fewer than SOHIT_TSV_MIN lines, a kept row
    without a weight), which keeps the host entry list and `loop`."""
    inp = _apc_input(lines)
    if inp[0] == 'columns':
        return apc_columns(*inp[1:], damp=damp, device_stage=device_stage, loop=loop, rows=rows)
    names, row, col, score, n = _apc_entries_of_rows(*inp[1:])
    if n == 0:
        return []
    return _exemplar_groups(names, loop(row, col, score, n, damp)[0])


def parse(argv):
    from .fsearch import parse_flags
    return parse_flags(argv, DEFAULTS)


def main(argv=None):
    argv = list(sys.argv if argv is None else argv)
    args = parse(argv)
    if args['-i'] == '':
        manual_print(argv[0] if argv else 'find_cluster.py')
        raise SystemExit()
    try:
        qry, ifl, alg = args['-i'], float(args['-I']), args['-a'].lower()
        dmp, bch = float(args['-d']), int(args['-b'])
        float(args['-p']), int(args['-t'])
    except Exception:
        manual_print(argv[0] if argv else 'find_cluster.py')
        raise SystemExit()
    named = any((t == '-a' and i + 2 < len(argv)) or (t[:2] == '-a' and len(t) > 2) for i, t in enumerate(argv[1:]))   # (the default is 'apc': only a named algorithm runs)
    if alg == 'apc' and named and bch > 0:
        gpu = str(args['-G']).upper()[:1] == 'A'
        run, warm_up = (lambda f: apc(f, dmp, _device_loop, gpu, _device_rows)), (lambda: device_apc([0], [0], [0.], 1, dmp, rounds=1))
    elif alg == 'mcl':
        gpu = {'T': True, 'M': 'matrix', 'A': 'all'}.get(str(args['-G']).upper()[:1], False)
        run = lambda f: cnc(f, ifl, device_stage=gpu)
        warm_up = lambda: device_mcl(np.array([0, 1]), np.array([0]), np.array([1.], dtype=np.float32), ifl, rounds=1)
    else:
        if not named:
            why = 'no algorithm named: say -a mcl or -a apc (the reference\'s default, apc, has to be asked for here)'
        elif alg == 'apc':
            why = '-a apc needs a batch size -b above 0 (the reference\'s in-place float32 variant of -b 0 is not provided; -a mcl is)'
        elif alg == 'sap':
            why = '-a sap is not provided (it needs pysapc); -a mcl and -a apc are'
        elif alg.startswith('ap'):
            why = '-a %s is not provided (the reference runs it as apc without preference entries); -a mcl and -a apc are' % args['-a']
        else:
            why = 'unknown algorithm -a %s: -a mcl and -a apc are provided' % args['-a']
        sys.stderr.write('find_cluster: %s\n' % why)
        return 2
    # the HIP runtime and the loop kernels' code object take ~0.25 s to come up: a thread brings them up on a 1 x 1 problem while
    # this one reads the edges and finds the components (failures there are left to the real call, which reports them)
    import threading

    def warm():
        try:
            warm_up()
        except Exception:
            pass
    wt = threading.Thread(target=warm, daemon=True)
    wt.start()
    try:
        with open(qry, 'r') as f:
            groups = run(f)
        w = sys.stdout.write
        for grp in groups:
            w('\t'.join(grp) + '\n')
    finally:
        wt.join(30.0)   # never leave the interpreter while the thread is inside HIP initialisation (an edge-less input ends before it)
    return 0


if __name__ == '__main__':
    if __package__ in (None, ''):
        import os
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from swiftortho_amd.find_cluster import main as _m
        sys.exit(_m())
    sys.exit(main())
