"""Inputs of the device batch call of `find_cluster -a mcl` (find_cluster.device_mcl_rows / libsohit so_mcl_rows, and device_readout /
so_mcl_readout), shared by tests/test_mcl_rows.py (CPU) and tests/test_gpu_mcl_rows.py (GPU).  No GPU here.

A batch is (gx, gy, z, n_labels): the gene labels of its rows in batch order and their float64 weights.  No batch holds a self pair,
a NaN or a pair in both orientations (the device call refuses those; refusals() lists one of each).  Every batch is at the smallest
shape where its kernel can go wrong.  The sizes are the code's own: the assembly and read-out kernels run 256 lanes a workgroup over
the rows and over the 2 x rows positions of the sequence x0, y0, x1, y1, ...; scan_u32 takes 8192 values per workgroup and changes from
one launch to three above 4 x 8192 values.  The family graph of about 20 000 rows is the only large batch.

A read-out matrix is (indptr, indices, data): any CSR, stored zeros and unsorted columns included."""
import functools

import numpy as np

import cnc_inputs as ci

LANES = 256                 # lanes per workgroup of the numbering / k_rows_* / k_ro_* kernels
SCAN_TILE = 8192            # values per workgroup of scan_u32
SCAN_ONE_LAUNCH = 4 * 8192  # scan_u32: up to here one launch, above it three


def labelled(rows, spare=0, seed=0):
    """rows (a, b, weight) over any hashable genes -> (gx, gy, z, n_labels): a gene's label is a seeded permutation of its order of
    first appearance among n + spare labels, so the matrix numbering never coincides with the labels"""
    number = {}
    for a, b, _ in rows:
        for g in (a, b):
            if g not in number:
                number[g] = len(number)
    n_labels = len(number) + spare
    perm = np.random.default_rng(1000 + seed).permutation(n_labels)
    gx = np.array([perm[number[a]] for a, _, _ in rows], dtype=np.int64)
    gy = np.array([perm[number[b]] for _, b, _ in rows], dtype=np.int64)
    return gx, gy, np.array([w for _, _, w in rows], dtype=np.float64), n_labels


def sized(n, r, seed):
    """exactly n genes and r rows (r >= (n + 1) // 2, n >= 2): rows that bring in the genes two at a time, then random pairs -- repeats
    among them -- with the smaller gene first (no pair in both orientations); weights over four decades; rows shuffled"""
    rng = np.random.default_rng(seed)
    pairs = [(g, g + 1) if g + 1 < n else (g - 1, g) for g in range(0, n, 2)]
    assert len(pairs) <= r
    while len(pairs) < r:
        a, b = rng.integers(0, n, 2).tolist()
        if a != b:
            pairs.append((min(a, b), max(a, b)))
    w = np.round(10 ** rng.uniform(-2, 2, r), 4).tolist()
    return [(pairs[i][0], pairs[i][1], w[i]) for i in rng.permutation(r).tolist()]


def repeated(times, first_line, fill=300):
    """`fill` light rows of a chain, and in their midst the pair (p, q) on `times` consecutive lines from line `first_line`, heaviest
    first: the last line wins the entry, the first one sets both diagonals"""
    rows = [(("c", i), ("c", i + 1), 0.25) for i in range(fill)]
    rep = [("p", "q", float(2 * times - k)) for k in range(times)]
    return rows[:first_line] + rep + rows[first_line:]


def hub(leaves, last):
    """a hub with `leaves` neighbours.  last: rows between the leaves come first, so the hub is the last gene (the last non-empty
    matrix row); otherwise it is gene 0"""
    rows = []
    if last:
        rows = [(("l", i), ("l", min(i + 1, leaves - 1)), 0.5) for i in range(0, leaves - 1, 2)] + [(("l", leaves - 2), ("l", leaves - 1), 0.5)]
        return rows + [(("l", i), "hub", 1.0 + i % 7) for i in range(leaves)]
    return [("hub", ("l", i), 1.0 + i % 7) for i in range(leaves)]


@functools.lru_cache(maxsize=None)
def batches():
    """name -> (gx, gy, z, n_labels), read-only; every batch also with its rows reversed (name + '_reversed')"""
    out = {"one_row": labelled([("a", "b", 2.5)])}
    for r in (LANES // 2 - 1, LANES // 2, LANES // 2 + 1, LANES - 1, LANES, LANES + 1):          # the positions' and the rows' workgroup edge
        out["rows%d" % r] = labelled(sized(40, r, r), seed=r)
    for n in (63, 64, 65, LANES - 1, LANES, LANES + 1):                                            # a wave / a workgroup of genes
        out["genes%d" % n] = labelled(sized(n, n + n // 2 + 3, n), seed=n)
    for r in (SCAN_TILE // 2, SCAN_TILE, SCAN_ONE_LAUNCH // 2, SCAN_ONE_LAUNCH):                   # scan_u32's edges, over positions and rows
        for d in (-1, 0, 1):
            out["rows%d" % (r + d)] = labelled(sized(700, r + d, r + d), seed=r + d)
    out["unused_labels"] = labelled(sized(70, 150, 5), spare=300, seed=5)
    out["first_seen_as_y"] = labelled([("a", "b", 1.0), ("a", "c", 2.0), ("d", "c", 0.5), ("a", "e", 3.0), ("f", "e", 1.5)], seed=2)
    out["repeat2_straddles_256"] = labelled(repeated(2, LANES - 1), seed=3)
    out["repeat3_straddles_256"] = labelled(repeated(3, LANES - 2), seed=4)
    out["repeat64_straddles_256"] = labelled(repeated(64, LANES - 32), seed=6)
    out["hub1025_first_row"] = labelled(hub(1025, False), seed=7)
    out["hub1025_last_row"] = labelled(hub(1025, True), seed=8)
    out["all_negative"] = labelled([(a, b, -w) for a, b, w in sized(30, 80, 9)], seed=9)
    out["all_zero_or_tiny"] = labelled([(a, b, (-0.0, 1e-50, 0.0, -1e-50)[i % 4]) for i, (a, b, w) in enumerate(sized(30, 80, 10))], seed=10)
    out["one_denormal"] = labelled([("a", "b", -0.0), ("b", "c", 1e-40), ("c", "d", 1e-50), ("a", "d", -0.0)], seed=11)
    out["overflow"] = labelled([("a", "b", 1e300), ("b", "c", -1e300), ("c", "d", 2.0), ("a", "d", 3.0), ("e", "f", -1e300), ("e", "d", 1e39), ("a", "b", 1e300)], seed=12)
    out["family"] = labelled(ci.family_graph(31, 200, 18), spare=1000, seed=13)
    for name in list(out):
        gx, gy, z, n_labels = out[name]
        out[name + "_reversed"] = (gx[::-1].copy(), gy[::-1].copy(), z[::-1].copy(), n_labels)
    for v in out.values():
        for a in v[:3]:
            a.setflags(write=False)
    return out


# batches whose Markov loop the tests run
# (not the hubs: a star of 1025 leaves squares to a dense matrix of a million entries)
LOOP_BATCHES = ("one_row", "rows255", "rows256", "rows257", "genes65", "unused_labels", "first_seen_as_y", "repeat64_straddles_256", "one_denormal",
                "all_zero_or_tiny", "all_negative", "family", "family_reversed")


def refusals():
    """name -> ((gx, gy, z, n_labels), a piece of the message, refused before a device is looked for)"""
    gx, gy, z, n_labels = batches()["first_seen_as_y"]
    at = lambda a, i, v: np.where(np.arange(len(a)) == i, v, a)
    return {"nan_weight": ((gx, gy, at(z, 3, np.nan), n_labels), "NaN", True),
            "self_pair": ((gx, at(gy, 2, gx[2]), z, n_labels), "self pair", True),
            "label_above": ((at(gx, 4, n_labels), gy, z, n_labels), "outside 0 .. n_labels - 1", True),
            "label_below": ((gx, at(gy, 0, -1), z, n_labels), "outside 0 .. n_labels - 1", True),
            "negative_labels": ((gx[:0], gy[:0], z[:0], -1), "bad arguments", True),
            "too_many_labels": ((gx[:0], gy[:0], z[:0], 2 ** 31), "2^31", True),
            "both_orientations": ((np.append(gx, gy[1]), np.append(gy, gx[1]), np.append(z, 9.0), n_labels), "(a, b) and as (b, a)", False)}


def csr(data, n, seed, last_row_empty=False):
    """the float32 values `data` as the stored entries of an n x n CSR matrix: row lengths and columns drawn at random (empty rows
    among them, columns in any order)"""
    rng = np.random.default_rng(seed)
    data = np.asarray(data, dtype=np.float32)
    rows = np.sort(rng.integers(0, n - 1 if last_row_empty else n, len(data)))
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    return indptr, rng.integers(0, n, len(data)).astype(np.int32), data


def _values(nnz, zeros, seed):
    """nnz values of which about a third lie below the threshold, zeros at the given positions"""
    rng = np.random.default_rng(seed)
    v = np.where(rng.random(nnz) < 0.33, 3e-6, rng.uniform(0.1, 1.0, nnz)).astype(np.float32)
    for p in zeros:
        if 0 <= p < nnz:
            v[p] = 0
    return v


@functools.lru_cache(maxsize=None)
def readout_matrices():
    """name -> (indptr, indices, data), read-only"""
    f = np.float32
    out = {"nnz0": csr([], 5, 0), "all_stored_zeros": csr([0.0] * 300, 40, 1), "no_zeros": csr(_values(300, (), 2), 40, 2),
           "zero_at_0": csr(_values(300, (0,), 3), 40, 3), "zero_at_last": csr(_values(300, (299,), 4), 40, 4),
           "shifted_pairing": csr([0.0, 5e-6, 1.0, 1.0], 3, 5),
           "specials": csr([np.nan, -0.0, -1.0, 1.0, np.inf, -np.inf, f(1e-5), np.nextafter(f(1e-5), f(1)), 0.0, np.nextafter(f(1e-5), f(0)), -np.nan, 1e-40, -1e-40, 0.5,
                            0.5, 0.5, 0.5, 0.5], 6, 6),
           "empty_last_row": csr(_values(50, (7, 8), 7), 9, 7, last_row_empty=True),
           "one_row": csr(_values(70, (3, 64), 8), 1, 8)}
    for edge in (LANES, 4 * LANES, SCAN_TILE, SCAN_ONE_LAUNCH):
        for d in (-1, 0, 1):
            nnz = edge + d
            out["nnz%d" % nnz] = csr(_values(nnz, (edge - 2, edge - 1, edge, 17, nnz - 1 if d == 0 else 0), nnz), 90, nnz)
    for d in (-1, 0, 1):                                     # ... and the same edge over the non-zero entries, which the second pass runs over
        nnz = LANES + d + 5
        out["nonzero%d" % (LANES + d)] = csr(_values(nnz, (0, 100, 101, 255, nnz - 1), nnz), 90, nnz)
    for v in out.values():
        for a in v:
            a.setflags(write=False)
    return out
