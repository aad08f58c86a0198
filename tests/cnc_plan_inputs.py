"""Inputs of the row plan of `find_cluster -a mcl` (find_cluster.row_plan / device_row_plan, libsohit so_cnc_plan), shared by
tests/test_cnc_plan.py (CPU) and tests/test_gpu_cnc_plan.py (GPU).  No GPU here.

An input is (cx, cy, Z, n_codes): the id codes of the rows in file order, cx <= cy in every row, the float64 weights, and the number of
codes.  Genes are written as sortable tuples; a gene's code is its rank among the input's genes in sorted order (what the byte order of
the ids is to real rows), optionally spread out so that codes stay unused; a row's ends are put smaller code first.

Every input is at the smallest shape where its kernel can go wrong.  The sizes are the code's own (read out of swiftortho_amd/csrc):
the numbering (k_util.hip) / k_plan_* / k_cnc_* kernels run 256 lanes a workgroup over the rows, over the 2 x rows positions of cx0, cy0, cx1, ... and over the
kept rows; scan_u32 (k_util.hip: SCAN_TILE = 256 * 4 * 8, SCAN_SMALL_TILES = 4) takes 8192 values per workgroup and changes from one launch
to three above 4 x 8192 values -- it scans the positions, the rows and the kept rows.  The family graph of about 19 000 rows is the only
large input.

Two cases the plan cannot show, by the rules of group_numbers(): component 0 (the one of the last gene) never merges, its genes carry -1
and a row inside it always exists (the last gene's best row) -- so every input with a row keeps a row, and the pool -1 is present among
the kept rows of EVERY input.  `no_rows` is therefore the only input without a kept row and `one_kept` keeps as few as rows allow.  Every other
component holds a row of its own (its genes' best rows), which makes it a level-2 node with a group number: every row is kept only
where there is ONE component, `one_component`, which is all pool -- there the -1 is all there is to order.  The CPU test asserts this
from numpy."""
import functools

import numpy as np

import cnc_inputs as ci

LANES = 256                 # lanes per workgroup of the numbering / k_plan_* / k_cnc_* kernels
SCAN_TILE = 8192            # values per workgroup of scan_u32
SCAN_ONE_LAUNCH = 4 * 8192  # scan_u32: up to here one launch, above it three
KEPT = (LANES - 1, LANES, LANES + 1, 1023, 1024, 1025, 4095, 4096, 4097, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1,
        SCAN_ONE_LAUNCH - 1, SCAN_ONE_LAUNCH, SCAN_ONE_LAUNCH + 1)
ROWS = (SCAN_ONE_LAUNCH // 2 - 1, SCAN_ONE_LAUNCH // 2, SCAN_ONE_LAUNCH // 2 + 1)   # 2 x rows positions at scan_u32's change of path
TAIL = ("z", 0), ("z", 1)


def coded(rows, low=0, stride=1, high=0):
    """rows (a, b, weight) over sortable genes -> (cx, cy, Z, n_codes): code = low + stride * rank of the gene in sorted order, so `low`
    codes below, `stride - 1` between any two and `high` above the genes stay unused"""
    genes = sorted({g for a, b, _ in rows for g in (a, b)})
    code = {g: low + stride * k for k, g in enumerate(genes)}
    cx = np.array([min(code[a], code[b]) for a, b, _ in rows], dtype=np.int64)
    cy = np.array([max(code[a], code[b]) for a, b, _ in rows], dtype=np.int64)
    n_codes = (low + stride * (len(genes) - 1) + 1 + high) if genes else low + high
    return cx, cy, np.array([w for _, _, w in rows], dtype=np.float64), n_codes


def group_rows(g):
    """two heavy pairs joined by a light row: two level-1 components, one level-2 group, three rows inside it"""
    u, v = ("g", g, "u"), ("g", g, "v")
    return [(u + (0,), u + (1,), 5.0), (v + (0,), v + (1,), 5.0), (u + (0,), v + (0,), 1.0)]


def tail_rows(extra=0):
    """the last pair of an input: it holds the last gene, so it is component 0, whose genes carry -1; with `extra` more rows in a chain"""
    return [(TAIL[0], TAIL[1], 5.0)] + [(("z", 1 + k), ("z", 2 + k), 5.0) for k in range(extra)]


def blocks(kept, seed=None):
    """exactly `kept` kept rows: (kept - 1) // 3 + 1 level-2 groups of three rows each, of which the first in file order is group 0 and is
    dropped, then a tail of 1 + (kept - 1) % 3 rows in the pool.  seed: the groups' rows shuffled (the tail stays last), so neither the
    group numbers nor the gene numbers follow the codes"""
    G, extra = divmod(kept - 1, 3)
    rows = [r for g in range(G + 1) for r in group_rows(g)]
    if seed is not None:
        rows = [rows[i] for i in np.random.default_rng(seed).permutation(len(rows)).tolist()]
    return rows + tail_rows(extra)


def repeated(times, first_chain_row, chain=300):
    """Group 0 (dropped); group 1 = a pair ("a", .) joined to a chain ("c", 0) - ("c", 1) - ... of equal weights; the tail.  In sorted order
    the pool row is position 0, ("a", 0) - ("a", 1) and ("a", 0) - ("c", 0) positions 1 and 2, chain row i position 3 + i.  Chain row
    `first_chain_row` is given `times` times, spread over the file, heaviest first: the repeats sit side by side in the order, the
    lightest -- whose text sorts first -- LAST among them"""
    rows = group_rows(0) + [(("a", 0), ("a", 1), 5.0), (("a", 0), ("c", 0), 1.0)]
    rep = [(("c", first_chain_row), ("c", first_chain_row + 1), 5.0 - 0.01 * k) for k in range(times)]
    for i in range(chain):
        if i != first_chain_row:
            rows.append((("c", i), ("c", i + 1), 5.0))
        if i % 3 == 0 and i // 3 < times:
            rows.append(rep[i // 3])
    return rows + tail_rows()


def family():
    """a family graph with few bridges -- about a hundred level-2 groups -- and twelve of its rows given once more, lighter"""
    rows = ci.family_graph(22, 160, 25, 0.4, 0.4)
    return rows + [(a, b, w * 0.5) for a, b, w in rows[len(rows) // 13::len(rows) // 13][:12]]


@functools.lru_cache(maxsize=None)
def inputs():
    """name -> (cx, cy, Z, n_codes), read-only; every input also with its rows reversed (name + '_reversed')"""
    out = {"no_rows": coded([], high=5),
           "one_row": coded([("a", "b", 2.5)]),
           "two_rows": coded([("a", "b", 2.5), ("c", "d", 1.0)]),
           "two_rows_shared": coded([("b", "c", 2.5), ("a", "b", 1.0)], low=1),
           # every row brings in codes below those of all rows before it: first appearance runs against the codes
           "codes_against_appearance": coded([(("g", 90 - g) + r[0][2:], ("g", 90 - g) + r[1][2:], r[2]) for g in range(40) for r in group_rows(0)] + [(("a", 0), ("a", 1), 5.0)]),
           "unused_codes": coded(blocks(40, seed=1), low=7, stride=3, high=11),
           "one_kept": coded(blocks(1)),
           "one_component": coded([(("c", i), ("c", i + 1), float(i + 1)) for i in range(300)]),
           "group0_dropped": coded(ci.component_zero_rule()),
           "self_pairs": coded(group_rows(0) + group_rows(1) + [(("g", 1, "u", 0), ("g", 1, "u", 0), 0.5), (("s",), ("s",), 3.0), (("g", 1, "u", 1), ("g", 1, "u", 1), 9.0),
                                                               (("s",), ("g", 1, "v", 1), 1.0), (TAIL[0], TAIL[0], 7.0)] + tail_rows(1)),
           "family": coded(family(), high=1000)}
    for k in KEPT:
        out["kept%d" % k] = coded(blocks(k, seed=k))
    for n in ROWS:
        out["rows%d" % n] = coded(blocks(n - 3, seed=n), stride=2)
    out["repeat2_straddles_256"] = coded(repeated(2, LANES - 4))
    out["repeat3_straddles_256"] = coded(repeated(3, LANES - 4))
    out["repeat64_straddles_256"] = coded(repeated(64, LANES - 35))
    for name in list(out):
        cx, cy, z, n_codes = out[name]
        out[name + "_reversed"] = (cx[::-1].copy(), cy[::-1].copy(), z[::-1].copy(), n_codes)
    for v in out.values():
        for a in v[:3]:
            a.setflags(write=False)
    return out


def refusals():
    """name -> ((cx, cy, Z, n_codes), a piece of the message)"""
    cx, cy, z, n_codes = inputs()["group0_dropped"]
    at = lambda a, i, v: np.where(np.arange(len(a)) == i, v, a)
    return {"nan_weight": ((cx, cy, at(z, 3, np.nan), n_codes), "NaN"),
            "code_above": ((cx, at(cy, 4, n_codes), z, n_codes), "outside 0 .. n_codes - 1"),
            "code_below": ((at(cx, 0, -1), cy, z, n_codes), "outside 0 .. n_codes - 1"),
            "x_above_y": ((at(cx, 2, cy[2]), at(cy, 2, cx[2]), z, n_codes), "cx > cy"),
            "negative_codes": ((cx[:0], cy[:0], z[:0], -1), "bad arguments"),
            "too_many_codes": ((cx[:0], cy[:0], z[:0], 2 ** 31), "2^31")}
