"""TEST INFRASTRUCTURE -- id-coded relation rows aimed at the edges of the device stage of `find_cluster -a apc -G A` (libsohit
so_apc_rows, swiftortho_amd/csrc/apc.hip): numbering against code order, unused codes and taxa, block and scan bounds, rows of the
layout at the lane / wave split, self and repeated pairs, weights at the edges of float32, a column whose entry order shows in a bit.
Every input is (cx, cy, z, n_codes, taxon_of_code) for find_cluster.apc_entry_columns (the definition) and device_apc_rows; each comes a
second time with its rows reversed.  tests/test_apc_rows.py asserts from the definition alone that every input holds what its name
promises; tests/test_gpu_apc_rows.py runs them on the device."""
import functools

import numpy as np

from apc_edge_inputs import LM, QUARTER_ULP, TINY, W

HUB_LENGTHS = (LM, LM + 1, W, W + 1)            # entries of the hub's row (and column), its preference entry included
GENE_COUNTS = (255, 256, 257)
ROW_COUNTS = (4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768, 32769)
REPEATS = (2, 3, 64)
SMALL = 1500                                     # entries up to which the literal oracle runs too


def _mk(rows, n_codes, tax=None):
    """rows (a, b, w) of codes -> columns with cx <= cy; taxon code % 3 unless given"""
    cx = np.array([min(r[0], r[1]) for r in rows], dtype=np.int64)
    cy = np.array([max(r[0], r[1]) for r in rows], dtype=np.int64)
    z = np.array([r[2] for r in rows], dtype=np.float64)
    tax = np.arange(n_codes, dtype=np.int32) % 3 if tax is None else np.asarray(tax, dtype=np.int32)
    assert len(tax) == n_codes and (len(cx) == 0 or (cx.min() >= 0 and cy.max() < n_codes))
    return cx, cy, z, int(n_codes), tax


def _weights(n, seed):
    """half of the weights from three values (ties inside rows and columns), the rest spread over four decades"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(n) < 0.5, rng.choice([1.0, 2.5, 10.0], n), np.round(10 ** rng.uniform(-2, 2, n), 4)).tolist()


# ---- sizes and codes ------------------------------------------------------------------------------------------------------------------
def chain(codes, seed=1):
    """rows (codes[i], codes[i + 1]) in that order"""
    w = _weights(len(codes) - 1, seed)
    return [(codes[i], codes[i + 1], w[i]) for i in range(len(codes) - 1)]


def codes_ascending():
    return _mk(chain(list(range(12))), 12)


def codes_descending():
    return _mk(chain(list(range(11, -1, -1))), 12)


def codes_shuffled():
    rng = np.random.default_rng(7)
    return _mk(chain(rng.permutation(40).tolist(), 2) + chain(rng.permutation(40).tolist(), 3), 40)


UNUSED_USED = (3, 4, 7, 8, 12)                   # of 20 codes: unused ones below, between and above


def unused_codes():
    u = UNUSED_USED
    return _mk([(u[4], u[0], 2.0), (u[1], u[2], 1.0), (u[0], u[3], 2.5), (u[2], u[4], 0.5)], 20)


def taxon_of_unused_codes_only():
    """taxon 2 is carried by codes 0, 1 and 9 alone, and no row names them: two taxa count"""
    tax = [2, 2, 0, 1, 0, 1, 0, 1, 0, 2]
    return _mk([(2, 3, 1.0), (4, 5, 2.0), (3, 6, 2.0), (7, 8, 1.5), (2, 8, 0.25)], 10, tax)


def one_taxon():
    return _mk(chain(list(range(9)), 4), 9, [0] * 9)


def every_gene_its_taxon():
    return _mk(chain([5, 1, 7, 3, 0, 8, 2], 5), 9, list(range(9)))


def gene_count(d):
    """a path over d genes whose codes are shuffled against their numbers, 5 codes unused"""
    codes = np.random.default_rng(d).permutation(d + 5)[:d].tolist()
    return _mk(chain(codes, d), d + 5)


def row_count(n):
    """n random rows over 700 codes (self pairs and repeated pairs among them)"""
    rng = np.random.default_rng(n)
    a, b = rng.integers(0, 700, n).tolist(), rng.integers(0, 700, n).tolist()
    return _mk(list(zip(a, b, _weights(n, n + 1))), 700, (np.arange(700) % 7).tolist())


# ---- row lengths --------------------------------------------------------------------------------------------------------------------
def hub(L, hub_first, self_pair=False):
    """one hub whose row holds exactly L entries: its preference entry, L - 1 leaves -- or L - 3 leaves and a self pair, which stands
    twice.  `hub_first`: the hub is gene 0 (it opens the first row); otherwise a leaf is, and the hub is gene 1.  A second, short star
    hangs on the last leaf."""
    leaves = L - 3 if self_pair else L - 1
    h = 2 * leaves + 1                            # the hub's code lies above its leaves': every row reads (leaf, hub)
    w = _weights(leaves, L)
    rows = [(k, h, w[k]) for k in range(leaves)]
    if hub_first:
        rows = [(h, h + 1, 3.0)] + rows[:-1]      # (cx = h < cy: the hub comes first; still L - 1 / L - 3 partners)
    if self_pair:
        rows.insert(len(rows) // 2, (h, h, 1.5))
    rows += [(leaves - 2, h + 2, 1.0), (leaves - 2, h + 3, 2.0)]
    return _mk(rows, h + 4)


def self_pairs():
    return _mk([(0, 0, 2.0), (0, 1, 1.0), (2, 2, 0.5), (1, 2, 4.0), (2, 2, 0.5), (3, 3, 1.0)], 4)


def repeated(k):
    """one pair on k lines with k weights, the lines placed across positions 255 | 256, behind a path of filler rows"""
    fill = 256 - (k + 1) // 2
    rows = chain(list(range(2, fill + 3)), k)
    assert len(rows) == fill
    rows += [(0, 1, 1.0 + 0.25 * (j % 5)) for j in range(k)]
    rows += [(1, 2, 2.0), (0, fill + 2, 0.5)]
    return _mk(rows, fill + 3)


# ---- weights --------------------------------------------------------------------------------------------------------------------------
WEIGHTS = {"zeros": (0.0, -0.0), "denormal": (1e-42, 3e-45), "overflow": (1e39, -1e39), "nan": (float("nan"),), "pinf": (float("inf"),),
           "ninf": (-float("inf"),), "tie_to_even": (1.0 + 2.0 ** -24,), "round_up": (1.0 + 2.0 ** -24 + 2.0 ** -50,)}


def weights(kind):
    """two small stars joined by a row; the named weights on the first rows of the first star"""
    rows = [(k, 20, 1.0 + 0.5 * (k % 3)) for k in range(8)] + [(k, 21, 2.0) for k in range(8, 14)] + [(7, 8, 0.75)]
    for j, v in enumerate(WEIGHTS[kind]):
        rows[2 * j + 1] = (rows[2 * j + 1][0], rows[2 * j + 1][1], v)
    return _mk(rows, 22)


# ---- a column whose sum shows the order of its entries -----------------------------------------------------------------------------------
def ordered_column(n, tiny_first):
    """hub code n with n leaves: the hub's column holds the leaves' entries in row order, then its preference entry.  All weights 0 but
    3 * 2^-55 twice, 2^-24 and 1.0 (apc_edge_inputs.ordered_column): after one round at damping 0.5 the A of the hub's diagonal is the
    float32 of half the float64 sum IN ENTRY ORDER -- tiny + tiny + 2^-24 + 1 rounds up, 1 + 2^-24 + tiny + tiny does not."""
    s = [0.0] * n
    if tiny_first:
        s[0] = s[1] = TINY
        s[n - 2], s[n - 1] = QUARTER_ULP, 1.0
    else:
        s[0], s[1] = 1.0, QUARTER_ULP
        s[n - 2] = s[n - 1] = TINY
    return _mk([(k, n, s[k]) for k in range(n)], n + 1, [0] * (n + 1))


# ---- the registry ----------------------------------------------------------------------------------------------------------------------
def _registry():
    reg = {"one_row": lambda: _mk([(0, 1, 1.5)], 2), "two_rows": lambda: _mk([(1, 2, 1.5), (0, 1, 0.5)], 3), "no_row": lambda: _mk([], 3),
           "codes_ascending": codes_ascending, "codes_descending": codes_descending, "codes_shuffled": codes_shuffled, "unused_codes": unused_codes,
           "taxon_of_unused_codes_only": taxon_of_unused_codes_only, "one_taxon": one_taxon, "every_gene_its_taxon": every_gene_its_taxon,
           "self_pairs": self_pairs}
    for d in GENE_COUNTS:
        reg["genes_%d" % d] = functools.partial(gene_count, d)
    for n in ROW_COUNTS:
        reg["rows_%d" % n] = functools.partial(row_count, n)
    for L in HUB_LENGTHS:
        reg["hub_first_L%d" % L] = functools.partial(hub, L, True)
        reg["hub_later_L%d" % L] = functools.partial(hub, L, False)
        reg["hub_self_L%d" % L] = functools.partial(hub, L, False, True)
    for k in REPEATS:
        reg["repeated_%d" % k] = functools.partial(repeated, k)
    for kind in WEIGHTS:
        reg["weights_" + kind] = functools.partial(weights, kind)
    for tag, n in (("lane", LM - 1), ("wave", W + 6)):
        reg["ordered_%s_tiny_first" % tag] = functools.partial(ordered_column, n, True)
        reg["ordered_%s_one_first" % tag] = functools.partial(ordered_column, n, False)
    return reg


REGISTRY = _registry()
BASE_NAMES = sorted(REGISTRY)
NAMES = sorted(BASE_NAMES + [n + "_rev" for n in BASE_NAMES])
ORDERED = [n for n in BASE_NAMES if n.startswith("ordered_")]
HUNDRED = ("hub_later_L%d" % (W + 1), "repeated_64", "codes_shuffled")          # the inputs that also run the reference's 100 rounds


@functools.lru_cache(maxsize=None)
def rows(name):
    """(cx, cy, z, n_codes, taxon_of_code) of an input, built once, read-only; `<name>_rev`: the same rows in reverse order"""
    if name.endswith("_rev"):
        cx, cy, z, n_codes, tax = rows(name[:-4])
        out = (cx[::-1].copy(), cy[::-1].copy(), z[::-1].copy(), n_codes, tax)
    else:
        out = REGISTRY[name]()
    for x in out:
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def definition(name):
    """apc_entry_columns of an input, once, read-only: (gene_code, row, col, score, n_genes, n_taxa_used)"""
    from swiftortho_amd import find_cluster as fc
    out = fc.apc_entry_columns(*rows(name))
    for x in out[:4]:
        x.setflags(write=False)
    return out


def is_small(name):
    return len(definition(name)[1]) <= SMALL


def rounds_of(name):
    return (1, 2, 3, 10, 100) if (name[:-4] if name.endswith("_rev") else name) in HUNDRED else (1, 2, 3, 10)


@functools.lru_cache(maxsize=None)
def oracle_snapshots(name, damp):
    """the literal oracle's (labels, R, A) on the definition's entries after each round asked of a small input, from one run"""
    from apc_numpy_oracle import apc_rounds
    _, row, col, score, n, _ = definition(name)
    want, out = rounds_of(name), {}
    with np.errstate(all="ignore"):
        for t, snap in enumerate(apc_rounds(row, col, score, n, damp, max(want))):
            if t + 1 in want:
                for x in snap:
                    x.setflags(write=False)
                out[t + 1] = snap
    return out
