"""Inputs of the component stage of `find_cluster -a mcl` (find_cluster.group_numbers, libsohit so_cnc_groups), shared by
tests/test_cnc_groups.py (CPU) and tests/test_gpu_cnc.py (GPU), and a plain-Python restatement of the closed form the kernels compute.

An input is (X, Y, Z, n): the gene numbers of the rows in file order, genes numbered 0 .. n-1 by first appearance (x of a row before
its y), and the float64 weights.  Every input is small: the smallest shapes at which a sweep, a block edge (256 lanes a workgroup, 1024 =
four of them) or a rule can go wrong; the two family graphs of about 20 000 genes and 100 000 rows are the only large ones."""
import functools
import math

import numpy as np


def from_rows(rows):
    """rows (a, b, weight) over any hashable gene labels -> (X, Y, Z, n), genes numbered by first appearance, x before y"""
    number = {}
    X, Y, Z = [], [], []
    for a, b, w in rows:
        for g in (a, b):
            if g not in number:
                number[g] = len(number)
        X.append(number[a]), Y.append(number[b]), Z.append(w)
    return np.array(X, dtype=np.int64), np.array(Y, dtype=np.int64), np.array(Z, dtype=np.float64), len(number)


def chain(k, order):
    """a path v0 - v1 - ... - v(k-1) whose weights rise along it: every gene's best neighbour is the next one, the last one's the one
    before it, so every row is a tie row and the tie graph is the one chain.  order: 'up' (gene numbers rise along the chain), 'down' (they
    fall), or a seed (rows and their two ends shuffled: a shuffled numbering)"""
    rows = [(i, i + 1, float(i + 1)) for i in range(k - 1)]
    if order == "down":
        rows = [(b, a, w) for a, b, w in reversed(rows)]
    elif order != "up":
        rng = np.random.default_rng(order)
        rows = [rows[i] for i in rng.permutation(len(rows)).tolist()]
        rows = [(b, a, w) if f else (a, b, w) for (a, b, w), f in zip(rows, (rng.random(len(rows)) < 0.5).tolist())]
    return rows


def star(leaves, hub_last):
    """a hub with `leaves` leaves, all weights equal.  hub_last: lighter rows between the leaves come first, so the hub is gene n-1 (those
    rows are no tie rows: every leaf's best row is the hub's); otherwise the hub is gene 0"""
    rows = []
    if hub_last:
        rows = [(("l", i), ("l", (i + 1) % leaves), 0.5) for i in range(0, leaves, 2)]
    return rows + [("hub", ("l", i), 1.0) for i in range(leaves)]


def sized(n, r, seed):
    """exactly n genes and r rows (r >= (n + 1) // 2): rows that bring in the genes two at a time, then random pairs, self pairs among them;
    weights 1 .. 4 so that ties are common; row order shuffled"""
    rng = np.random.default_rng(seed)
    rows = [(g, min(g + 1, n - 1), float(rng.integers(1, 5))) for g in range(0, n, 2)]
    assert len(rows) <= r
    while len(rows) < r:
        a, b = rng.integers(0, n, 2).tolist()
        rows.append((a, b, float(rng.integers(1, 5))))
    return [rows[i] for i in rng.permutation(r).tolist()]


def component_chain(k, seed=None):
    """k level-1 components (pairs with a heavy row) joined into a path by light rows, then one more pair that becomes component 0: level 2
    is one chain of k components"""
    rows = [(("p", c, 0), ("p", c, 1), 9.0) for c in range(k)] + [(("p", c, 1), ("p", c + 1, 0), 1.0) for c in range(k - 1)]
    if seed is not None:
        rng = np.random.default_rng(seed)
        rows = [rows[i] for i in rng.permutation(len(rows)).tolist()]
    return rows + [("z0", "z1", 9.0)]


def component_zero_rule():
    """A = {a1, a2}, B = {b1, b2} joined by a light row: the first row with two non-zero numbers touches them, so they are level-2 group 0,
    which is dropped.  D, E joined: group 1, kept.  C = {c1, c2, c3} holds the last gene: component 0, with light rows to A and to B -- it
    does not merge, its genes get -1 and its inner rows are kept."""
    return [("a1", "a2", 5.0), ("b1", "b2", 5.0), ("a1", "b1", 1.0), ("d1", "d2", 5.0), ("e1", "e2", 5.0), ("d1", "e1", 1.0),
            ("c1", "c2", 5.0), ("c1", "a1", 1.0), ("c2", "b2", 1.0), ("c2", "c3", 5.0)]


def level2_order(variant):
    """four level-2 groups of two components each (pairs joined by a light row), then a pair that becomes component 0.
    'opposite': in file order, so the group of the first rows holds the LARGEST component numbers (components are numbered from the last
    gene down).  'same': every component gets a third gene in a late row, the first component's last, so the group of the first rows
    holds the smallest numbers.  A seed: the rows of 'same' shuffled."""
    rows = []
    for g in range(4):
        rows += [(("u", g, 0), ("u", g, 1), 5.0), (("v", g, 0), ("v", g, 1), 5.0), (("u", g, 0), ("v", g, 0), 1.0)]
    if variant != "opposite":
        for g in (3, 2, 1, 0):
            rows += [(("v", g, 1), ("v", g, 2), 5.0), (("u", g, 1), ("u", g, 2), 5.0)]
    if variant not in ("opposite", "same"):
        rng = np.random.default_rng(variant)
        rows = [rows[i] for i in rng.permutation(len(rows)).tolist()]
    return rows + [("z0", "z1", 5.0)]


def family_graph(seed, nfam, famsize, density=0.6, bridges=3.0):
    """tests/test_find_cluster.py `_family_graph`, as rows: dense families, weights over four decades, weak bridges (`bridges` per family), five repeated rows;
    a row's ends are ordered as their ids would be"""
    rng = np.random.default_rng(seed)
    rows = []
    iu, ju = np.triu_indices(famsize, 1)
    for f in range(nfam):
        use = rng.random(len(iu)) < density
        w = np.round(10 ** rng.uniform(-2, 2, int(use.sum())), 4)
        rows += [((f, i), (f, j), z) for i, j, z in zip(iu[use].tolist(), ju[use].tolist(), w.tolist())]
    for _ in range(int(nfam * bridges)):
        f, g = rng.integers(0, nfam, 2).tolist()
        a, b = sorted(((f, 0), (g, 1)))
        rows.append((a, b, 0.01))
    return rows + rows[:5]


def random_small(seed):
    """2 .. 40 genes, 1 .. 80 rows, weights 1 .. 4 (ties are common), self pairs and repeated pairs"""
    rng = np.random.default_rng(seed)
    g = int(rng.integers(2, 41))
    r = int(rng.integers(1, 81))
    a, b = rng.integers(0, g, r), rng.integers(0, g, r)
    same = rng.random(r) < 0.08
    b[same] = a[same]
    w = rng.integers(1, 5, r).astype(float)
    return from_rows(list(zip(a.tolist(), b.tolist(), w.tolist())))


def _with_tail(rows):
    """... and a last pair, which becomes component 0: the rows before it then carry non-zero component numbers"""
    return rows + [("tail0", "tail1", 7.0)]


@functools.lru_cache(maxsize=None)
def inputs():
    """name -> (X, Y, Z, n), read-only"""
    out = {"no_rows": from_rows([]), "one_self_pair": from_rows([("a", "a", 1.0)]), "one_pair": from_rows([("a", "b", 1.0)])}
    for k in (2, 63, 64, 65, 257, 5000):
        for order in ("up", "down", 7):
            out["chain%d_%s" % (k, order)] = from_rows(chain(k, order))
    for leaves in (64, 65, 1025):
        out["star%d_hub0" % leaves] = from_rows(star(leaves, False))
        out["star%d_hub_last" % leaves] = from_rows(star(leaves, True))
    out["complete40"] = from_rows([(i, j, 2.0) for i in range(40) for j in range(i + 1, 40)])
    for v in (255, 256, 257, 1023, 1024, 1025):
        out["genes%d" % v] = from_rows(sized(v, v + v // 2 + 7, v))
        out["rows%d" % v] = from_rows(sized(v // 2 + 5, v, v + 1))
    for k in (65, 300):
        out["component_chain%d" % k] = from_rows(component_chain(k))
        out["component_chain%d_shuffled" % k] = from_rows(component_chain(k, 3))
    out["component_zero_rule"] = from_rows(component_zero_rule())
    for variant in ("opposite", "same", 5, 6):
        out["level2_%s" % variant] = from_rows(level2_order(variant))
    out["self_pair_only_row"] = from_rows(_with_tail([("s", "s", 3.0), ("a", "b", 1.0), ("b", "c", 1.0)]))
    out["self_pair_beside_heavier"] = from_rows(_with_tail([("t", "t", 1.0), ("t", "u", 2.0), ("a", "b", 1.0), ("u", "a", 0.5)]))
    # a ties with b and with c, and c has a better row of its own: a - c is a tie row only because EVERY row that reaches a's best is one
    out["two_best_neighbours"] = from_rows(_with_tail([("a", "b", 1.0), ("a", "c", 1.0), ("c", "d", 2.0)]))
    out["repeated_pair_two_weights"] = from_rows(_with_tail([("a", "b", 1.0), ("b", "c", 1.5), ("a", "b", 2.0), ("c", "d", 1.0)]))
    out["negative_weights"] = from_rows(_with_tail([("a", "b", -1.0), ("b", "c", -2.0), ("c", "d", -1.5), ("d", "e", -3.0), ("e", "f", -1.5)]))
    # a's best is +0.0 (a - b); a - c weighs -0.0, and c has a better row (c - d): only `-0.0 == 0.0` makes a - c a tie row
    out["signed_zeros"] = from_rows(_with_tail([("a", "b", 0.0), ("a", "c", -0.0), ("c", "d", 1.0), ("e", "f", -0.0), ("e", "g", 0.0), ("g", "h", 2.0)]))
    out["infinities"] = from_rows(_with_tail([("a", "b", math.inf), ("b", "c", -math.inf), ("c", "d", -math.inf), ("e", "f", 1.0), ("f", "g", math.inf),
                                              ("h", "h", -math.inf), ("d", "e", -math.inf)]))
    out["family_a"] = from_rows(family_graph(21, 1060, 18))
    out["family_b"] = from_rows(family_graph(22, 800, 25, 0.4, 0.4))     # few bridges: hundreds of level-2 groups
    for v in out.values():
        for a in v[:3]:
            a.setflags(write=False)
    return out


def keep_rows(X, Y, grp):
    """the rows cnc hands on: both ends in the same level-2 group, and that group is not 0"""
    gx, gy = grp[X], grp[Y]
    return (gx != 0) & (gy != 0) & (gx == gy)


# ---- the closed form, in plain Python -----------------------------------------------------------------------------------------------
DEVIATIONS = ("min_label", "first_best_only", "signed_zero", "rank_by_component", "component0_merges", "keep_group0")


def _components(n, pairs, largest=True):
    """label of every node = the largest (smallest) node of its connected component"""
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for u, v in pairs:
        ru, rv = find(u), find(v)
        if ru != rv:
            hi, lo = (max(ru, rv), min(ru, rv)) if largest else (min(ru, rv), max(ru, rv))
            parent[lo] = hi
    return [find(a) for a in range(n)]


def closed_form(X, Y, Z, n, deviation=None):
    """what the kernels compute, step by step as the issue states it -> (comp1, grp, keep).  `deviation`: one of DEVIATIONS, a single
    wrong turn (the tests show that each is told apart from group_numbers by some input)"""
    assert deviation is None or deviation in DEVIATIONS
    X, Y, Z = [int(v) for v in X], [int(v) for v in Y], [float(v) for v in Z]
    rows = range(len(X))
    if not len(X):
        return np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int64), np.zeros(0, dtype=bool)
    image = (lambda z: (z, math.copysign(1.0, z))) if deviation == "signed_zero" else (lambda z: z + 0.0 if z != 0 else 0.0)
    # 1. the largest weight over the rows that touch a gene
    best, first_best = [None] * n, [None] * n
    for i in rows:
        for g in (X[i], Y[i]):
            if best[g] is None or image(Z[i]) > best[g]:
                best[g], first_best[g] = image(Z[i]), i
    # 2. tie rows; level-1 components
    if deviation == "first_best_only":
        tie = [first_best[X[i]] == i or first_best[Y[i]] == i for i in rows]
    else:
        tie = [image(Z[i]) == best[X[i]] or image(Z[i]) == best[Y[i]] for i in rows]
    lab = _components(n, [(X[i], Y[i]) for i in rows if tie[i]], largest=deviation != "min_label")
    # 3. a component's number = how many components have a larger root
    roots = sorted(set(lab))
    below = {r: k for k, r in enumerate(roots)}
    comp1 = [len(roots) - 1 - below[lab[g]] for g in range(n)]
    # 4. level 2 over the component numbers
    joins = [i for i in rows if deviation == "component0_merges" or (comp1[X[i]] != 0 and comp1[Y[i]] != 0)]
    lab2 = _components(len(roots), [(comp1[X[i]], comp1[Y[i]]) for i in joins])
    first = {}
    for i in joins:
        first.setdefault(lab2[comp1[X[i]]], i)
    if deviation == "rank_by_component":
        order = sorted(first, key=lambda r: min(c for c in range(len(roots)) if lab2[c] == r))
    else:
        order = sorted(first, key=lambda r: first[r])
    rank = {r: k for k, r in enumerate(order)}
    grp = [rank.get(lab2[c], -1) if (c != 0 or deviation == "component0_merges") else -1 for c in comp1]
    # 5. rows inside one group other than group 0
    keep = [grp[X[i]] == grp[Y[i]] and (grp[X[i]] != 0 or deviation == "keep_group0") for i in rows]
    return np.array(comp1, dtype=np.int64), np.array(grp, dtype=np.int64), np.array(keep, dtype=bool)
