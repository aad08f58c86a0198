"""TEST INFRASTRUCTURE -- the random relation graphs of the affinity-propagation tests (tests/test_find_cluster_apc.py), shared with
the stale-memory test of tests/test_gpu_mcl.py"""
import functools

import numpy as np


def _apc_graph(seed, nfam, famsize, p, hub_small=0, hub_big=0):
    """relation rows of random family graphs: families of `famsize` genes joined with probability p, half of the weights drawn from
    three values (ties inside rows and columns), weak bridges between families, repeated pairs with the same and with another weight,
    a self pair, optionally a hub gene tied to `hub_small` genes of the families and one tied to `hub_big` genes of its own, and a
    gene that only appears on a row with an unparsable weight (it has nothing but its preference entry)"""
    rng = np.random.default_rng(seed)
    lines, genes = [], []
    for f in range(nfam):
        names = ["t%d|f%dg%d" % (k % 7, f, k) for k in range(famsize)]
        genes += names
        for i in range(famsize):
            for j in range(i + 1, famsize):
                if rng.random() < p:
                    a, b = sorted((names[i], names[j]))
                    w = float(rng.choice([1.0, 2.5, 10.0])) if rng.random() < 0.5 else float(np.round(10 ** rng.uniform(-2, 2), 4))
                    lines.append("OT\t%s\t%s\t%r\n" % (a, b, w))
    for _ in range(nfam * 3):   # weak bridges
        f, g = rng.integers(0, nfam, 2)
        a, b = sorted(("t0|f%dg0" % f, "t1|f%dg1" % g))
        lines.append("CO\t%s\t%s\t0.01\n" % (a, b))
    if hub_small:
        for g in rng.choice(len(genes), hub_small, replace=False).tolist():
            a, b = sorted(("t3|hub", genes[g]))
            lines.append("OT\t%s\t%s\t%r\n" % (a, b, float(rng.choice([0.5, 3.0]))))
    for k in range(hub_big):
        a, b = sorted(("t4|HUB", "t%d|leaf%d" % (k % 7, k)))
        lines.append("OT\t%s\t%s\t%r\n" % (a, b, float(rng.choice([1.0, 2.0, 4.0]) if k % 3 else np.round(rng.uniform(0.1, 5), 3))))
    lines += lines[:7]                                               # repeated pairs, same weight
    lines += [l.rsplit("\t", 1)[0] + "\t3.125\n" for l in lines[7:12]]   # ... and another one
    lines += ["IP\tt0|f0g0\tt0|f0g0\t2.0\n", "OT\tt5|alone\tt6|alone\tn/a\n"]
    order = rng.permutation(len(lines)).tolist()
    return [lines[o] for o in order]


GRAPHS = {"families": dict(seed=1, nfam=30, famsize=10, p=0.6, hub_small=75),
          "hubs": dict(seed=2, nfam=20, famsize=8, p=0.6, hub_small=90, hub_big=1150),
          "dense": dict(seed=3, nfam=2, famsize=96, p=0.72, hub_small=70)}


@functools.lru_cache(maxsize=None)
def _entries(graph):
    from swiftortho_amd import find_cluster as fc
    return fc.apc_entries(_apc_graph(**GRAPHS[graph]))
