"""Container-only: goldens for the affinity-propagation clustering stage (`find_cluster -a apc`).

    python tools/refharness/make_apc_goldens.py [--force]

Runs the REAL reference script bin/find_cluster.py -a apc (numpy + networkx; tools/refharness/fcshim/ stands in for its numba
and cffi imports, so the loop runs as plain Python: ~30 s for the largest input) on .orth files and stores its stdout.
Fixtures: tests/golden/apc_<name>.<variant>.apc (expected stdout), apc_<name>.json (input file name, flags per variant),
apc_odd_rows.orth, a small input written here that holds the rows fc2mat treats specially, and apc_hub_edges.orth, the two-hub graph
of tests/apc_edge_inputs.py at the hub degrees that give rows of APC_LANE_MAX + 1 and 64 + 1 entries.
"""
import json
import os
import sys

from make_cluster_goldens import FORCE, GOLD, ROOT, run_ref_find_cluster

# a repeated pair with two weights, a self pair, an x > y row, three-column rows, an id without '|', a weight of the form 1.5rm3 and an
# unparsable weight whose genes appear nowhere else (they are numbered all the same, and end as groups of their own)
ODD_ROWS = [
    "OT\tt1|a\tt1|b\t3.5",
    "OT\tt1|a\tt1|b\t1.25",
    "IP\tt1|c\tt1|c\t2.0",
    "OT\tt2|z\tt1|a\t9.0",
    "t1|b\tt2|d\t4.0",
    "OT\tnopipe\tt2|d\t1.0",
    "OT\tt1|c\tt2|d\t1.5rm3",
    "OT\tu1|lost\tu2|lost\tabc",
    "OT\tt1|a\tt2|d\t6.0",
    "t3|e\tt3|f\t7.5",
    "OT\tt1|b\tt3|e\t0.5",
    "OT\tt2|g\tt3|f\t7.5",
    "CO\tt2|g\tt3|e\t7.5",
    "OT\tt1|c\tt2|g\t0.25",
]


def hub_edges_rows(seed=2, taxa=2):
    """two hubs sharing most leaves, tied weights, pairs in a seeded order (tests/apc_edge_inputs.py two_hub_pairs): after fc2mat's
    doubling and preference entries the hubs' rows hold LM + 1 and W + 1 entries -- one past the lane / wave split of so_apc, one past
    a full chunk"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import apc_edge_inputs as X
    pairs, _ = X.two_hub_pairs(X.LM + 1, X.W + 1, seed)
    name = lambda g: "t%d|g%03d" % (g % taxa, g)
    return ["OT\t%s\t%s\t%r" % (tuple(sorted((name(x), name(y)))) + (w,)) for x, y, w in pairs]


def make(name, orth_file, variants):
    meta_path = os.path.join(GOLD, "apc_%s.json" % name)
    if os.path.isfile(meta_path) and not FORCE:
        print(name, "exists, skipped")
        return
    meta = {"input": os.path.basename(orth_file), "variants": {}}
    for v, flags in variants.items():
        out = run_ref_find_cluster(orth_file, flags)
        open(os.path.join(GOLD, "apc_%s.%s.apc" % (name, v)), "wb").write(out)
        meta["variants"][v] = flags
        print(name, v, "groups", out.count(b"\n"), "genes", len(out.split()))
    json.dump(meta, open(meta_path, "w"), indent=1)


def main():
    default = {"default": ["-a", "apc"]}
    for n in ("taxa5", "taxa3_dense", "taxa4_colon", "toy_default"):
        make(n, os.path.join(GOLD, "orth_%s.default.orth" % n), default)
    odd = os.path.join(GOLD, "apc_odd_rows.orth")
    if FORCE or not os.path.isfile(odd):
        open(odd, "w").write("".join(l + "\n" for l in ODD_ROWS))
    make("odd_rows", odd, default)
    hub = os.path.join(GOLD, "apc_hub_edges.orth")
    if FORCE or not os.path.isfile(hub):
        open(hub, "w").write("".join(l + "\n" for l in hub_edges_rows()))
    make("hub_edges", hub, {"default": ["-a", "apc"], "d0.9": ["-a", "apc", "-d", "0.9"]})
    make("taxa8_big", os.path.join(GOLD, "clu_taxa8_big.orth"),
         {"default": ["-a", "apc"], "d0.95": ["-a", "apc", "-d", "0.95"], "b1000": ["-a", "apc", "-b", "1000"]})


if __name__ == "__main__":
    main()
