"""The shared-family counts and the gene-content tree in one warm process: so_pan_shared (one matrix; B bootstrap replicates, draw and
product split by events) against the numpy definitions of swiftortho_amd/pan.py, and the whole `scripts/pan_genome.py -t -B` command under
`-G T` and `-G F`, alternating, on a synthetic pan-genome of `rows` families x `taxa` genomes: 2 % core families (each genome holds one
with probability 0.98), the others accessory -- the genomes stand in groups of 20, an accessory family lives in one group and is held by
1 + floor(19 u^2) of its genomes (u uniform), so most families are rare, as they are in a real table.
    python tools/diag/pan_content_cost.py [rows] [taxa] [rounds] [B] [device | command | host | all]
Defaults: 200000 rows x 500 taxa, 5 rounds, B = 100, all.  `command` writes the two input files under a temporary directory."""
import os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from swiftortho_amd import pan

what = sys.argv[-1] if sys.argv[-1] in ("device", "command", "host", "all") else "all"      # host: the command under -G F alone (no device needed)
args = [int(x) for x in sys.argv[1:] if x.isdigit()]
R = args[0] if args else 200000
T = args[1] if len(args) > 1 else 500
rounds = args[2] if len(args) > 2 else 5
B = args[3] if len(args) > 3 else 100
SEED = 1


def line(name, tt, note=""):
    tt = sorted(tt)
    print("%-58s min %.4f s  median %.4f s  (%d rounds)  %s" % (name, tt[0], tt[len(tt) // 2], len(tt), note))
    sys.stdout.flush()


def timed(f, n, warm=True):
    out, tt = None, []
    for r in range(n + (1 if warm else 0)):     # the first round warms up (allocator, code objects)
        t = time.time(); out = f(); dt = time.time() - t
        if r or not warm:
            tt.append(dt)
    return out, tt


def synthetic(R, T):
    """-> (row, taxon) int32 of the members, rows in file order"""
    rng = np.random.RandomState(7)
    n_core = R // 50
    core = rng.random_sample((n_core, T)) < .98
    cr, ct = np.nonzero(core)
    n_acc = R - n_core
    groups = (T + 19) // 20
    g = rng.randint(0, groups, size=n_acc)
    k = 1 + np.floor(19 * rng.random_sample(n_acc) ** 2).astype(np.int64)
    ar = np.repeat(np.arange(n_acc), k)
    at = g[ar] * 20 + (rng.random_sample(len(ar)) * 20).astype(np.int64)      # (a genome drawn twice for a family: listed twice, counted once)
    at = np.minimum(at, T - 1)
    row = np.concatenate([cr, n_core + ar]).astype(np.int32)
    tax = np.concatenate([ct, at]).astype(np.int32)
    return row, tax


row, tax = synthetic(R, T)
print("%d rows x %d taxa, %d members (%.1f a row)" % (R, T, len(row), len(row) / float(R)))

if what in ("device", "all"):
    pan.device_shared_counts(row[:8], tax[:8], R, T)       # warm-up: the library, the device, the code objects
    S, tt = timed(lambda: pan.device_shared_counts(row, tax, R, T), rounds)
    line("so_pan_shared, one matrix (upload, product, copy back)", tt)
    ev = []

    def bare(nb):
        st = {}
        out = pan._device_shared("pan_content_cost", row, tax, R, T, SEED, 0, nb, 0, st, want=True, timed=True)
        ev.append(st)
        return out
    _, tt = timed(lambda: bare(0), rounds)
    line("... the same with events", tt, "product %.3f ms (min), %d ranges of row words" % (min(e["product_ms"] for e in ev[1:]), ev[-1]["ranges"]))
    del ev[:]
    Sb, tt = timed(lambda: bare(B), rounds)
    line("so_pan_shared, %d replicates (one call)" % B, tt, "events: draw %.2f ms, product %.2f ms (min over the rounds; %d batch(es), %d MB of counts)"
         % (min(e["draw_ms"] for e in ev[1:]), min(e["product_ms"] for e in ev[1:]), ev[-1]["batches"], ev[-1]["bytes"] >> 20))
    counts = pan.count_matrix(row, tax, R, T)
    want, tt = timed(lambda: pan.shared_counts(counts), rounds, warm=False)
    line("numpy: shared_counts (float64 products)", tt, "device identical to numpy: %s" % np.array_equal(S, want))
    want, tt = timed(lambda: pan.boot_shared(counts, SEED, B - 1), rounds, warm=False)
    line("numpy: boot_shared, one replicate", tt, "device identical to numpy: %s" % np.array_equal(Sb[B - 1], want))
    del counts, S, Sb, want

if what in ("command", "host", "all"):
    with tempfile.TemporaryDirectory() as d:
        fa, gr = os.path.join(d, "x.fsa"), os.path.join(d, "x.clsr")
        names = ["t%03d" % t for t in range(T)]
        order = np.argsort(row, kind="stable")
        r_s, t_s = row[order], tax[order]
        _, first = np.unique(np.stack([r_s, t_s], 1), axis=0, return_index=True)      # one gene per (family, genome)
        r_s, t_s = r_s[np.sort(first)], t_s[np.sort(first)]
        ids = ["%s|f%d" % (names[t], r) for r, t in zip(r_s.tolist(), t_s.tolist())]
        with open(fa, "w") as o:
            o.write("".join(">%s\nM\n" % i for i in ids))
        bounds = np.flatnonzero(np.concatenate([[True], r_s[1:] != r_s[:-1], [True]]))
        with open(gr, "w") as o:
            o.write("".join("\t".join(ids[a:b]) + "\n" for a, b in zip(bounds[:-1].tolist(), bounds[1:].tolist())))
        print("the command's input: %d genes, %d group lines" % (len(ids), len(bounds) - 1))
        del ids
        tt, out = {"T": [], "F": []}, {}
        for r in range(rounds):
            for G in ("F",) if what == "host" else ("T", "F"):              # alternating
                nwk = os.path.join(d, "x_%s.nwk" % G)
                t = time.time()
                with open(os.devnull, "wb") as null:
                    subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pan_genome.py"), "-i", fa, "-g", gr, "-t", nwk, "-B", str(B), "-S", str(SEED), "-G", G],
                                   stdout=null, check=True, env=dict(os.environ, PYTHONHASHSEED="0"))
                tt[G].append(time.time() - t)
                out[G] = open(nwk, "rb").read()
                print("  round %d -G %s: %.1f s" % (r, G, tt[G][-1]))
                sys.stdout.flush()
        if tt["T"]:
            line("pan_genome.py -t -B %d -G T (the whole command)" % B, tt["T"])
        line("pan_genome.py -t -B %d -G F (the whole command)" % B, tt["F"], "the two trees are the same bytes: %s" % (out["T"] == out["F"]) if tt["T"] else "")
