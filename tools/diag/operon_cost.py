"""The operon-pair stage on a synthetic operon table in one warm process, alternating: the device call in both modes
(operon.device_operon_pairs: so_operon_pairs, passing pairs in index order | all candidates in first-occurrence order) | the numpy
definition (operon.candidate_pairs) | the host set replay and filter behind the candidates (operon.reference_order + passes + scores);
minimum and median of the rounds after a warm-up round, with the call's counters.
    python tools/diag/operon_cost.py [taxa] [operons per taxon] [rounds] [--no-device]
Generator (numpy RandomState(7)): every operon holds 2 .. 7 distinct families; the first operon of every taxon holds family 1 (one
family present in every taxon), the other families are drawn from a long tail (weight 1 / (rank + 400) over 40 families per taxon).  Half the
operons hold a gene of family 0, lengths are the slice length plus 0 .. 2.  Defaults: 300 taxa x 300 operons, 9 rounds."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from swiftortho_amd import operon

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n_taxa = int(args[0]) if args else 300
n_per = int(args[1]) if len(args) > 1 else 300
rounds = int(args[2]) if len(args) > 2 else 9
use_device = "--no-device" not in sys.argv

rng = np.random.RandomState(7)
n_ops, n_fam = n_taxa * n_per, 2 + 40 * n_taxa
w = 1. / (400. + np.arange(1, n_fam - 1))
cdf = np.cumsum(w / w.sum())
size = rng.randint(2, 8, size=n_ops)
draw = 2 + np.minimum(np.searchsorted(cdf, rng.rand(n_ops, 7)), n_fam - 3)      # families 2 .. n_fam - 1, a long tail
draw[::n_per, 0] = 1                                                           # one family present in every taxon
start, fam = [0], []
for k in range(n_ops):
    f = list(dict.fromkeys(draw[k, :size[k]].tolist()))
    fam += f
    start.append(len(fam))
start, fam = np.asarray(start, dtype=np.int64), np.asarray(fam, dtype=np.int32)
length = (np.diff(start) + rng.randint(0, 3, size=n_ops)).astype(np.int32)
table = operon.OperonTable(None, length, (rng.rand(n_ops) < .5).astype(np.uint8), start, fam, n_fam)
fsize = np.bincount(fam, minlength=n_fam)
print("%d operons (%d taxa x %d), %d families, %d entries; largest family lists: %s; expansions %d" %
      (n_ops, n_taxa, n_per, n_fam, len(fam), np.sort(fsize)[::-1][:5].tolist(), int((fsize.astype(np.int64) ** 2).sum())))


def replay(c):
    o = operon.reference_order(c.cand_start, c.j)
    i, j, n = c.i[o], c.j[o], c.nshr[o]
    keep = operon.passes(n, length[i], length[j])
    return i[keep], j[keep], operon.scores(n[keep], length[i[keep]], length[j[keep]])


dev = lambda flags: operon.device_operon_pairs(start, fam, length, table.has0, n_fam, flags)
stages = [("numpy definition (candidate_pairs)", lambda: operon.candidate_pairs(table))]
if use_device:
    stages = [("device call, passing pairs by (i, j)", lambda: dev(0)), ("device call, all candidates", lambda: dev(1))] + stages
res, times = {}, {k: [] for k, _ in stages}
times["host set replay, filter and score"] = []
for r in range(rounds + 1):     # round 0 warms up (allocator, code objects)
    for k, f in stages:
        t = time.time(); res[k] = f(); dt = time.time() - t
        if r:
            times[k].append(dt)
    t = time.time(); ref = replay(res["numpy definition (candidate_pairs)"]); dt = time.time() - t
    if r:
        times["host set replay, filter and score"].append(dt)
    sys.stderr.write("round %d done\n" % r), sys.stderr.flush()
base = res["numpy definition (candidate_pairs)"]
keep = np.flatnonzero(operon.passes(base.nshr, length[base.i], length[base.j]))
keep = keep[np.lexsort((base.j[keep], base.i[keep]))]
for k in times:
    v = sorted(times[k])
    g = res.get(k)
    if g is None:
        note = "%d lines" % len(ref[0])
    elif k.startswith("device call, passing"):
        note = "identical to numpy: %s  %s" % (all(np.array_equal(getattr(g, n), getattr(base, n)[keep]) for n in ("i", "j", "nshr")), g.stats)
    else:
        note = "identical to numpy: %s  %s" % (all(np.array_equal(getattr(g, n), getattr(base, n)) for n in ("i", "j", "nshr", "cand_start")), g.stats or "")
    print("%-40s min %.4f s  median %.4f s  max %.4f s  (%d rounds)  %s" % (k, v[0], v[len(v) // 2], v[-1], len(v), note))
print("candidates %d, passing %d, self pairs %d" % (len(base.i), len(keep), int((base.i == base.j).sum())))
