"""The phyletic-profile stage in one warm process: so_phyletic_pairs (the whole device call, and its count pass, emit pass and sort split by
events) against the numpy definition swiftortho_amd/phyletic.py linked_pairs(), on `rows` families x `taxa` genomes in `modules` modules --
family e carries module e % modules' random profile (every genome with probability 1 / 2) with genome (e // modules) % taxa flipped, the
table of tests/phyletic_inputs.py module_bits() --, every family eligible, at Jaccard 4/5 and two shared genomes.
    python tools/diag/phyletic_cost.py [rows] [taxa] [modules] [rounds] [sample]
Defaults: 200000 rows x 500 taxa, 2000 modules, 9 rounds after a warm call; the definition is timed on the first `sample` (4000) rows and
scaled by (rows / sample)^2 -- its product is quadratic in the rows --, not run on all of them."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from swiftortho_amd import pan, phyletic
sys.path.insert(0, os.path.join(ROOT, "tests"))
from phyletic_inputs import module_bits      # the table of the tests, not a copy of it

args = [int(x) for x in sys.argv[1:] if x.isdigit()]
R = args[0] if args else 200000
T = args[1] if len(args) > 1 else 500
M = args[2] if len(args) > 2 else 2000
rounds = args[3] if len(args) > 3 else 9
sample = min(args[4] if len(args) > 4 else 4000, R)
NUM, DEN, K_MIN = 4, 5, 2


def line(name, tt, note=""):
    tt = sorted(tt)
    print("%-52s min %9.3f ms  median %9.3f ms  (%d runs)  %s" % (name, tt[0], tt[len(tt) // 2], len(tt), note))
    sys.stdout.flush()


bits = module_bits(R, T, M)
r, t = np.nonzero(bits)
table = pan.MemberTable(r.astype(np.int32), t.astype(np.int32), R, R)
print("%d families x %d genomes in %d modules, %d members; Jaccard >= %d/%d, shared >= %d, every family eligible" % (R, T, M, len(r), NUM, DEN, K_MIN))

small = pan.MemberTable(table.row[:8], table.taxon[:8], R, R)
phyletic.device_linked_pairs(small, T, 1, T, K_MIN, NUM, DEN)          # warm-up: the library, the device, the code objects
phyletic.device_linked_pairs(table, T, 1, T, K_MIN, NUM, DEN)          # a warm call on the input itself
wall, ev = [], []
for _ in range(rounds):
    st = {}
    t0 = time.time()
    links = phyletic.device_linked_pairs(table, T, 1, T, K_MIN, NUM, DEN, stats=st, timed=True)
    wall.append((time.time() - t0) * 1e3), ev.append(st)
line("so_phyletic_pairs (upload, passes, sort, copy back)", wall, "%d pairs, %d eligible, %d tile pairs, %d waits" % (len(links.a), st["n_eligible"], st["tiles"], st["waits"]))
for k in ("count_ms", "emit_ms", "sort_ms"):
    line("  ... %s (events)" % k[:-3], [e[k] for e in ev])
pair_words = st["n_eligible"] * (st["n_eligible"] - 1) // 2 * ((T + 63) // 64)
print("  the count pass: %.3e family pairs x %d taxon words in %.3f ms = %.3e pair-words / s" % (st["n_eligible"] * (st["n_eligible"] - 1) / 2., (T + 63) // 64,
                                                                                         min(e["count_ms"] for e in ev), pair_words / (min(e["count_ms"] for e in ev) * 1e-3)))

rs = np.flatnonzero(table.row < sample)
sub = pan.MemberTable(table.row[rs], table.taxon[rs], sample, sample)
tt = []
for _ in range(3):
    t0 = time.time()
    want = phyletic.linked_pairs(sub, T, 1, T, K_MIN, NUM, DEN)
    tt.append((time.time() - t0) * 1e3)
scale = (R / float(sample)) ** 2
line("numpy: linked_pairs on the first %d rows" % sample, tt, "x %.0f = %.1f s for %d rows (scaled, not run)" % (scale, min(tt) * scale / 1e3, R))
keep = links.b < sample
same = np.array_equal(links.a[keep], want.a) and np.array_equal(links.b[keep], want.b) and np.array_equal(links.shared[keep], want.shared)
print("the device's pairs among the first %d rows are the definition's: %s (%d pairs)" % (sample, same, len(want.a)))
