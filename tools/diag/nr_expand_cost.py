"""What pipeline.orthology_from_search(collapse=True) moves, on the config-3 generator's proteins with a seeded tenth of the records
duplicated (exact copies under new ids):
  (a) FASTA file -> relations: the parent commit's only route -- nr.search_collapsed() (nr_flt, bin/find_hit.py, nr2full through two text
      files) followed by bin/find_orth.py -- against ONE process, orthology_from_search(collapse=True, device_stage='relations');
      fresh processes, alternating;
  (b) the expansion alone on the rows of that search, one warm process: nr.device_expand() (so_nr_expand) against the host nr2full() on
      the text of the same rows;
  (c) nr.collapse_tables() against nr.nr_flt() on the same file.
  python tools/diag/nr_expand_cost.py <work dir> [proteins] [runs]
The parent's path is the yardstick in every part."""
import collections, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from swiftortho_amd import fsearch, nr, synthprot

tmp = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 9
os.makedirs(tmp, exist_ok=True)
SEED, HITS = "111111", "500"
py = sys.executable
clock = time.perf_counter
med = lambda v: sorted(v)[len(v) // 2]
line = lambda k, v: print("%-66s min %.4f s  median %.4f s  spread (max - min) %.4f s  (%d runs)" % (k, min(v), med(v), max(v) - min(v), len(v)))

# the set: every record of the generator, and a copy of a seeded tenth of them under new ids, shuffled into the file
fas = os.path.join(tmp, "x.fsa")
rs = np.random.RandomState(12345)
rec = synthprot.synthprot(n, 300).split(b">")[1:]
pick = rs.choice(len(rec), len(rec) // 10, replace=False)
new = [b"t%04d|c%07d\n" % (k % max(2, n // 2000), k) + rec[s].split(b"\n", 1)[1] for k, s in enumerate(pick.tolist())]
both = rec + new
data = b"".join(b">" + both[i] for i in rs.permutation(len(both)))
open(fas, "wb").write(data)
print("%d proteins + %d exact copies = %d records, %.1f MB" % (n, len(new), len(both), len(data) / 1e6))

# ---- (a) end to end ---------------------------------------------------------------------------------------------------------------------
chain = os.path.join(tmp, "chain.py")
open(chain, "w").write("import sys\nsys.path.insert(0, %r)\nfrom swiftortho_amd import nr\nprint(nr.search_collapsed(%r, seed=%r, cpus='1', hits=%r))\n" % (ROOT, fas, SEED, HITS))
one = os.path.join(tmp, "one.py")
open(one, "w").write("import sys, json\nsys.path.insert(0, %r)\nfrom swiftortho_amd import nr, pipeline\n"
                     "lines, t = pipeline.orthology_from_search(%r, device_stage='relations', collapse=True, **nr.collapsed_search_kw(%r, %r))\n"
                     "sys.stdout.buffer.write(b'\\n'.join(lines) + b'\\n')\nsys.stderr.write(json.dumps(t))\n" % (ROOT, fas, SEED, HITS))
wall, parts, stage = collections.defaultdict(list), None, {}
print("== (a) FASTA file -> relations: search_collapsed() + find_orth.py (the parent commit's route) against one process, fresh processes, alternating ==")
for r in range(runs):
    t = clock()
    sc = subprocess.run([py, chain], capture_output=True, check=True, text=True).stdout.strip().splitlines()[-1]
    t1 = clock()
    out0 = subprocess.run([py, os.path.join(ROOT, "bin", "find_orth.py"), "-i", sc], capture_output=True, check=True).stdout
    t2 = clock()
    wall["search_collapsed() + bin/find_orth.py (parent)"].append(t2 - t)
    parts = (t1 - t, t2 - t1)
    t = clock()
    r1 = subprocess.run([py, one], capture_output=True, check=True)
    wall["one process: orthology_from_search(collapse=True, 'relations')"].append(clock() - t)
    stage = json.loads(r1.stderr.decode().strip().splitlines()[-1])
for k, v in wall.items():
    line(k, v)
    print("    every run: %s" % " ".join("%.3f" % x for x in v))
print("    parent, last run: search_collapsed %.3f  find_orth %.3f" % parts)
print("    one process, stage times of the last run: %s" % "  ".join("%s %s" % (k, ("%.3f" % v) if isinstance(v, float) else v) for k, v in stage.items()))
print("output identical: %s (%d relations)" % (out0 == r1.stdout, out0.count(b"\n")))

# ---- (b) the expansion alone ------------------------------------------------------------------------------------------------------------
print("== (b) the rows of the collapsed search -> the expanded rows: device_expand() against nr2full() on their text, one warm process ==")
tables = nr.collapse_tables(data)
s = fsearch.Searcher(**nr.collapsed_search_kw(SEED, HITS))
s.load_ref_bytes(tables.fasta)
s.load_queries_bytes(tables.fasta)
dev = s.search_device()
took = collections.defaultdict(list)
for r in range(runs + 1):   # round 0 warms up
    t = clock()
    e = nr.device_expand(dev, tables)
    t1 = clock()
    rows_out, waits = len(e), e.waits
    e.close()
    if r:
        took["device_expand() (so_nr_expand), records stay in HBM"].append(t1 - t)
nr_sc = os.path.join(fas + "_results", "x.fsa_nr.fsa.sc")
text = open(nr_sc).readlines()
for r in range(3):
    t = clock()
    full = nr.nr2full(text)
    took["nr2full() on the text rows (parent; without reading / writing the files)"].append(clock() - t)
s.close()
for k, v in took.items():
    line(k, v)
print("%d collapsed rows -> %d expanded rows (%d by nr2full), %.1f MB of records written, %d host waits" % (len(dev), rows_out, len(full), rows_out * 80 / 1e6, waits))

# ---- (c) the collapse -------------------------------------------------------------------------------------------------------------------
print("== (c) the collapse of the %d records, one process, alternating ==" % len(both))
took = collections.defaultdict(list)
for r in range(runs):
    t = clock()
    lines = nr.nr_flt(open(fas, "r"))
    t1 = clock()
    tb = nr.collapse_tables(open(fas, "rb").read())
    t2 = clock()
    took["nr_flt() (parent)"].append(t1 - t)
    took["collapse_tables()"].append(t2 - t1)
for k, v in took.items():
    line(k, v)
print("same collapsed FASTA: %s (%d distinct sequences)" % ("".join(l + "\n" for l in lines).encode() == tb.fasta, len(tb.off) - 1))
