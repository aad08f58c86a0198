"""What follows the candidate tables of find_orth on BASELINE config 5's hit records (100k-protein self-search), host and device side by side,
in one process and alternating:
  (a) the path without the relations kernels: device_candidates_from_records() with its eight downloads | numpy relation_tables() |
      lines_from_tables() -- each timed on its own (how the host part divides between tables and text);
  (b) device_relation_tables_from_records() | lines_from_tables();
then orthology_from_search() with device_stage=True against device_stage='relations'.
  python tools/diag/orth_rel_cost.py [proteins] [rounds] [--trace]
(a) is the yardstick, never (b).  --trace: only the search and the relations call, for a profiler run of its own
(rocprofv3 --kernel-trace --stats -- python tools/diag/orth_rel_cost.py 100000 3 --trace)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from swiftortho_amd import find_orth as fo, fsearch, pipeline, synthprot

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else 100000
rounds = int(args[1]) if len(args) > 1 else 5
trace = "--trace" in sys.argv
meta = json.load(open(os.path.join(ROOT, "tests", "golden", "pipe_c3.json" if n == 100000 else "pipe_c2.json")))
d = dict(zip(meta["find_hit_flags"][0::2], meta["find_hit_flags"][1::2]))
kw = dict(ssd=d["-s"], nr=d["-r"], ht=int(d["-M"]), chk=int(d["-c"]), step=int(d["-j"]), v=int(d["-v"]), expect=float(d["-e"]), flt=d["-F"])
fa = synthprot.synthprot(n, 300)
ids = fo.fasta_ids(fa)
s = fsearch.Searcher(**kw)
s.load_ref_bytes(fa)
s.load_queries_bytes(fa)
dev = s.search_device()
print("%d proteins, %d hit records resident (%d MB)" % (n, len(dev), len(dev) * 80 >> 20))
if trace:
    for _ in range(rounds):
        fo.device_relation_tables_from_records(dev, ids, ids)
    s.close()
    sys.exit(0)
box = {}


def a_candidates():
    box["names"], box["tax"], box["taxa"], box["cand"] = fo._device_records(dev, ids, ids, .5, 0., "no", "|")


def a_tables():
    box["a_tables"] = fo.relation_tables(box["names"], box["tax"], box["taxa"], box["cand"])


def a_text():
    box["a_lines"] = fo.lines_from_tables(box["names"], box["a_tables"])


def b_relations():
    box["b_names"], box["b_tables"] = fo.device_relation_tables_from_records(dev, ids, ids)


def b_text():
    box["b_lines"] = fo.lines_from_tables(box["b_names"], box["b_tables"])


stages = [("(a) device_candidates_from_records(), 8 tables down", a_candidates), ("(a) numpy relation_tables()", a_tables), ("(a) lines_from_tables()", a_text),
          ("(b) device_relation_tables_from_records()", b_relations), ("(b) lines_from_tables()", b_text)]
times = {k: [] for k, _ in stages}
for r in range(rounds + 1):   # round 0 warms up (allocator, code objects)
    for k, f in stages:
        t = time.time(); f(); dt = time.time() - t
        if r:
            times[k].append(dt)
A, B, cand = box["a_tables"], box["b_tables"], box["cand"]
same = all(np.array_equal(getattr(A, k).view(np.int64), getattr(B, k).view(np.int64)) for k in fo.RelationTables.FIELDS)
print("%d in-paralog, %d ortholog, %d co-ortholog rows from %d / %d / %d candidate rows, %d names, %d taxa;  tables identical to numpy: %s;  lines identical: %s"
      % (len(A.ip_a), len(A.ot_a), len(A.co_a), len(cand.ip_a), len(cand.ot_a), len(cand.co_key), len(box["names"]), len(box["taxa"]), same, box["a_lines"] == box["b_lines"]))
for k, _ in stages:
    print("%-54s min %.4f s  median %.4f s  (%d rounds)" % (k, min(times[k]), sorted(times[k])[len(times[k]) // 2], rounds))
tot = lambda p: sum(min(times[k]) for k, _ in stages if k.startswith(p))
print("sum of minima: (a) %.4f s   (b) %.4f s" % (tot("(a)"), tot("(b)")))
tt = []
for r in range(rounds):
    t = time.time(); fo._record_maps(ids, ids); fo._taxa(box["names"], "|"); tt.append(time.time() - t)
print("%-54s min %.4f s  (name codes and taxa on the host: part of both records calls above)" % ("_record_maps() + _taxa()", min(tt)))
# the relations kernels, every array once per pass that needs it (the radix sorts' own passes in between are not counted): the in-paralog table
# read by the forward flags (16 B a row), by the emit (8 B), and its forward half gathered by the normaliser and the two emit passes (3 x 24 B)
# with the 12 B (key, row) lists written, read by the sort, written sorted, read; per ortholog row the two gene codes read (16 B), five 4 B
# words written, the counts scanned (8 B); per product 28 B read of the pair's words and 12 B of flag / position written, scanned (8 B) and read
# (12 B); per section row before the repeat rule 24 B read, the pair sort's 12 B lists four times, 12 B of flags / scan; per kept row 24 B + 12 B
# written, the group sort's lists, 16 B gathered twice and 8 B written; the three tables out (24 B a row)
fwd = int(np.sum(cand.ip_a < cand.ip_b))
lo, hi = np.searchsorted(cand.ip_a, cand.ot_a, "left"), np.searchsorted(cand.ip_a, cand.ot_a, "right")
lo2, hi2 = np.searchsorted(cand.ip_a, cand.ot_b, "left"), np.searchsorted(cand.ip_a, cand.ot_b, "right")
nq, ns = hi - lo, hi2 - lo2
products = int(np.sum(np.where((nq > 0) | (ns > 0), (nq + 1) * (ns + 1), 0)))
n_ot, n_cb = len(cand.ot_a), len(A.co_a)   # (co-ortholog rows before the repeat rule: not known to the host; the kept ones stand in)
parts = (("in-paralogs", len(cand.ip_a) * 24 + fwd * (3 * 24 + 4 * 12 + 24)), ("ortholog pairs", n_ot * (16 + 20 + 8)), ("products", products * (28 + 12 + 8 + 12)),
         ("sections", (n_ot + n_cb) * (24 + 12 + 36 + 4 * 12 + 2 * 16 + 8) + n_cb * 4 * 12), ("tables out", (len(A.ip_a) + len(A.ot_a) + len(A.co_a)) * 24))
traffic = sum(b for _, b in parts)
print("%d forward in-paralog pairs, %d co-ortholog products" % (fwd, products))
print("algorithmic traffic of the relations kernels: %.1f MB = %.1f us at 8 TB/s  (%s)" % (traffic / 1e6, traffic / 8e6, ", ".join("%s %.1f" % (k, b / 1e6) for k, b in parts)))
s.close()
p = os.path.join(__import__("tempfile").mkdtemp(), "x.fsa")
open(p, "wb").write(fa)
print("== orthology_from_search(), device_stage=True / 'relations', alternating ==")
for r in range(3):
    for stage in (True, "relations"):
        lines2, tm = pipeline.orthology_from_search(p, device_stage=stage, **kw)
        print("device_stage=%r" % (stage,), {k: round(v, 3) if isinstance(v, float) else v for k, v in tm.items()}, "relations identical:", lines2 == box["a_lines"])
