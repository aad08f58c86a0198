"""What `find_cluster -a mcl -G A` and pipeline.groups_from_search() move, on BASELINE config 5 (100k-protein find_hit -> find_orth ->
find_cluster -a mcl -I 1.5):
  (a) the plan in front of the batches, in one process and alternating: numpy row_plan() behind the device component stage -- the lines
      the parent commit ran inside cnc() -- against device_row_plan(), one device call;
  (b) the command `find_cluster.py -a mcl -I 1.5` with -G M and -G A, process start to exit, alternating, fresh processes;
  (c) the one-process path groups_from_search() against the three commands on the same FASTA file (with their defaults, and with the
      device switches the parent commit had: find_orth -G R, find_cluster -G M), with its stage times.
  python tools/diag/cnc_plan_cost.py <work dir> [proteins] [rounds]
The yardstick is the parent's path in the same call, never the new code against itself.  Leaves <work dir>/x.opc behind."""
import collections, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from swiftortho_amd import find_cluster as fc, pipeline, synthprot

tmp = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 9
os.makedirs(tmp, exist_ok=True)
meta = json.load(open(os.path.join(ROOT, "tests", "golden", "pipe_c3.json" if n == 100000 else "pipe_c2.json")))
d = dict(zip(meta["find_hit_flags"][0::2], meta["find_hit_flags"][1::2]))
p, sc, op = os.path.join(tmp, "x.fsa"), os.path.join(tmp, "x.sc"), os.path.join(tmp, "x.opc")
py = sys.executable
find_hit = [py, os.path.join(ROOT, "bin", "find_hit.py"), "-p", "blastp", "-i", p, "-d", p, "-o", sc, "-a", "1", "-e", d["-e"], "-v", d["-v"], "-j", d["-j"], "-F", d["-F"],
            "-s", d["-s"], "-r", "aa9", "-M", d["-M"], "-c", d["-c"]]
find_orth = [py, os.path.join(ROOT, "bin", "find_orth.py"), "-i", sc]
find_cluster = [py, os.path.join(ROOT, "bin", "find_cluster.py"), "-i", op, "-a", "mcl", "-I", "1.5"]
if not os.path.isfile(op):
    open(p, "wb").write(synthprot.synthprot(n, 300))
    subprocess.run(find_hit, check=True)
    open(op, "wb").write(subprocess.run(find_orth, capture_output=True, check=True).stdout)

clock = time.perf_counter
med = lambda v: sorted(v)[len(v) // 2]
line = lambda k, v: print("%-58s min %.4f s  median %.4f s  spread (max - min) %.4f s  (%d runs)" % (k, min(v), med(v), max(v) - min(v), len(v)))

# ---- (a) the plan ---------------------------------------------------------------------------------------------------------------------
names, cx, cy, Z, ztext = fc._edge_columns(open(op))
took, info = collections.defaultdict(list), {}
for r in range(rounds + 1):   # round 0 warms up (HIP runtime, code object, allocator)
    t = clock(); a = fc.row_plan(cx, cy, Z, len(names), groups=fc._device_stage); ta = clock() - t
    t = clock(); b = fc.device_row_plan(cx, cy, Z, len(names), info=info); tb = clock() - t
    t = clock(); g = fc.device_group_numbers(a.X, a.Y, Z, len(a.gene_code)); tg = clock() - t
    if r:
        took["(a) numpy row_plan() behind device_group_numbers (parent)"].append(ta)
        took["    of which device_group_numbers"].append(tg)
        took["(a) device_row_plan()"].append(tb)
same = all(np.array_equal(getattr(a, f), getattr(b, f)) for f in fc.RowPlan.FIELDS)
print("%d proteins: %d rows, %d codes, %d genes, %d kept rows, %d cut(s), %d tied;  every field identical: %s" % (n, len(cx), len(names), len(a.gene_code), len(a.order), len(a.cut),
                                                                                                                len(a.tied), same))
print("device_row_plan: %s" % " ".join("%s=%d" % kv for kv in sorted(info.items())))
print("== (a) the plan in front of the batches, one process, alternating, round 0 (warm-up) not counted ==")
for k, v in took.items():
    line(k, v)
print("moved: up %.1f MB (codes and weights), down %.1f MB (gene numbers, order, component and group numbers)" % (len(cx) * 16 / 1e6, (len(cx) * 8 + len(a.order) * 4 + len(a.gene_code) * 12) / 1e6))

# ---- (b) the command ------------------------------------------------------------------------------------------------------------------
print("== (b) find_cluster.py -i x.opc -a mcl -I 1.5 -G M|A, process start to exit, fresh processes, alternating ==")
runs = max(rounds, 9)
wall, outs = collections.defaultdict(list), {}
for r in range(runs):
    for g in ("M", "A"):
        t = clock()
        outs[g] = subprocess.run(find_cluster + ["-G", g], capture_output=True, check=True).stdout
        wall[g].append(clock() - t)
for g in ("M", "A"):
    line("find_cluster.py -a mcl -I 1.5 -G %s (%d groups)" % (g, outs[g].count(b"\n")), wall[g])
    print("    every run: %s" % " ".join("%.3f" % v for v in wall[g]))
print("difference of the medians (M - A): %.4f s;  output identical: %s" % (med(wall["M"]) - med(wall["A"]), outs["M"] == outs["A"]))

# ---- (c) the one-process path ---------------------------------------------------------------------------------------------------------
print("== (c) FASTA file -> groups: the three commands against one process (pipeline.groups_from_search), alternating ==")
kw = dict(ssd=d["-s"], nr=d["-r"], ht=int(d["-M"]), chk=int(d["-c"]), step=int(d["-j"]), v=int(d["-v"]), expect=float(d["-e"]), flt=d["-F"])
one = os.path.join(tmp, "one_process.py")
open(one, "w").write("import sys, json\nsys.path.insert(0, %r)\nfrom swiftortho_amd import pipeline\ngroups, t = pipeline.groups_from_search(%r, **%r)\n"
                     "sys.stdout.write(''.join('\\t'.join(g) + '\\n' for g in groups))\nsys.stderr.write(json.dumps(t))\n" % (ROOT, p, kw))


def three(orth_flags, cluster_flags):
    t = clock()
    subprocess.run(find_hit, check=True, capture_output=True)
    t1 = clock()
    open(op, "wb").write(subprocess.run(find_orth + orth_flags, capture_output=True, check=True).stdout)
    t2 = clock()
    out = subprocess.run(find_cluster + cluster_flags, capture_output=True, check=True).stdout
    t3 = clock()
    return t3 - t, (t1 - t, t2 - t1, t3 - t2), out


wall, parts, stage = collections.defaultdict(list), {}, {}
for r in range(max(3, rounds // 3)):
    w, parts["three commands, defaults"], out0 = three([], [])
    wall["three commands, defaults"].append(w)
    w, parts["three commands, find_orth -G R, find_cluster -G M"], out1 = three(["-G", "R"], ["-G", "M"])
    wall["three commands, find_orth -G R, find_cluster -G M"].append(w)
    t = clock()
    r1 = subprocess.run([py, one], capture_output=True, check=True)
    wall["one process: groups_from_search()"].append(clock() - t)
    stage = json.loads(r1.stderr.decode().strip().splitlines()[-1])
for k, v in wall.items():
    line(k, v)
    if k in parts:
        print("    last run: find_hit %.3f  find_orth %.3f  find_cluster %.3f" % parts[k])
print("    groups_from_search() stage times of the last run: %s" % "  ".join("%s %s" % (k, ("%.3f" % v) if isinstance(v, float) else v) for k, v in stage.items()))
print("output identical: %s (%d groups)" % (out0 == out1 == r1.stdout, r1.stdout.count(b"\n")))
