"""What `find_cluster -a apc -G A` moves, on BASELINE config 5's relations (100k-protein find_hit -> find_orth):
  (a) apc_entries() + device_apc() -- tokeniser, entry list in numpy, grouping on the host, upload, loop, download of R and A: the lines
      the parent commit ran -- against the tokeniser + device_apc_rows() (rows up, numbering, layout and loop on the device, gene codes
      and labels down), alternating in one warm process;
  (b) the command `find_cluster.py -a apc` against `-a apc -G A`, process start to exit, fresh processes, alternating -- and, with a built
      checkout of the parent commit as the fourth argument, the parent's own `find_cluster.py -a apc` in the same alternation;
  (c) the three commands find_hit, find_orth, find_cluster -a apc [-G A] against pipeline.groups_from_search(algorithm='apc') in one
      process, on the same FASTA file, alternating.
  python tools/diag/apc_rows_cost.py <work dir> [proteins] [runs] [parent checkout]
The parent's path is the yardstick in every part.  Leaves <work dir>/x.opc behind for a profiler run of the command."""
import collections, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from swiftortho_amd import find_cluster as fc, synthprot

tmp = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 9
parent = sys.argv[4] if len(sys.argv) > 4 else None
os.makedirs(tmp, exist_ok=True)
meta = json.load(open(os.path.join(ROOT, "tests", "golden", "pipe_c3.json" if n == 100000 else "pipe_c2.json")))
d = dict(zip(meta["find_hit_flags"][0::2], meta["find_hit_flags"][1::2]))
p, sc, op = os.path.join(tmp, "x.fsa"), os.path.join(tmp, "x.sc"), os.path.join(tmp, "x.opc")
py = sys.executable
find_hit = [py, os.path.join(ROOT, "bin", "find_hit.py"), "-p", "blastp", "-i", p, "-d", p, "-o", sc, "-a", "1", "-e", d["-e"], "-v", d["-v"], "-j", d["-j"], "-F", d["-F"],
            "-s", d["-s"], "-r", "aa9", "-M", d["-M"], "-c", d["-c"]]
find_orth = [py, os.path.join(ROOT, "bin", "find_orth.py"), "-i", sc]
find_cluster = [py, os.path.join(ROOT, "bin", "find_cluster.py"), "-i", op, "-a", "apc"]
if not os.path.isfile(op):
    open(p, "wb").write(synthprot.synthprot(n, 300))
    subprocess.run(find_hit, check=True)
    open(op, "wb").write(subprocess.run(find_orth, capture_output=True, check=True).stdout)

clock = time.perf_counter
med = lambda v: sorted(v)[len(v) // 2]
line = lambda k, v: print("%-58s min %.4f s  median %.4f s  spread (max - min) %.4f s  (%d runs)" % (k, min(v), med(v), max(v) - min(v), len(v)))

# ---- (a) from the text to the labels, one warm process -----------------------------------------------------------------------------------
data = open(op, "rb").read()
took, info = collections.defaultdict(list), {}
for r in range(runs + 1):   # round 0 warms up (HIP runtime, code object, allocator)
    t = clock(); names, row, col, score, ng = fc.apc_entries(data); t1 = clock(); lab_a = fc.device_apc(row, col, score, ng, 0.5)[0]; t2 = clock()
    kind, ids, cx, cy, z = fc._apc_input(data); t3 = clock(); tax = fc._taxon_codes(ids)[0]; t4 = clock()
    gene_code, lab_b = fc.device_apc_rows(cx, cy, z, len(ids), tax, 0.5, info=info); t5 = clock()
    if r:
        took["(a) apc_entries() + device_apc() (parent)"].append(t2 - t)
        took["    of which apc_entries()"].append(t1 - t)
        took["    of which device_apc()"].append(t2 - t1)
        took["(a) tokeniser + taxon codes + device_apc_rows()"].append(t5 - t2)
        took["    of which the tokeniser"].append(t3 - t2)
        took["    of which the taxon codes"].append(t4 - t3)
        took["    of which device_apc_rows()"].append(t5 - t4)
same = kind == "columns" and [ids[c] for c in gene_code.tolist()] == names and np.array_equal(lab_a, lab_b)
deg = np.bincount(row, minlength=ng)
print("%d proteins: %d rows, %d codes, %d genes, %d entries, longest row %d, rows above 32 entries: %d;  genes and labels identical: %s"
      % (n, len(cx), len(ids), ng, len(row), deg.max(), int((deg > 32).sum()), same))
print("device_apc_rows: %s" % " ".join("%s=%d" % kv for kv in sorted(info.items())))
print("== (a) relation text -> exemplar labels, 100 rounds, one process, alternating, round 0 (warm-up) not counted ==")
for k, v in took.items():
    line(k, v)
print("moved: (parent) up %.1f MB (layout and scores), down %.1f MB (labels, R and A);  (-G A) up %.1f MB (codes, weights, taxa), down %.1f MB (gene codes and labels)"
      % (len(row) * 20 / 1e6 + ng * 24 / 1e6, (len(row) * 8 + ng * 4) / 1e6, (len(cx) * 16 + len(ids) * 4) / 1e6, ng * 8 / 1e6))

# ---- (b) the command ------------------------------------------------------------------------------------------------------------------
print("== (b) find_cluster.py -i x.opc -a apc [-G A], process start to exit, fresh processes, alternating ==")
cmds = [("find_cluster.py -a apc", find_cluster), ("find_cluster.py -a apc -G A", find_cluster + ["-G", "A"])]
if parent:
    cmds.insert(0, ("parent commit: find_cluster.py -a apc", [py, os.path.join(parent, "bin", "find_cluster.py"), "-i", op, "-a", "apc"]))
wall, outs = collections.defaultdict(list), {}
for r in range(max(runs, 9)):
    for k, c in cmds:
        t = clock()
        outs[k] = subprocess.run(c, capture_output=True, check=True).stdout
        wall[k].append(clock() - t)
for k, _ in cmds:
    line("%s (%d groups)" % (k, outs[k].count(b"\n")), wall[k])
    print("    every run: %s" % " ".join("%.3f" % v for v in wall[k]))
print("difference of the medians (%s - -G A): %.4f s;  output identical: %s" % (cmds[0][0], med(wall[cmds[0][0]]) - med(wall[cmds[-1][0]]), len(set(outs.values())) == 1))

# ---- (c) the one-process path ---------------------------------------------------------------------------------------------------------
print("== (c) FASTA file -> groups: the three commands against one process (pipeline.groups_from_search(algorithm='apc')), alternating ==")
kw = dict(ssd=d["-s"], nr=d["-r"], ht=int(d["-M"]), chk=int(d["-c"]), step=int(d["-j"]), v=int(d["-v"]), expect=float(d["-e"]), flt=d["-F"], algorithm="apc")
one = os.path.join(tmp, "one_process_apc.py")
open(one, "w").write("import sys, json\nsys.path.insert(0, %r)\nfrom swiftortho_amd import pipeline\ngroups, t = pipeline.groups_from_search(%r, **%r)\n"
                     "sys.stdout.write(''.join('\\t'.join(g) + '\\n' for g in groups))\nsys.stderr.write(json.dumps(t))\n" % (ROOT, p, kw))


def three(cluster_flags):
    t = clock()
    subprocess.run(find_hit, check=True, capture_output=True)
    t1 = clock()
    open(op, "wb").write(subprocess.run(find_orth, capture_output=True, check=True).stdout)
    t2 = clock()
    out = subprocess.run(find_cluster + cluster_flags, capture_output=True, check=True).stdout
    t3 = clock()
    return t3 - t, (t1 - t, t2 - t1, t3 - t2), out


wall, parts, stage = collections.defaultdict(list), {}, {}
for r in range(max(3, runs // 3)):
    w, parts["three commands, find_cluster -a apc"], out0 = three([])
    wall["three commands, find_cluster -a apc"].append(w)
    w, parts["three commands, find_cluster -a apc -G A"], out1 = three(["-G", "A"])
    wall["three commands, find_cluster -a apc -G A"].append(w)
    t = clock()
    r1 = subprocess.run([py, one], capture_output=True, check=True)
    wall["one process: groups_from_search(algorithm='apc')"].append(clock() - t)
    stage = json.loads(r1.stderr.decode().strip().splitlines()[-1])
for k, v in wall.items():
    line(k, v)
    if k in parts:
        print("    last run: find_hit %.3f  find_orth %.3f  find_cluster %.3f" % parts[k])
print("    groups_from_search() stage times of the last run: %s" % "  ".join("%s %s" % (k, ("%.3f" % v) if isinstance(v, float) else v) for k, v in stage.items()))
print("output identical: %s (%d groups)" % (out0 == out1 == r1.stdout, r1.stdout.count(b"\n")))
