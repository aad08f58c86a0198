"""What `find_cluster -a mcl -G M` moves, on BASELINE config 5's relations (100k-protein find_hit -> find_orth): the stages of cnc() with
the batches on the host path and on the device path, in one process and alternating:
  (a) block_matrix_arrays() + device_mcl() + surviving_pair_columns() -- the batch as the host runs it (and as the parent commit ran it:
      the lines are the same);
  (b) device_mcl_rows() -- rows up, matrix assembled, iterated and read out on the device, pairs down; and the same call with rounds=0,
      which leaves the assembly and the read-out alone;
both behind the device component stage.  Then the command `find_cluster.py -a mcl -I 1.5` with -G F, -G T and -G M, process start to
exit, alternating, in fresh processes.
  python tools/diag/mcl_rows_cost.py <work dir> [proteins] [rounds]
(a) is the yardstick, never (b).  Leaves <work dir>/x.opc behind for a profiler run of the command."""
import collections, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from swiftortho_amd import find_cluster as fc, synthprot

tmp = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
os.makedirs(tmp, exist_ok=True)
meta = json.load(open(os.path.join(ROOT, "tests", "golden", "pipe_c3.json" if n == 100000 else "pipe_c2.json")))
d = dict(zip(meta["find_hit_flags"][0::2], meta["find_hit_flags"][1::2]))
p, sc, op = os.path.join(tmp, "x.fsa"), os.path.join(tmp, "x.sc"), os.path.join(tmp, "x.opc")
py = sys.executable
if not os.path.isfile(op):
    open(p, "wb").write(synthprot.synthprot(n, 300))
    subprocess.run([py, os.path.join(ROOT, "bin", "find_hit.py"), "-p", "blastp", "-i", p, "-d", p, "-o", sc, "-a", "1", "-e", d["-e"], "-v", d["-v"], "-j", d["-j"], "-F", d["-F"],
                    "-s", d["-s"], "-r", "aa9", "-M", d["-M"], "-c", d["-c"]], check=True)
    open(op, "wb").write(subprocess.run([py, os.path.join(ROOT, "bin", "find_orth.py"), "-i", sc], capture_output=True, check=True).stdout)

clock = time.perf_counter
real = {k: getattr(fc, k) for k in ("block_matrix_arrays", "surviving_pair_columns", "device_mcl_rows", "device_mcl", "_device_stage")}
spent, marks, shape = collections.defaultdict(float), {}, {}


def timed(name, first=None):
    f = real[name]

    def wrapper(*a, **k):
        t = clock()
        if first:
            marks.setdefault(first, t)
        r = f(*a, **k)
        spent[name] += clock() - t
        marks[name + " end"] = clock()
        return r
    return wrapper


def mcl_rows(gx, gy, z, n_labels, inflation, **kw):
    shape.update(rows=shape.get("rows", 0) + len(gx), batches=shape.get("batches", 0) + 1)
    return timed("device_mcl_rows", "batches begin")(gx, gy, z, n_labels, inflation, **kw)


fc.block_matrix_arrays = timed("block_matrix_arrays", "batches begin")
fc.surviving_pair_columns = timed("surviving_pair_columns")
fc.device_mcl_rows = mcl_rows
STAGES = ["tokenising and numbering", "component stage (device)", "row order", "assembly", "upload + loop + download", "read-out", "rows to pairs (one call)",
          "components and names"]


def one_cnc(matrix):
    """cnc() once -> (seconds per stage, groups)"""
    spent.clear(), marks.clear(), shape.clear()
    t0 = clock()
    stage = timed("_device_stage", "stage begin")
    groups = fc.cnc(open(op), 1.5, mcl=timed("device_mcl"), groups=stage, device_stage="matrix" if matrix else True)
    t1 = clock()
    batch = spent["block_matrix_arrays"] + spent["device_mcl"] + spent["surviving_pair_columns"] + spent["device_mcl_rows"]
    return {"tokenising and numbering": marks["stage begin"] - t0, "component stage (device)": spent["_device_stage"],
            "row order": marks["batches begin"] - marks["_device_stage end"], "assembly": spent["block_matrix_arrays"], "upload + loop + download": spent["device_mcl"],
            "read-out": spent["surviving_pair_columns"], "rows to pairs (one call)": spent["device_mcl_rows"],
            "components and names": t1 - marks["batches begin"] - batch, "cnc()": t1 - t0}, groups


paths = [("(a) host batches", False), ("(b) device batches", True)]
times = {k: collections.defaultdict(list) for k, _ in paths}
out = {}
for r in range(rounds + 1):   # round 0 warms up (HIP runtime, code object, allocator)
    for k, matrix in paths:
        st, out[k] = one_cnc(matrix)
        if r:
            for s, v in st.items():
                times[k][s].append(v)
print("%d proteins: %d rows in %d batch(es), %d groups;  identical groups: %s" % (n, shape["rows"], shape["batches"], len(out[paths[0][0]]), out[paths[0][0]] == out[paths[1][0]]))
med = lambda v: sorted(v)[len(v) // 2]
print("== cnc() by stage, seconds, min / median of %d rounds, the two paths alternating ==" % rounds)
print("%-28s %-19s %-19s" % ("", paths[0][0], paths[1][0]))
for s in STAGES + ["cnc()"]:
    print("%-28s %s" % (s, " ".join("%7.4f / %7.4f  " % (min(times[k][s]), med(times[k][s])) for k, _ in paths)))

# the batch alone, on the rows of the last batch cnc() formed: the device call with and without the loop, the host path piece by piece
box = {}
fc.device_mcl_rows = lambda gx, gy, z, n_labels, inflation, **kw: box.update(b=(gx, gy, z, n_labels)) or real["device_mcl_rows"](gx, gy, z, n_labels, inflation, **kw)
fc.block_matrix_arrays, fc.surviving_pair_columns = real["block_matrix_arrays"], real["surviving_pair_columns"]
fc.cnc(open(op), 1.5, device_stage="matrix")
gx, gy, z, n_labels = box["b"]
labels = list(range(n_labels))
alone = collections.defaultdict(list)
for r in range(rounds + 1):
    t = clock(); m = real["block_matrix_arrays"](gx, gy, z, labels); a = clock() - t
    info = {}
    t = clock(); f = real["device_mcl"](*m[1:], 1.5, info=info); b = clock() - t
    t = clock(); pr = real["surviving_pair_columns"](*f); c = clock() - t
    info2 = {}
    t = clock(); g = real["device_mcl_rows"](gx, gy, z, n_labels, 1.5, info=info2); e = clock() - t
    t = clock(); real["device_mcl_rows"](gx, gy, z, n_labels, 1.5, rounds=0); e0 = clock() - t
    if r:
        for k, v in (("(a) block_matrix_arrays", a), ("(a) device_mcl", b), ("(a) surviving_pair_columns", c), ("(a) the three", a + b + c), ("(b) device_mcl_rows", e),
                     ("(b) device_mcl_rows, rounds=0", e0)):
            alone[k].append(v)
print("== the last batch alone: %d rows, %d genes, %d matrix entries in, %d out, %d pairs;  %d rounds, converged %d;  pairs identical: %s, rounds identical: %s =="
      % (len(gx), len(m[0]), len(m[3]), len(f[2]), len(pr[0]), info["rounds"], info["converged"], np.array_equal(pr[0], g[1]) and np.array_equal(pr[1], g[2]), info == info2))
for k, v in alone.items():
    print("%-32s min %.4f s  median %.4f s  (%d rounds)" % (k, min(v), med(v), rounds))
print("moved per batch: (a) up %.1f MB (the matrix), down %.1f MB (the final matrix);  (b) up %.1f MB (the rows), down %.1f MB (gene labels and pairs)"
      % ((len(m[1]) * 4 + len(m[3]) * 8) / 1e6, (len(f[0]) * 4 + len(f[2]) * 8) / 1e6, len(gx) * 16 / 1e6, (len(g[0]) * 4 + len(g[1]) * 8) / 1e6))

print("== find_cluster.py -i x.opc -a mcl -I 1.5 -G F|T|M, process start to exit, fresh processes, alternating ==")
cmd = [py, os.path.join(ROOT, "bin", "find_cluster.py"), "-i", op, "-a", "mcl", "-I", "1.5"]
runs = max(rounds, 5)
wall, outs = collections.defaultdict(list), {}
for r in range(runs):
    for g in ("F", "T", "M"):
        t = clock()
        outs[g] = subprocess.run(cmd + ["-G", g], capture_output=True, check=True).stdout
        wall[g].append(clock() - t)
for g in ("F", "T", "M"):
    print("find_cluster.py -a mcl -I 1.5 -G %s  min %.3f s  median %.3f s  spread (max - min) %.3f s  (%d runs, %d groups)"
          % (g, min(wall[g]), med(wall[g]), max(wall[g]) - min(wall[g]), runs, outs[g].count(b"\n")))
    print("    every run: %s" % " ".join("%.3f" % v for v in wall[g]))
print("output identical: %s" % (outs["F"] == outs["T"] == outs["M"]))
