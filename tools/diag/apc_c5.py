"""`find_cluster -a apc` on BASELINE config 5's relations (100k-protein find_hit -> find_orth): wall time of the command next to
`-a mcl` on the same file, size of the entry list, and the loop alone.   python tools/diag/apc_c5.py <work dir> [proteins]
Leaves <work dir>/x.opc behind for a profiler run of the command (rocprofv3 --kernel-trace --stats -- python bin/find_cluster.py ...)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from swiftortho_amd import find_cluster, synthprot

tmp = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
os.makedirs(tmp, exist_ok=True)
meta = json.load(open(os.path.join(ROOT, "tests", "golden", "pipe_c3.json" if n == 100000 else "pipe_c2.json")))
d = dict(zip(meta["find_hit_flags"][0::2], meta["find_hit_flags"][1::2]))
p, sc, op = os.path.join(tmp, "x.fsa"), os.path.join(tmp, "x.sc"), os.path.join(tmp, "x.opc")
open(p, "wb").write(synthprot.synthprot(n, 300))
py = sys.executable
subprocess.run([py, os.path.join(ROOT, "bin", "find_hit.py"), "-p", "blastp", "-i", p, "-d", p, "-o", sc, "-a", "1", "-e", d["-e"], "-v", d["-v"], "-j", d["-j"], "-F", d["-F"],
                "-s", d["-s"], "-r", "aa9", "-M", d["-M"], "-c", d["-c"]], check=True)
open(op, "wb").write(subprocess.run([py, os.path.join(ROOT, "bin", "find_orth.py"), "-i", sc], capture_output=True, check=True).stdout)
for alg in (["-a", "mcl", "-I", "1.5"], ["-a", "apc"], ["-a", "apc"]):
    t = time.time()
    grp = subprocess.run([py, os.path.join(ROOT, "bin", "find_cluster.py"), "-i", op] + alg, capture_output=True, check=True).stdout
    print("find_cluster.py %s: %.2f s, %d groups" % (" ".join(alg), time.time() - t, grp.count(b"\n")))
t = time.time()
names, row, col, score, ng = find_cluster.apc_entries(open(op))
t1 = time.time() - t
deg = __import__("numpy").bincount(row, minlength=ng)
print("apc_entries: %.2f s, %d genes, %d entries, longest row %d, rows above 32 entries: %d" % (t1, ng, len(row), deg.max(), int((deg > 32).sum())))
find_cluster.device_apc(row, col, score, ng, 0.5, rounds=1)
for rounds in (100, 100):
    t = time.time()
    find_cluster.device_apc(row, col, score, ng, 0.5, rounds=rounds)
    print("device_apc, %d rounds (grouping on the host, upload, loop, download): %.3f s" % (rounds, time.time() - t))
