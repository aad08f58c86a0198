"""The three cluster-stage device calls that share one call scope and one gene numbering -- device_mcl_rows(), device_row_plan(),
device_apc_rows() -- and their commands, THIS checkout against a built checkout of the parent commit, on BASELINE config 5's relations
(the x.opc that mcl_rows_cost.py / cnc_plan_cost.py / apc_rows_cost.py leave in <work dir>; made here when it is missing):
  (a) each call once per fresh process behind a warm-up call, the two checkouts alternating, 9 processes each;
  (b) `find_cluster.py -a mcl -I 1.5 -G M`, `... -G A` and `find_cluster.py -a apc -G A`, process start to exit, alternating;
  (c) the three hit-table calls on the records config 5's search leaves in HBM -- device_candidates_from_records(),
      device_relation_tables_from_records(), rbh.device_core_table_from_records() -- as in (a): the search, a warm-up call and one timed
      call per fresh process;
  (d) `find_orth.py -G R`, `scripts/get_rbh.py -G T` and `scripts/rbh2phy.py -G T` on <work dir>/x.sc, once per checkout: same bytes?
  python tools/diag/shared_call_cost.py <work dir> <parent checkout> [runs]
The yardstick is the parent's median; a line passes when this checkout's median exceeds it by no more than the parent's own spread."""
import collections, json, os, subprocess, sys, time

clock = time.perf_counter
if sys.argv[1] == "--worker":   # <root> <x.opc>: the three calls of that checkout, one timed run each behind a warm-up
    root, op = sys.argv[2], sys.argv[3]
    sys.path.insert(0, root)
    from swiftortho_amd import find_cluster as fc
    box, real = {}, fc.device_mcl_rows
    fc.device_mcl_rows = lambda gx, gy, z, n_labels, inflation, **kw: box.update(b=(gx, gy, z, n_labels)) or real(gx, gy, z, n_labels, inflation, **kw)
    fc.cnc(open(op), 1.5, device_stage="matrix")   # (config 5 is one batch; the call doubles as the warm-up of the runtime)
    names, cx, cy, Z, _ = fc._edge_columns(open(op))
    _, ids, ax, ay, az = fc._apc_input(open(op, "rb").read())
    tax = fc._taxon_codes(ids)[0]
    calls = {"device_mcl_rows": lambda: real(*box["b"], 1.5), "device_row_plan": lambda: fc.device_row_plan(cx, cy, Z, len(names)),
             "device_apc_rows": lambda: fc.device_apc_rows(ax, ay, az, len(ids), tax, 0.5)}
    took = {}
    for k, f in calls.items():
        f()
        t = clock(); f(); took[k] = clock() - t
    print(json.dumps(took))
    sys.exit(0)

if sys.argv[1] == "--table-worker":   # <root>: config 5's search, then the three hit-table calls of that checkout on its resident records
    root = sys.argv[2]
    sys.path.insert(0, root)
    from swiftortho_amd import find_orth as fo, fsearch, rbh, synthprot
    d = json.load(open(os.path.join(root, "tests", "golden", "pipe_c3.json")))["find_hit_flags"]
    d = dict(zip(d[0::2], d[1::2]))
    fa = synthprot.synthprot(100000, 300)
    ids = fo.fasta_ids(fa)
    s = fsearch.Searcher(ssd=d["-s"], nr=d["-r"], ht=int(d["-M"]), chk=int(d["-c"]), step=int(d["-j"]), v=int(d["-v"]), expect=float(d["-e"]), flt=d["-F"])
    s.load_ref_bytes(fa)
    s.load_queries_bytes(fa)
    dev = s.search_device()
    calls = {"device_candidates_from_records": lambda: fo.device_candidates_from_records(dev, ids, ids),
             "device_relation_tables_from_records": lambda: fo.device_relation_tables_from_records(dev, ids, ids),
             "rbh.device_core_table_from_records": lambda: rbh.device_core_table_from_records(dev, ids, ids, fa)}
    took = {}
    for k, f in calls.items():
        f()
        t = clock(); f(); took[k] = clock() - t
    s.close()
    print(json.dumps(took))
    sys.exit(0)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
tmp, parent = sys.argv[1], os.path.abspath(sys.argv[2])
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 9
py, op = sys.executable, os.path.join(tmp, "x.opc")
if not os.path.isfile(op):
    subprocess.run([py, os.path.join(ROOT, "tools", "diag", "cnc_plan_cost.py"), tmp, "100000", "1"], check=True, capture_output=True)
sides = (("parent", parent), ("this", ROOT))
med = lambda v: sorted(v)[len(v) // 2]


def report(title, took):
    print("== %s ==" % title)
    for what in took["parent"]:
        for side, _ in sides:
            v = took[side][what]
            print("%-7s %-36s min %.4f s  median %.4f s  spread (max - min) %.4f s  (%d runs)" % (side, what, min(v), med(v), max(v) - min(v), len(v)))
        p, t = took["parent"][what], took["this"][what]
        print("        %-36s median - parent's median %+.4f s, parent's spread %.4f s: %s" % (what, med(t) - med(p), max(p) - min(p),
                                                                                         "within" if med(t) - med(p) <= max(p) - min(p) else "EXCEEDS"))


took = {side: collections.defaultdict(list) for side, _ in sides}
for r in range(runs):
    for side, root in sides:
        out = subprocess.run([py, os.path.abspath(__file__), "--worker", root, op], capture_output=True, check=True).stdout
        for k, v in json.loads(out.decode().strip().splitlines()[-1]).items():
            took[side][k].append(v)
report("(a) one device call behind a warm-up, a fresh process per run, the checkouts alternating", took)

cmds = (("find_cluster.py -a mcl -I 1.5 -G M", ["-a", "mcl", "-I", "1.5", "-G", "M"]), ("find_cluster.py -a mcl -I 1.5 -G A", ["-a", "mcl", "-I", "1.5", "-G", "A"]),
        ("find_cluster.py -a apc -G A", ["-a", "apc", "-G", "A"]))
took, outs = {side: collections.defaultdict(list) for side, _ in sides}, collections.defaultdict(set)
for r in range(runs):
    for what, flags in cmds:
        for side, root in sides:
            t = clock()
            outs[what].add(subprocess.run([py, os.path.join(root, "bin", "find_cluster.py"), "-i", op] + flags, capture_output=True, check=True).stdout)
            took[side][what].append(clock() - t)
report("(b) the commands, process start to exit, fresh processes, alternating", took)
print("output identical between the checkouts: %s" % all(len(v) == 1 for v in outs.values()))

took = {side: collections.defaultdict(list) for side, _ in sides}
for r in range(runs):
    for side, root in sides:
        out = subprocess.run([py, os.path.abspath(__file__), "--table-worker", root], capture_output=True, check=True).stdout
        for k, v in json.loads(out.decode().strip().splitlines()[-1]).items():
            took[side][k].append(v)
report("(c) one hit-table call on config 5's resident records behind a warm-up, a fresh process per run, the checkouts alternating", took)

sc, fsa = os.path.join(tmp, "x.sc"), os.path.join(tmp, "x.fsa")
outs = collections.defaultdict(set)
for side, root in sides:
    cwd = os.path.join(tmp, "families_" + side)   # (rbh2phy.py writes its family files where it runs)
    os.makedirs(cwd, exist_ok=True)
    for what, cmd in (("find_orth.py -G R", [os.path.join(root, "bin", "find_orth.py"), "-i", sc, "-G", "R"]),
                      ("scripts/get_rbh.py -G T", [os.path.join(root, "scripts", "get_rbh.py"), sc, "-G", "T"]),
                      ("scripts/rbh2phy.py -G T", [os.path.join(root, "scripts", "rbh2phy.py"), "-i", sc, "-f", fsa, "-G", "T", "-o", "groups.tsv"])):
        outs[what].add(subprocess.run([py] + cmd, capture_output=True, check=True, cwd=cwd).stdout)
    outs["rbh2phy.py: the files it wrote"].add(tuple((f, open(os.path.join(cwd, f), "rb").read()) for f in sorted(os.listdir(cwd))))
print("== (d) the hit-table commands on x.sc, once per checkout ==")
for what, v in outs.items():
    print("%-36s identical between the checkouts: %s" % (what, len(v) == 1))
