"""The launches of ONE so_orth_candidates_records call out of a kernel trace of `orth_cost.py ... --trace`:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/diag/orth_cost.py 100000 3 --trace
    python tools/diag/orth_trace.py DIR
The trace also holds the search that made the records; the last call = everything from the last k_orth_unpack launch on."""
import csv, glob, os, sys

f = sorted(glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True))[0]
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
name = lambda r: r["Kernel_Name"].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0][:72]
first = max(i for i, r in enumerate(rows) if "k_orth_unpack" in r["Kernel_Name"])
call = rows[first:]
t0 = int(call[0]["Start_Timestamp"])
print("last so_orth_candidates_records call: %d launches" % len(call))
print("%10s %10s %10s  %s" % ("start us", "dur us", "gap us", "kernel"))
prev, total, per = t0, 0, {}
for r in call:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    print("%10.1f %10.1f %10.1f  %s" % ((s - t0) / 1e3, (e - s) / 1e3, (s - prev) / 1e3, name(r)))
    prev, total = e, total + e - s
    k = per.setdefault(name(r), [0, 0])
    k[0] += 1; k[1] += e - s
print("== per kernel, this call ==")
for k, (c, ns) in sorted(per.items(), key=lambda kv: -kv[1][1]):
    print("%4d x %10.1f us  %5.1f %%  %s" % (c, ns / 1e3, 100. * ns / total, k))
print("kernels busy %.1f us of %.1f us from the first launch to the last kernel's end" % (total / 1e3, (prev - t0) / 1e3))
