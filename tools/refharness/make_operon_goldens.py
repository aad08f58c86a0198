"""Container-only: goldens for the operon stage (swiftortho_amd/operon.py, csrc/operon.hip).

    python tools/refharness/make_operon_goldens.py

Runs the REAL reference scripts/operon_cluster.py (it imports networkx, which must be importable) on the inputs of
tests/operon_inputs.GOLDEN_CASES, each in a child process of its own on two temporary files.  The order of the script's lines is the
iteration order of CPython sets of small integers, which does not depend on the hash seed.
Stored per case (tests/golden/operon_<name>.json, one line): the input as GOLDEN_CASES names it (literal text of the two files, or the
arguments the generator regenerates them from) and the script's standard output.  No reference source text is stored.
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("SWIFTORTHO_REFERENCE", "/root/reference")
GOLD = os.path.join(ROOT, "tests", "golden")


def run_reference(groups, operons):
    """-> the standard output of the real script"""
    with tempfile.TemporaryDirectory(prefix="operon_") as d:
        gr, op = os.path.join(d, "in.groups"), os.path.join(d, "in.operon")
        with open(gr, "w") as f:
            f.write(groups)
        with open(op, "w") as f:
            f.write(operons)
        r = subprocess.run([sys.executable, "-W", "ignore", os.path.join(REFERENCE, "scripts", "operon_cluster.py"), "-g", gr, "-p", op], cwd=d,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, PYTHONIOENCODING="utf-8"))
        if r.returncode != 0:
            raise RuntimeError(r.stderr.decode()[-3000:])
        return r.stdout.decode("utf-8")


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import operon_inputs
    for name in operon_inputs.golden_names():
        groups, operons = operon_inputs.case_texts(name)
        out = run_reference(groups, operons)
        meta = {"input": operon_inputs.GOLDEN_CASES[name], "stdout": out}
        path = os.path.join(GOLD, "operon_%s.json" % name)
        with open(path, "w") as f:
            f.write(json.dumps(meta, separators=(",", ":")) + "\n")
        lines = out.split("\n")[:-1]
        print(name, "lines", len(lines), "self pairs", sum(1 for l in lines if l.split("\t")[0] == l.split("\t")[1]), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
