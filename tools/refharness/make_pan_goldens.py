"""Container-only: goldens for the pan-genome stage (swiftortho_amd/pan.py, csrc/pan.hip).

    python tools/refharness/make_pan_goldens.py [case ...]

Without a case name every case is made again; with names only those (a fixture holds the taxon order of the child that made it, so a
fixture that is made again differs from the committed one although it says the same: name the new cases and leave the others alone).
Runs the REAL reference scripts/pan_genome.py on the inputs of tests/pan_inputs.GOLDEN_CASES, each in a child process with a temporary
working directory (the script leaves pan.npy / type.txt there) and two harness-side stand-ins:
  * Bio.SeqIO (tools/refharness/biostub);
  * the script does `import scipy as np` and `from scipy import median, mean`, which a current scipy no longer serves: the child adds
    numpy's public names to the imported scipy module.  scipy.optimize.curve_fit is wrapped so that a fit that raises (few points, two
    taxa) hands back ones instead of ending the script in front of its table: the fits are not part of what is stored.
numexpr is not importable here, so the script takes its plain numpy branch (ys <= Ts - 1): the one swiftortho_amd/pan.py restates.
Stored per case (tests/golden/pan_<name>.json, one line): the input as GOLDEN_CASES names it (literal text, or the arguments synth()
regenerates it from) and the flags; the taxon order read back from the `#family` line (Python's set order in THAT child); the
`# Number` line; the table text from the `#family` line on; the text of <groups>_xy.txt.  No fit parameter and no reference source text
is stored.
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


def child(script, argv):
    import runpy
    sys.path.insert(0, os.path.join(HERE, "biostub"))
    import numpy
    import scipy
    import scipy.optimize
    try:
        import numexpr  # noqa: F401
        raise SystemExit("numexpr is importable: the script would take its other branch")
    except ImportError:
        pass
    for name in dir(numpy):
        if not name.startswith("_") and not hasattr(scipy, name):
            setattr(scipy, name, getattr(numpy, name))
    real = scipy.optimize.curve_fit

    def curve_fit(f, x, y, **kw):
        try:
            return real(f, x, y, **kw)
        except Exception:
            p = f.__code__.co_argcount - 1
            return numpy.ones(p), numpy.eye(p)
    scipy.optimize.curve_fit = curve_fit
    sys.argv = [script] + argv
    runpy.run_path(script, run_name="__main__")


def run_reference(fasta, groups, allow, flags):
    """-> (stdout text, _xy.txt text) of the real script"""
    with tempfile.TemporaryDirectory(prefix="pan_") as d:
        fa, gr = os.path.join(d, "in.fsa"), os.path.join(d, "in.clsr")
        open(fa, "w").write(fasta)
        open(gr, "w").write(groups)
        argv = ["-i", fa, "-g", gr] + flags
        if allow is not None:
            open(os.path.join(d, "taxa.txt"), "w").write(allow)
            argv += ["-r", os.path.join(d, "taxa.txt")]
        env = dict(os.environ, PYTHONIOENCODING="utf-8")
        r = subprocess.run([sys.executable, "-W", "ignore", os.path.abspath(__file__), "--child", os.path.join(REFERENCE, "scripts", "pan_genome.py")] + argv, cwd=d,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        if r.returncode != 0:
            raise RuntimeError(r.stderr.decode()[-3000:])
        return r.stdout.decode("utf-8"), open(gr + "_xy.txt").read()


def main(names=()):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pan_inputs
    unknown = sorted(set(names) - set(pan_inputs.golden_names()))
    if unknown:
        raise SystemExit("no such case in tests/pan_inputs.GOLDEN_CASES: %s" % ", ".join(unknown))
    for name in list(names) or pan_inputs.golden_names():
        fasta, groups, allow, flags = pan_inputs.case_texts(name)
        out, xy = run_reference(fasta, groups, allow, flags)
        lines = out.split("\n")
        number = [l for l in lines if l.startswith("# Number")]
        head = [k for k, l in enumerate(lines) if l.startswith("#family")]
        assert len(number) == 1 and len(head) == 1, out[-2000:]
        spec, _ = pan_inputs.GOLDEN_CASES[name]
        meta = {"input": spec, "flags": flags, "taxa": lines[head[0]].split("\t")[2:], "number": number[0], "table": "\n".join(lines[head[0]:]), "xy": xy}
        open(os.path.join(GOLD, "pan_%s.json" % name), "w").write(json.dumps(meta, separators=(",", ":")) + "\n")
        print(name, "taxa", len(meta["taxa"]), "rows", meta["table"].count("\n") - 1, meta["number"].replace("\t", " "), "xy lines", xy.count("\n"))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3:])
    else:
        main(sys.argv[1:])
