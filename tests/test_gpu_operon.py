"""The operon pairs on the GPU (csrc/operon.hip, include/sohit.h so_operon_pairs) against the numpy definition
(swiftortho_amd/operon.py candidate_pairs) array for array, in both modes -- on the designed tables at the kernels' edges
(tests/operon_inputs.py) and on the inputs of the REAL reference script's goldens (tests/golden/operon_*.json) -- with
SOHIT_OPERON_EXPAND unset and at 1, 7, 64 and 1000 expansions per batch and with device memory poisoned, each setting in a fresh child
process (tests/operon_device_child.py) that serves every table; scripts/operon_cluster.py -G T against the goldens;
scripts/run_all_fast.py -p with and without -G T; the host waits of a call.

Run on the GPU box:  python -m pytest tests/test_gpu_operon.py -m gpu -q
"""
import functools
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import operon_inputs as oi
from conftest import GOLD, ROOT
from test_operon import write_case

pytestmark = pytest.mark.gpu

SCRIPT = os.path.join(ROOT, "scripts", "operon_cluster.py")
# (SOHIT_OPERON_EXPAND, SOHIT_POISON)
RUNS = [(b, None) for b in oi.BUDGETS] + [(None, 0), (None, 255), (7, 0), (7, 255)]


@pytest.fixture(scope="module")
def operon():
    from swiftortho_amd import operon
    return operon


@functools.lru_cache(maxsize=None)
def all_tables():
    import operon_device_child
    return dict(operon_device_child.tables())


@functools.lru_cache(maxsize=None)
def wanted(key):
    """the numpy definition on a table: computed once, shared, left unchanged"""
    from swiftortho_amd import operon
    return operon.candidate_pairs(all_tables()[key])


@functools.lru_cache(maxsize=None)
def device_run(budget, poison):
    """every table through a fresh child process under the two switches -> {array name: array}"""
    env = dict(os.environ)
    for name, v in (("SOHIT_OPERON_EXPAND", budget), ("SOHIT_POISON", poison)):
        env.pop(name, None)
        if v is not None:
            env[name] = str(v)
    with tempfile.TemporaryDirectory(prefix="operon_") as d:
        out = os.path.join(d, "out.npz")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "operon_device_child.py"), out], capture_output=True, env=env)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        with np.load(out) as z:
            return {k: z[k] for k in z.files}


def table_keys():
    return ["d_" + k for k in sorted(oi.designed())] + ["g_" + n for n in oi.golden_names()]


@pytest.mark.parametrize("budget,poison", RUNS)
@pytest.mark.parametrize("key", table_keys())
def test_both_modes_equal_the_definition(operon, key, budget, poison):
    got, want, t = device_run(budget, poison), wanted(key), all_tables()[key]
    ln = np.asarray(t.length)
    keep = operon.passes(want.nshr, ln[want.i], ln[want.j])
    o = np.flatnonzero(keep)
    o = o[np.lexsort((want.j[o], want.i[o]))]
    totals = oi.batch_totals(t, budget)
    launched = sum(1 for x in totals if x)
    for flags, rows, waits in ((0, o, 1 + 3 * launched), (1, slice(None), 1 + 2 * launched)):
        p = "%s/%d/" % (key, flags)
        for name in ("i", "j", "nshr"):
            a, b = got[p + name], getattr(want, name)[rows]
            assert a.dtype == np.int32 and a.tolist() == b.tolist(), (key, flags, name)
        if flags:
            assert got[p + "cand_start"].dtype == np.int64 and got[p + "cand_start"].tolist() == want.cand_start.tolist()
        n_pairs, n_cand, n_exp, batches, n_waits = got[p + "stats"].tolist()
        assert (n_pairs, n_cand, n_exp) == (len(o), len(want.i), sum(oi.expansion_totals(t))), (key, flags)
        assert batches == len(totals) and n_waits == (waits if totals else 0), (key, flags, batches, n_waits)
        if key.startswith("d_") and budget in oi.designed()[key[2:]][1]:
            assert batches > 1


def test_twice_in_one_process_and_the_public_interface(operon, monkeypatch):
    """in-process: the same arrays twice; operon_pairs(device_stage=True) in both orders equals the host path, scores included"""
    monkeypatch.setenv("SOHIT_OPERON_EXPAND", "64")
    monkeypatch.setenv("SOHIT_POISON", "165")
    for key in ("d_lists", "d_random", "g_taxa30", "g_fam0"):
        t, want = all_tables()[key], wanted(key)
        for _ in range(2):
            c = operon.device_operon_pairs(t.start, t.fam, t.length, t.has0, t.n_fam, operon.ALL_CANDIDATES)
            assert c.i.tolist() == want.i.tolist() and c.j.tolist() == want.j.tolist() and c.nshr.tolist() == want.nshr.tolist()
            assert c.stats["batches"] == oi.expected_batches(t, 64) and (c.stats["batches"] > 1 or key == "g_fam0")
        for order in ("reference", "index"):
            a, b = operon.operon_pairs(t, order), operon.operon_pairs(t, order, device_stage=True)
            assert all(x.tolist() == y.tolist() for x, y in zip(a, b)) and len(a[0]) > 0 and b[2].dtype == np.float64


def test_waits_do_not_grow_with_the_operons(operon, monkeypatch):
    """inside one batch the host waits of a call are a constant: the index's groups, the batch's runs, (the survivors,) the rows"""
    monkeypatch.delenv("SOHIT_OPERON_EXPAND", raising=False)
    for flags, waits in ((0, 4), (1, 3)):
        for n in (1, 70, 700):
            t = oi.Table([([1, 2, 3, 4], 4, 0)] * n)
            c = operon.device_operon_pairs(t.start, t.fam, t.length, t.has0, t.n_fam, flags)
            assert c.stats == {"n_pairs": n * n, "n_candidates": n * n, "n_expansions": 4 * n * n, "batches": 1, "waits": waits}
            assert len(c.i) == n * n and set(c.nshr.tolist()) == {4}


def test_refusals_and_nothing_to_launch(operon):
    t = oi.designed()["rank_ties"][0]
    args = dict(start=t.start, fam=t.fam, length=t.length, has0=t.has0, n_fam=t.n_fam)
    twice = t.fam.copy()
    twice[1] = t.fam[0]
    want = operon.candidate_pairs(t)
    for change, word in ((dict(flags=4), "flags"), (dict(fam=twice), "repeated"), (dict(n_fam=5), "a family outside"), (dict(device=1 << 10), "device")):
        with pytest.raises(RuntimeError) as e:
            operon.device_operon_pairs(**dict(args, **change))
        assert word in str(e.value), (word, str(e.value))
        good = operon.device_operon_pairs(flags=1, **args)          # a refusal leaves nothing behind: the next call is served
        assert good.j.tolist() == want.j.tolist()
    for key in ("none", "one_bare", "bare"):                         # no operon, or none with an indexed family: served without a launch
        t = oi.designed()[key][0]
        c = operon.device_operon_pairs(t.start, t.fam, t.length, t.has0, t.n_fam, 1)
        assert len(c.i) == 0 and c.cand_start.tolist() == [0] * (t.n_ops + 1) and c.stats["waits"] == 0 and c.stats["batches"] == 0


@pytest.mark.parametrize("name", oi.golden_names())
def test_script_G_T_equals_the_reference(tmp_path, name):
    gr, op = write_case(tmp_path, name)
    r = subprocess.run([sys.executable, SCRIPT, "-g", gr, "-p", op, "-G", "T"], capture_output=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.decode() == oi.golden(name)["stdout"]


def operons_of_fasta(path):
    """an operon file for a FASTA file: per taxon the genes in the order of their ids, four to an operon, strands alternating"""
    by_taxon = {}
    for line in open(path):
        if line.startswith(">"):
            g = line[1:].split()[0]
            by_taxon.setdefault(g.split("|")[0], []).append(g)
    lines = ["gene_id\tstrand"]
    for tax in sorted(by_taxon):
        genes = sorted(by_taxon[tax])
        for k in range(0, len(genes), 4):
            lines.append(("-->" if (k // 4) % 2 == 0 else "<--").join(genes[k:k + 4]) + "\t+")
    return "\n".join(lines) + "\n"


def test_run_all_fast_with_an_operon_file(tmp_path):
    """scripts/run_all_fast.py -p: <operon name>.xyz and .clsr beside the other files, the same bytes with and without -G T, the .xyz what
    scripts/operon_cluster.py prints for the .clsr of the run; without -p neither file appears"""
    files = {}
    for g in "FT":
        d = tmp_path / g
        d.mkdir()
        fas, opf = str(d / "p.fsa"), str(d / "q.operon")
        shutil.copy(os.path.join(GOLD, "nr_dups.fsa"), fas)
        with open(opf, "w") as f:
            f.write(operons_of_fasta(fas))
        p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_all_fast.py"), "-i", fas, "-p", opf, "-s", "111111", "-a", "1", "-v", "500", "-y", "0",
                            "-G", g], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        assert "operon clustering time:" in p.stdout
        files[g] = {e: open(fas + "_results/" + e, "rb").read() for e in ("q.operon.xyz", "q.operon.clsr", "p.fsa.xyz", "p.fsa.clsr")}
        r = subprocess.run([sys.executable, SCRIPT, "-g", fas + "_results/p.fsa.clsr", "-p", opf], capture_output=True)
        assert r.returncode == 0 and r.stdout == files[g]["q.operon.xyz"]
    print("operon .xyz lines:", files["F"]["q.operon.xyz"].count(b"\n"), ".clsr lines:", files["F"]["q.operon.clsr"].count(b"\n"))
    assert files["T"] == files["F"] and files["F"]["q.operon.xyz"].count(b"\n") > 5 and files["F"]["q.operon.clsr"]
