"""The row plan of `find_cluster -a mcl` on the GPU (libsohit so_cnc_plan, swiftortho_amd/csrc/cnc.hip) against its numpy definition
find_cluster.row_plan(): every field `array_equal` on every input of tests/cnc_plan_inputs.py, with the order made by one 64-bit key and
by two stable passes; under stale device memory; a short input right behind a long one; the refusals; `-G A` down to the golden bytes;
the tables route and the one-process path from a FASTA file to the groups."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cnc_plan_inputs as pi
from conftest import GOLD, ROOT
from test_cnc_plan import FIELDS, nothing_allocated, refused, table_cases, tables_from_rows
from test_find_cluster import cluster_cases
from test_gpu_orth_relations import SEARCH_KW

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "bin", "find_cluster.py")


@functools.lru_cache(maxsize=None)
def expected(name):
    """row_plan of an input, once, read-only"""
    from swiftortho_amd import find_cluster as fc
    P = fc.row_plan(*pi.inputs()[name])
    for f in FIELDS:
        getattr(P, f).setflags(write=False)
    return P


def check(name, two_pass, what=""):
    from swiftortho_amd import find_cluster as fc
    cx, cy, z, n_codes = pi.inputs()[name]
    want, info = expected(name), {}
    got = fc.device_row_plan(cx, cy, z, n_codes, info=info, two_pass=two_pass)
    for f in FIELDS:
        a = getattr(got, f)
        assert a.dtype == np.int64 and np.array_equal(a, getattr(want, f)), (name, two_pass, f, what)
    assert info["n_genes"] == len(want.gene_code) and info["n_keep"] == len(want.order), (name, info)
    assert info["n_comp1"] == (int(want.comp1.max()) + 1 if len(cx) else 0) and info["n_grp"] == (int(want.grp.max()) + 1 if len(cx) else 0), (name, info)
    if len(cx):
        assert info["sort_passes"] == (2 if two_pass else 1), (name, info)
        # one wait each for the genes, the roots, the kept rows, the cuts and ties, one more when there are any, and one per sweep
        assert info["waits"] == 4 + info["sweeps1"] + info["sweeps2"] + (1 if len(want.cut) or len(want.tied) else 0), (name, info)
    else:
        assert info["sort_passes"] == info["waits"] == info["sweeps1"] == 0, (name, info)
    return info


@pytest.mark.parametrize("two_pass", [False, True], ids=["one_key", "two_passes"])
@pytest.mark.parametrize("name", sorted(pi.inputs()))
def test_device_equals_numpy(name, two_pass):
    check(name, two_pass)


@pytest.mark.parametrize("poison", ["0xFF", "0x5A"])
def test_stale_device_memory(poison, monkeypatch):
    """every fresh device allocation pre-filled (so_cnc_plan reads SOHIT_POISON per call): 0xFF makes an unwritten first position, flag
    or key look like the largest value, 0x5A like an ordinary one"""
    monkeypatch.setenv("SOHIT_POISON", poison)
    for name in sorted(pi.inputs()):
        for two_pass in (False, True):
            check(name, two_pass, poison)


def test_a_short_input_right_behind_a_long_one():
    for two_pass in (False, True):
        check("family", two_pass)
        check("two_rows", two_pass, "after the family")
        check("kept32769", two_pass)
        check("one_row", two_pass, "after kept32769")
        check("no_rows", two_pass, "after one_row")
        check("group0_dropped", two_pass, "after no_rows")


@pytest.mark.parametrize("name", sorted(pi.refusals()))
def test_refusals_on_the_device_machine(name):
    """with a device present too: non-zero, the message, no result left allocated -- and the next call is served"""
    from swiftortho_amd import find_cluster as fc
    args, message = pi.refusals()[name]
    for flags in (0, 1):
        rc, msg, res = refused(args, flags)
        assert rc != 0 and message in msg, msg
        assert nothing_allocated(res)
    with pytest.raises(RuntimeError, match=re.escape(message)):
        fc.device_row_plan(*args)
    check("group0_dropped", False, "after a refusal")


def test_no_device_of_that_number():
    from swiftortho_amd import find_cluster as fc
    with pytest.raises(RuntimeError, match="device index out of range"):
        fc.device_row_plan(*pi.inputs()["one_row"], device=4096)


@pytest.mark.parametrize("name,variant", cluster_cases())
def test_find_cluster_cli_with_the_plan_on_the_device(name, variant, tmp_path):
    """`-a mcl -G A` prints the golden bytes"""
    meta = json.load(open(os.path.join(GOLD, "clu_%s.json" % name)))
    inp = os.path.join(GOLD, meta["input"])
    r = subprocess.run([sys.executable, CLI, "-i", inp, "-a", "mcl", "-G", "A"] + meta["variants"][variant], capture_output=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == open(os.path.join(GOLD, "clu_%s.%s.mcl" % (name, variant)), "rb").read()
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("name,variant", cluster_cases()[:2])
def test_the_device_plan_really_ran(name, variant, monkeypatch):
    """cnc(device_stage='all') asks device_row_plan once and the component stage of -G T never"""
    from swiftortho_amd import find_cluster as fc
    meta = json.load(open(os.path.join(GOLD, "clu_%s.json" % name)))
    a = fc.parse(["find_cluster.py", "-i", "x"] + meta["variants"][variant])
    calls = []
    real = fc.device_row_plan
    monkeypatch.setattr(fc, "device_row_plan", lambda *args, **kw: calls.append(1) or real(*args, **kw))
    monkeypatch.setattr(fc, "device_group_numbers", lambda *args, **kw: pytest.fail("the component stage was asked on its own"))
    groups = fc.cnc(open(os.path.join(GOLD, meta["input"])), float(a["-I"]), device_stage="all")
    assert "".join("\t".join(g) + "\n" for g in groups) == open(os.path.join(GOLD, "clu_%s.%s.mcl" % (name, variant))).read()
    assert calls == [1]


@pytest.mark.parametrize("case", ["both_sections_differ", "both_sections_equal", "large"])
def test_tables_on_the_device_equal_the_text(case):
    from swiftortho_amd import find_cluster as fc, find_orth as fo
    names, tables = tables_from_rows(*table_cases()[case])
    text = b"".join(l + b"\n" for l in fo.lines_from_tables(names, tables))
    want = fc.cnc(text, 1.5)
    assert len(want) > 3 and any(len(g) > 2 for g in want)
    assert fc.groups_from_tables(names, tables, 1.5, device_stage="all") == want
    assert fc.groups_from_tables(names, tables, 1.5) == want


def test_groups_from_search(tmp_path):
    """one process from the FASTA file to the groups == cnc() on the lines orthology_from_search() returns; the files only when asked for"""
    from swiftortho_amd import find_cluster as fc, pipeline, synthprot
    fa = synthprot.synthprot(600, 200, 61)
    p = str(tmp_path / "x.fsa")
    open(p, "wb").write(fa)
    lines, _ = pipeline.orthology_from_search(p, **SEARCH_KW)
    want = fc.cnc(b"".join(l + b"\n" for l in lines), 1.5)
    groups, t = pipeline.groups_from_search(p, **SEARCH_KW)
    assert groups == want
    assert sum(1 for g in want if len(g) > 2) > 1
    assert {"load", "search", "orth_relations", "cluster", "rows", "relations", "groups"} <= set(t) and "write_sc" not in t and "write_orth" not in t
    assert t["groups"] == len(want) and t["relations"] == len(lines) and sorted(os.listdir(str(tmp_path))) == ["x.fsa"]


def test_groups_from_search_writes_the_relations_when_asked(tmp_path):
    """the .orth file appears where its path is given and holds orthology_from_search()'s lines; the host stages of find_cluster give the
    same groups.  (The .sc file goes through a torch tensor, as in orthology_from_search(device_stage=True): bringing up torch's device
    context takes longer than a test may.)"""
    from swiftortho_amd import find_cluster as fc, pipeline, synthprot
    p, orth = str(tmp_path / "x.fsa"), str(tmp_path / "x.orth")
    open(p, "wb").write(synthprot.synthprot(120, 150, 3))
    groups, t = pipeline.groups_from_search(p, inflation=2.0, device_stage=False, orth_path=orth, **SEARCH_KW)
    text = open(orth, "rb").read()
    assert len(groups) >= 1 and groups == fc.cnc(text, 2.0) and "write_orth" in t and "write_sc" not in t
    assert text == b"".join(l + b"\n" for l in pipeline.orthology_from_search(p, **SEARCH_KW)[0])
    assert sorted(os.listdir(str(tmp_path))) == ["x.fsa", "x.orth"]
