"""The component stage of `find_cluster -a mcl` on the GPU (libsohit so_cnc_groups, swiftortho_amd/csrc/cnc.hip) against its numpy
definition find_cluster.group_numbers(): level-1 component numbers, level-2 group numbers and the kept rows, `array_equal` on every
input of tests/cnc_inputs.py (chains, stars, block edges, the component-0 rule, level-2 orders, self pairs, signed zeros, infinities,
two family graphs) and on seeded random graphs; under stale device memory; call after call; the refusals; and through cnc() and the
command line down to the golden bytes."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cnc_inputs as ci
from conftest import GOLD, ROOT
from test_cnc_groups import REFUSALS, refused
from test_find_cluster import cluster_cases

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "bin", "find_cluster.py")
N_RANDOM = 200


@functools.lru_cache(maxsize=None)
def expected(name):
    """group_numbers of a generator input, once: (comp1, grp, keep), read-only"""
    from swiftortho_amd import find_cluster as fc
    X, Y, Z, n = ci.inputs()[name]
    comp1, grp = fc.group_numbers(X, Y, Z, n)
    out = (comp1, grp, ci.keep_rows(X, Y, grp))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def random_expected(seed):
    from swiftortho_amd import find_cluster as fc
    X, Y, Z, n = ci.random_small(seed)
    comp1, grp = fc.group_numbers(X, Y, Z, n)
    return (X, Y, Z, n), (comp1, grp, ci.keep_rows(X, Y, grp))


def check(inp, want, what):
    from swiftortho_amd import find_cluster as fc
    X, Y, Z, n = inp
    info = {}
    comp1, grp, keep = fc.device_group_numbers(X, Y, Z, n, info=info)
    assert comp1.dtype == np.int64 and grp.dtype == np.int64 and keep.dtype == bool, what
    assert np.array_equal(comp1, want[0]), what
    assert np.array_equal(grp, want[1]), what
    assert np.array_equal(keep, want[2]), what
    assert info["n_comp1"] == (int(comp1.max()) + 1 if n else 0), what
    assert info["n_grp"] == (int(grp.max()) + 1 if n else 0), what
    assert info["n_keep"] == int(keep.sum()), what
    if n and len(X):
        assert 1 <= info["sweeps1"] <= n + 2 and (info["sweeps2"] == 0) == (info["n_comp1"] == 1) and info["sweeps2"] <= info["n_comp1"] + 2, (what, info)
    else:
        assert info["sweeps1"] == info["sweeps2"] == 0, what
    return info


@pytest.mark.parametrize("name", sorted(ci.inputs()))
def test_device_equals_numpy_on_the_generator(name):
    check(ci.inputs()[name], expected(name), name)


def test_device_equals_numpy_on_random_small_graphs():
    for seed in range(N_RANDOM):
        check(*random_expected(seed), "seed %d" % seed)


@pytest.mark.parametrize("poison", ["0xFF", "0x5A"])
def test_stale_device_memory(poison, monkeypatch):
    """every fresh device allocation pre-filled (so_cnc_groups reads SOHIT_POISON per call): 0xFF makes an unwritten label or first-row
    slot look like the largest value, 0x5A like an ordinary one"""
    monkeypatch.setenv("SOHIT_POISON", poison)
    for name in sorted(ci.inputs()):
        check(ci.inputs()[name], expected(name), name)
    for seed in range(N_RANDOM):
        check(*random_expected(seed), "seed %d" % seed)


def test_call_after_call():
    """the same call twice gives equal arrays, and a 2-gene input right behind the 5000-gene chain gets its own answer"""
    from swiftortho_amd import find_cluster as fc
    for name in ("family_b", "component_chain300_shuffled", "level2_5"):
        a, b = fc.device_group_numbers(*ci.inputs()[name]), fc.device_group_numbers(*ci.inputs()[name])
        assert all(np.array_equal(u, v) for u, v in zip(a, b)), name
    check(ci.inputs()["chain5000_7"], expected("chain5000_7"), "chain5000_7")
    check(ci.inputs()["one_pair"], expected("one_pair"), "one_pair after the chain")
    check(ci.inputs()["family_a"], expected("family_a"), "family_a")
    check(ci.inputs()["component_zero_rule"], expected("component_zero_rule"), "component_zero_rule after family_a")


@pytest.mark.parametrize("order", ["up", "down", 7])
def test_long_chain_ends_within_the_sweep_cap(order):
    """5000 genes in one chain, numbered along it, against it and shuffled: the labels settle within the cap of n + 2 sweeps (passing it
    would be an error, not a truncated answer), and the number of sweeps is reported"""
    name = "chain5000_%s" % order
    info = check(ci.inputs()[name], expected(name), name)
    print("%s: sweeps1 = %d" % (name, info["sweeps1"]))
    assert 2 <= info["sweeps1"] <= 5002 and info["sweeps2"] == 0 and info["n_comp1"] == 1 and info["n_keep"] == 4999


@pytest.mark.parametrize("case", [c for c in REFUSALS if c[0] in ("nan", "gene_above", "gene_below", "negative_genes")], ids=lambda c: c[0])
def test_refusals_on_the_device_machine(case):
    """with a device present too: non-zero, the message, no result left allocated -- and the next call is served"""
    rc, msg, res = refused(case)
    assert rc != 0 and case[2] in msg, msg
    assert not res.comp1 and not res.grp and not res.keep and res.n_genes == 0 and res.sweeps1 == 0
    from swiftortho_amd import find_cluster as fc
    with pytest.raises(RuntimeError, match="NaN"):
        fc.device_group_numbers([0, 1], [1, 2], [1.0, float("nan")], 3)
    with pytest.raises(RuntimeError, match="bad arguments"):
        fc.device_group_numbers([], [], [], -1)
    check(ci.inputs()["component_zero_rule"], expected("component_zero_rule"), "after a refusal")


@pytest.mark.parametrize("name,variant", cluster_cases())
def test_goldens_through_the_device_stage(name, variant, monkeypatch):
    """cnc(device_stage=True) with the device loop prints the golden text, and the device stage really ran"""
    from swiftortho_amd import find_cluster as fc
    meta = json.load(open(os.path.join(GOLD, "clu_%s.json" % name)))
    a = fc.parse(["find_cluster.py", "-i", "x"] + meta["variants"][variant])
    calls = []
    real = fc.device_group_numbers

    def spy(*args, **kw):
        calls.append(1)
        return real(*args, **kw)
    monkeypatch.setattr(fc, "device_group_numbers", spy)
    groups = fc.cnc(open(os.path.join(GOLD, meta["input"])), float(a["-I"]), device_stage=True)
    assert "".join("\t".join(g) + "\n" for g in groups) == open(os.path.join(GOLD, "clu_%s.%s.mcl" % (name, variant))).read()
    assert calls == [1]


@pytest.mark.parametrize("name,flags,golden", [("taxa4_colon", ["-a", "mcl", "-G", "T"], "clu_taxa4_colon.I1.5.mcl"), ("taxa8_big", ["-a", "mcl", "-Gt"], "clu_taxa8_big.I1.5.mcl"),
                                               ("taxa4_colon", ["-a", "apc", "-G", "T"], "apc_taxa4_colon.default.apc")])
def test_find_cluster_cli_with_the_stage_switch(name, flags, golden, tmp_path):
    """`-a mcl -G T` prints the golden bytes; `-a apc -G T` is accepted and prints the apc golden"""
    meta = json.load(open(os.path.join(GOLD, "clu_%s.json" % name)))
    inp = os.path.join(GOLD, meta["input"])
    r = subprocess.run([sys.executable, CLI, "-i", inp, "-I", "1.5"] + flags, capture_output=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == open(os.path.join(GOLD, golden), "rb").read()
    assert os.listdir(str(tmp_path)) == []
