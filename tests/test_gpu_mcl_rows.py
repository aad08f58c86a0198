"""One batch of `find_cluster -a mcl` from its rows to its surviving pairs on the GPU (libsohit so_mcl_rows / so_mcl_readout,
swiftortho_amd/csrc/mcl.hip) against its numpy definitions: the assembled matrix against find_cluster.block_matrix_arrays() bit for bit
(data compared as uint32, so a signed zero or a denormal cannot hide), the read-out against surviving_pair_columns(), full and cut
runs against the host path through device_mcl (the same loop code on bit-identical input: no tolerance), on every input of
tests/mcl_rows_inputs.py; the refusals; under stale device memory; long and short inputs in turn; and through cnc() and the command
line down to the golden bytes."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mcl_rows_inputs as mi
from conftest import GOLD, ROOT
from test_find_cluster import cluster_cases
from test_mcl_rows import family_lines

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "bin", "find_cluster.py")


@functools.lru_cache(maxsize=None)
def expected(name):
    """block_matrix_arrays of a batch and the read-out of that matrix, once: (gene, indptr, indices, data, pair_r, pair_c), read-only"""
    from swiftortho_amd import find_cluster as fc
    gx, gy, z, n_labels = mi.batches()[name]
    with np.errstate(over="ignore"):
        gene, indptr, indices, data = fc.block_matrix_arrays(gx, gy, z, list(range(n_labels)))
    with np.errstate(invalid="ignore"):
        r, c = fc.surviving_pair_columns(indptr, indices, data)
    out = (np.array(gene, dtype=np.int64), indptr, indices, data, r, c)
    for a in out:
        a.setflags(write=False)
    return out


def check_assembly(name):
    from swiftortho_amd import find_cluster as fc
    info = {}
    gene, pr, pc, indptr, indices, data = fc.device_mcl_rows(*mi.batches()[name], 1.5, rounds=0, want_matrix=True, info=info)
    want = expected(name)
    assert gene.dtype == pr.dtype == pc.dtype == indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float32, name
    assert np.array_equal(gene, want[0]), name
    assert np.array_equal(indptr, want[1]), name
    assert np.array_equal(indices, want[2]), name
    assert np.array_equal(data.view(np.uint32), want[3].view(np.uint32)), name
    assert np.array_equal(pr, want[4]) and np.array_equal(pc, want[5]), name
    assert info == {"rounds": 0, "converged": 0}, name


@pytest.mark.parametrize("name", sorted(mi.batches()))
def test_assembled_matrix_equals_numpy(name):
    check_assembly(name)


def check_readout(name):
    from swiftortho_amd import find_cluster as fc
    m = mi.readout_matrices()[name]
    with np.errstate(invalid="ignore"):
        want = fc.surviving_pair_columns(*m)
    got = fc.device_readout(*m)
    assert got[0].dtype == got[1].dtype == np.int64, name
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name


@pytest.mark.parametrize("name", sorted(mi.readout_matrices()))
def test_readout_equals_numpy(name):
    check_readout(name)


@pytest.mark.parametrize("prune", [0.0, -1.0, 0.5, float("inf"), float("nan"), 1e-40])
def test_readout_at_other_thresholds(prune):
    """a threshold of 0 keeps the denormal and not -0.0; a NaN threshold keeps nothing"""
    from swiftortho_amd import find_cluster as fc
    m = mi.readout_matrices()["specials"]
    with np.errstate(invalid="ignore"):
        want = fc.surviving_pair_columns(*m, prune=prune)
    got = fc.device_readout(*m, prune=prune)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def check_run(name, rounds):
    """device_mcl_rows against block_matrix_arrays -> device_mcl -> surviving_pair_columns: pairs, rounds and converged, exactly"""
    from swiftortho_amd import find_cluster as fc
    gx, gy, z, n_labels = mi.batches()[name]
    want_info, info = {}, {}
    gene, indptr, indices, data = expected(name)[:4]
    with np.errstate(invalid="ignore"):
        want = fc.surviving_pair_columns(*fc.device_mcl(indptr, indices, data, 1.5, rounds=rounds, info=want_info))
    got = fc.device_mcl_rows(gx, gy, z, n_labels, 1.5, rounds=rounds, info=info)
    assert np.array_equal(got[0], gene), (name, rounds)
    assert np.array_equal(got[1], want[0]) and np.array_equal(got[2], want[1]), (name, rounds)
    assert info == want_info, (name, rounds, info, want_info)
    return info, len(want[0])


@pytest.mark.parametrize("name", mi.LOOP_BATCHES)
def test_full_run_equals_the_host_path(name):
    info, npairs = check_run(name, 100)
    print("%s: rounds = %d, converged = %d, pairs = %d" % (name, info["rounds"], info["converged"], npairs))


@pytest.mark.parametrize("rounds", [2, 3, 4, 5, 6])
def test_cut_runs_end_on_stored_zeros(rounds):
    """a run cut after a few rounds ends on a matrix with pruned, stored zeros: the shifted pairing of the read-out is at work"""
    from swiftortho_amd import find_cluster as fc
    for name in ("family", "rows257", "genes65", "repeat64_straddles_256"):
        info, npairs = check_run(name, rounds)
        assert info == {"rounds": rounds, "converged": 0}
    gene, indptr, indices, data = expected("family")[:4]
    out = fc.device_mcl(indptr, indices, data, 1.5, rounds=rounds)
    assert rounds < 3 or np.any(out[2] == 0)


@pytest.mark.parametrize("name", sorted(mi.refusals()))
def test_refusals_on_the_device_machine(name):
    """every refusal gives its message, leaves nothing allocated, and the next call is served"""
    from swiftortho_amd import find_cluster as fc
    from test_mcl_rows import refused
    args, message, _ = mi.refusals()[name]
    rc, msg, res = refused(args)
    assert rc != 0 and message in msg, msg
    assert not res.gene and not res.pair_r and not res.pair_c and not res.indptr and not res.indices and not res.data
    assert res.n_genes == 0 and res.n_pairs == 0 and res.nnz == 0 and res.rounds == 0
    if len(args[0]):
        with pytest.raises(RuntimeError, match=message.replace("(", r"\(").replace(")", r"\)")):
            fc.device_mcl_rows(*args, 1.5)
    check_assembly("first_seen_as_y")
    check_run("first_seen_as_y", 100)
    with pytest.raises(RuntimeError, match="bad matrix"):
        fc.device_readout([0, 2, 1], [0, 1], [1.0, 1.0])
    check_readout("shifted_pairing")


def test_no_rows_is_served():
    from swiftortho_amd import find_cluster as fc
    info = {}
    gene, pr, pc, indptr, indices, data = fc.device_mcl_rows([], [], [], 5, 1.5, want_matrix=True, info=info)
    assert len(gene) == len(pr) == len(pc) == len(indices) == len(data) == 0 and indptr.tolist() == [0, 0] and info == {"rounds": 0, "converged": 0}


@pytest.mark.parametrize("poison", ["0xFF", "0x5A"])
def test_stale_device_memory(poison, monkeypatch):
    """every fresh device allocation pre-filled (the calls read SOHIT_POISON themselves): 0xFF makes an unwritten flag, first position
    or diagonal look like the largest value, 0x5A like an ordinary one"""
    monkeypatch.setenv("SOHIT_POISON", poison)
    for name in sorted(mi.batches()):
        check_assembly(name)
    for name in sorted(mi.readout_matrices()):
        check_readout(name)
    check_run("genes65", 100)
    check_run("rows257", 4)


def test_long_and_short_inputs_in_turn():
    for name in ("family", "one_row", "rows32769", "first_seen_as_y", "hub1025_last_row", "one_denormal", "family_reversed", "all_zero_or_tiny"):
        check_assembly(name)
    for name in ("nnz32769", "shifted_pairing", "nnz8193", "nnz0", "nnz1025", "specials"):
        check_readout(name)
    check_run("family", 100)
    check_run("one_row", 100)
    check_run("family", 3)
    check_run("first_seen_as_y", 100)


def test_cnc_over_several_batches(monkeypatch):
    """cnc(device_stage='matrix') == cnc() on a family graph cut into several batches, and every batch went through device_mcl_rows"""
    from swiftortho_amd import find_cluster as fc
    lines = family_lines()
    want = fc.cnc(lines, 1.5, chk=50)
    calls = []
    real = fc.device_mcl_rows

    def spy(*args, **kw):
        calls.append(len(args[0]))
        return real(*args, **kw)
    monkeypatch.setattr(fc, "device_mcl_rows", spy)
    monkeypatch.setattr(fc, "device_mcl", lambda *a, **k: pytest.fail("the host path ran"))
    assert fc.cnc(lines, 1.5, chk=50, device_stage="matrix") == want
    assert len(want) > 50 and len(calls) > 5


@pytest.mark.parametrize("name,variant", cluster_cases())
def test_goldens_through_the_command_line(name, variant, tmp_path):
    """every clu_* golden through `bin/find_cluster.py -a mcl -G M` gives the golden bytes"""
    meta = json.load(open(os.path.join(GOLD, "clu_%s.json" % name)))
    inp = os.path.join(GOLD, meta["input"])
    r = subprocess.run([sys.executable, CLI, "-i", inp, "-G", "M"] + meta["variants"][variant], capture_output=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == open(os.path.join(GOLD, "clu_%s.%s.mcl" % (name, variant)), "rb").read()
    assert os.listdir(str(tmp_path)) == []


def test_apc_ignores_the_matrix_value(tmp_path):
    """`-a apc -G M` is accepted and prints the apc golden"""
    meta = json.load(open(os.path.join(GOLD, "clu_taxa4_colon.json")))
    r = subprocess.run([sys.executable, CLI, "-i", os.path.join(GOLD, meta["input"]), "-a", "apc", "-Gm"], capture_output=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == open(os.path.join(GOLD, "apc_taxa4_colon.default.apc"), "rb").read()
