"""The split of find_orth.relations() into candidates() + relations_from_candidates(), and the inputs the GPU tests of the candidate
stage rest on (tests/orth_inputs.py).  CPU only.

What generate(seed) holds, asserted below so that no GPU test can pass on an input that skips a path: 2 600 names over 5 taxa in
families of 10 with about 85 % mutual hits; symmetric scores drawn from 8 integer values (ties everywhere); 5 % repeated subject rows
with a higher score; 12 query ids that come back with a second run, planted so that pairs are proposed 3 and 4 times; hub queries whose
runs hold exactly B - 1, B, B + 1 kept rows, and exactly B - 1, B, B + 1 distinct subjects under repeated rows, for every row bound B of
csrc/tune.h, and one of 2 000; half of a hub's subjects answer."""
import functools
import os
import re

import numpy as np
import pytest

import orth_inputs as oi
from conftest import GOLD, ROOT, orth_golden_cases
from test_find_orth import _load

SEEDS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def generated(seed):
    return oi.generate(seed)


@functools.lru_cache(maxsize=None)
def reference(seed, flags):
    return oi.reference(generated(seed), *oi.FLAG_SETS[flags])


def _golden(name, variant):
    from swiftortho_amd import find_orth as fo
    meta, sc = _load(name)
    a = fo.parse(["find_orth.py", "-i", sc] + meta["variants"][variant])
    cols = fo.columns_from_text(open(sc, "rb").read())
    want = open(os.path.join(GOLD, "orth_%s.%s.orth" % (name, variant)), "rb").read().split(b"\n")[:-1]
    return cols, (float(a["-c"]), float(a["-y"]), a["-n"], a["-s"]), want


def test_bounds_mirror_the_header():
    src = open(os.path.join(ROOT, "swiftortho_amd", "csrc", "tune.h")).read()
    for k in ("ORTH_WAVE_ROWS", "ORTH_LDS_ROWS", "ORTH_LDS_TAXA"):
        assert int(re.search(r"#define %s (\d+)" % k, src).group(1)) == getattr(oi, k), k


@pytest.mark.parametrize("name,variant", orth_golden_cases())
def test_split_reproduces_the_goldens(name, variant):
    """relations() == relations_from_candidates(candidates()) == the reference script's stdout, line for line"""
    from swiftortho_amd import find_orth as fo
    cols, flags, want = _golden(name, variant)
    assert len(want) > 10
    cand = fo.candidates(cols, *flags)
    tax, taxa = fo._taxa(cols.names, flags[3])
    assert fo.relations_from_candidates(cols.names, tax, taxa, cand) == want
    assert fo.relations(cols, *flags) == want
    assert cand.n_rows >= cand.n_groups >= cand.n_runs > 0
    # canonical order of the tables
    M = max(len(cols.names), 1)
    for a, b in ((cand.ot_a, cand.ot_b), (cand.ip_a, cand.ip_b)):
        assert np.all(np.diff(a * M + b) > 0)
    assert np.all(cand.ot_a < cand.ot_b) and np.all(np.diff(cand.co_key) > 0)
    assert sorted(zip(cand.ip_a.tolist(), cand.ip_b.tolist())) == sorted(zip(cand.ip_b.tolist(), cand.ip_a.tolist()))   # both orientations


def test_candidates_keyword_plugs_the_stage_in():
    """relations(candidates=f) calls f(cols, coverage, identity, norm, sep) instead of the numpy function, as cnc(..., mcl=device_mcl) does"""
    from swiftortho_amd import find_orth as fo
    cols, flags, want = _golden(*orth_golden_cases()[0])
    seen = []

    def stage(*a):
        seen.append(a)
        return fo.candidates(*a)

    assert fo.relations(cols, *flags, candidates=stage) == want
    assert len(seen) == 1 and seen[0][0] is cols and seen[0][1:] == flags
    assert fo.relations(cols, *flags, candidates=None) == want


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("flags", sorted(oi.FLAG_SETS))
def test_numpy_stage_equals_plain_python(seed, flags):
    """candidates() against the dictionary-and-loop restatement, table for table, value for value"""
    from swiftortho_amd import find_orth as fo
    ref = reference(seed, flags)
    got = oi.tables(fo.candidates(generated(seed), *oi.FLAG_SETS[flags]))
    for k in ("n_rows", "n_runs", "n_groups", "ot", "ip", "co"):
        assert got[k] == ref[k], k


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_guarantees(seed):
    from swiftortho_amd import find_orth as fo
    cols = generated(seed)
    assert len(cols.names) == 2600 and 30000 < len(cols.q) < 40000
    tax, taxa = fo._taxa(cols.names, "|")
    assert len(taxa) == 5
    assert len(np.unique(cols.score)) <= 4 * len(oi.SCORES)
    need = [B + d for B in oi.ROW_BOUNDS for d in (-1, 0, 1)]
    for flags in oi.FLAG_SETS:
        ref = reference(seed, flags)
        rows, subjects = set(ref["run_rows"]), set(ref["run_subjects"])
        # every tier bound from both sides, in kept rows and in distinct subjects; a run beyond all of them
        assert all(x in rows for x in need) and all(x in subjects for x in need), flags
        assert all(x + oi.REPEAT_EXTRA in rows for x in need) and oi.BIG_HUB in rows
        assert ref["n_groups"] < ref["n_rows"]          # repeated subject rows
        assert ref["n_runs"] == len(np.unique(cols.q)) + oi.RETURNING   # the second runs
        lines = fo.relations(cols, *oi.FLAG_SETS[flags])
        for kind in (b"IP", b"OT", b"CO"):
            assert any(l.startswith(kind) for l in lines), (flags, kind)
    ref = reference(seed, "no")
    assert ref["ot_sizes"] == [1, 2, 3, 4] and ref["ip_sizes"] == [1, 2, 3]


def test_last_pair_rule_is_met_both_ways():
    """the last key of a sorted candidate list is a pair (scored with the maximum) for some seeds and lists, and is none for others"""
    seen = {(reference(seed, "no")[k]) for seed in SEEDS for k in ("ot_last", "ip_last")}
    assert seen == {True, False}


@pytest.mark.parametrize("n_taxa", [oi.ORTH_LDS_TAXA - 1, oi.ORTH_LDS_TAXA, oi.ORTH_LDS_TAXA + 1])
def test_many_taxa_input(n_taxa):
    from swiftortho_amd import find_orth as fo
    cols = oi.many_taxa(n_taxa)
    ref = oi.reference(cols, .5, 0., "no")
    got = oi.tables(fo.candidates(cols, .5, 0., "no"))
    assert max(ref["run_rows"]) > oi.ORTH_WAVE_ROWS and len(ref["ot"]) > 100
    for k in ("n_rows", "n_runs", "n_groups", "ot", "ip", "co"):
        assert got[k] == ref[k], k


@pytest.mark.parametrize("case", sorted(oi.edge_inputs()))
def test_edge_inputs(case):
    from swiftortho_amd import find_orth as fo
    cols = oi.edge_inputs()[case]
    for flags in oi.FLAG_SETS.values():
        ref = oi.reference(cols, *flags)
        cand = fo.candidates(cols, *flags)
        got = oi.tables(cand)
        for k in ("n_rows", "n_runs", "n_groups", "ot", "ip", "co"):
            assert got[k] == ref[k], k
        for k in fo.Candidates.FIELDS:
            assert getattr(cand, k).dtype == (np.float64 if k.endswith(("_s", "_best")) else np.int64), k
        tax, taxa = fo._taxa(cols.names, "|")
        assert fo.relations(cols, *flags) == fo.relations_from_candidates(cols.names, tax, taxa, cand)
    got = oi.tables(fo.candidates(cols, .5, 0., "no"))
    empty = dict(ot=[], ip=[], co=[])
    want = {
        "no_rows": dict(empty, n_rows=0, n_runs=0, n_groups=0),
        "no_names": dict(empty, n_rows=0, n_runs=0, n_groups=0),
        "all_filtered": dict(empty, n_rows=0, n_runs=0, n_groups=0),
        "one_row": dict(empty, n_rows=1, n_runs=1, n_groups=1),
        "self_only": dict(empty, n_rows=2, n_runs=2, n_groups=2),
        "one_sided": dict(empty, n_rows=4, n_runs=4, n_groups=4),
        "one_taxon": dict(empty, ip=[(0, 1, 100.), (0, 2, 85.), (1, 0, 100.), (2, 0, 90.)]),
        # both maxima start from 0: the pairs scored -5 and -1 are proposed by neither side as ortholog / in-paralog
        "negative": dict(ot=[(2, 3, 40.)], ip=[(0, 1, 50.), (1, 0, 50.)], co=[(0 * 6 + 4, -5.)]),
        # a|1 - b|1 is proposed three times and dropped; a|1 - b|2 twice, by two runs of a|1 alone
        "second_run": dict(ot=[(0, 4, 100.), (0, 5, 60.)], ip=[], co=[], n_runs=6),
        "dedupe_bsr": dict(ot=[(0, 3, 120.)], n_rows=7, n_groups=6),
        "last_pair": dict(ot=[(0, 3, 95.), (4, 5, 70.)], ip=[(0, 1, 120.), (1, 0, 130.)]),
    }[case]
    for k, v in want.items():
        assert got[k] == v, k
    if case in ("no_rows", "no_names", "all_filtered"):
        assert fo.relations(cols) == []
    if case == "dedupe_bsr":   # the reference score of a|1 is the 80 of its first KEPT row, not the 500 of the filtered one
        assert oi.tables(fo.candidates(cols, .5, 0., "bsr"))["ot"] == [(0, 3, 1.5)]


def test_second_run_in_edge_input_is_counted():
    ref = oi.reference(oi.edge_inputs()["second_run"], .5, 0., "no")
    assert ref["ot_sizes"] == [2, 3]


def test_device_stage_has_no_cpu_fallback():
    """without a HIP device the device functions raise; they never compute on the host"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from swiftortho_amd import find_orth as fo
    cols = oi.edge_inputs()["last_pair"]
    with pytest.raises(RuntimeError) as e:
        fo.device_candidates(cols)
    assert "no HIP device" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        fo.relations(cols, candidates=fo.device_candidates)
    assert "no HIP device" in str(e.value)
    with pytest.raises(RuntimeError):   # n = 0 is served only where there is a device to serve it
        fo.device_candidates(oi.edge_inputs()["no_rows"])
