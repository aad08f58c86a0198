"""The pan-genome stage on the GPU (csrc/pan.hip, include/sohit.h so_pan_genome) against the numpy definitions (swiftortho_amd/pan.py)
array for array -- on the inputs of the REAL reference script's goldens (tests/golden/pan_*.json) and on designed member tables at the
kernels' edges (tests/pan_inputs.py): both tiers of k_pan_curve (SOHIT_PAN_TIER), device memory poisoned, twice in one process, with and
without the count matrix; every refusal; scripts/pan_genome.py -G T against -G F; pipeline.pan_genome_from_search against the script on
the groups file of the same search.

Run on the GPU box:  python -m pytest tests/test_gpu_pan.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import pan_curve_inputs as ci
import pan_inputs as pi
from test_pan import check_against_golden, library_result, run_script

pytestmark = pytest.mark.gpu

TIERS = ("lds", "global")
TIER_CODE = {"lds": 1, "global": 2}


@pytest.fixture(scope="module")
def pan():
    from swiftortho_amd import pan
    return pan


@functools.lru_cache(maxsize=None)
def numpy_result(key):
    """the numpy definitions on a designed case: computed once, shared, left unchanged"""
    from swiftortho_amd import pan
    case, (ts, tc) = {k: (c, r) for k, c, r in pi.designed()}[key]
    return pan.pan_genome(pan.MemberTable(case.row, case.taxon, case.n_rows, case.n_file_rows), case.n_taxa, ts, tc)


def same(got, want, counts=True):
    assert got.types.dtype == np.uint8 and got.types.tolist() == want.types.tolist()
    assert got.totals == want.totals
    for k in ("core", "spec", "panz"):
        a, b = getattr(got, k), getattr(want, k)
        assert a.dtype == np.int64 and a.shape == b.shape and a.tolist() == b.tolist(), k
    if counts:
        assert got.counts.dtype == np.int32 and got.counts.shape == want.counts.shape and got.counts.tolist() == want.counts.tolist()
    else:
        assert got.counts is None


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", pi.golden_names())
def test_goldens_through_the_device(pan, monkeypatch, name, tier):
    """the device call on the reference's inputs, in the reference's column order: the numpy arrays, and the reference's own text"""
    monkeypatch.setenv("SOHIT_PAN_TIER", tier)
    monkeypatch.setenv("SOHIT_POISON", "165")
    taxa, table, want = library_result(pan, name)
    taxa, table, got = library_result(pan, name, device_stage=True)
    same(got, want)
    check_against_golden(pan, name, taxa, table, got)
    assert got.stats == {"tier": TIER_CODE[tier], "waits": 1}
    again = library_result(pan, name, device_stage=True)[2]      # twice in one process: identical
    same(again, got)
    ts, tc = pi.flag_values(pi.case_texts(name)[3])
    same(pan.pan_genome(table, len(taxa), ts, tc, device_stage=True, want_counts=False), want, counts=False)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("key", [k for k, _, _ in pi.designed()])
def test_designed_tables(pan, monkeypatch, key, tier):
    """rows around a 64-row tile, taxa around 64 and at 100, all-zero rows, a full row, counts above 1, rows behind the file rows, one
    taxon (no curve) and no file row, under every threshold regime: array for array, device memory poisoned"""
    monkeypatch.setenv("SOHIT_PAN_TIER", tier)
    monkeypatch.setenv("SOHIT_POISON", "90")
    case, (ts, tc) = {k: (c, r) for k, c, r in pi.designed()}[key]
    want = numpy_result(key)
    table = pan.MemberTable(case.row, case.taxon, case.n_rows, case.n_file_rows)
    got = pan.pan_genome(table, case.n_taxa, ts, tc, device_stage=True)
    same(got, want)
    assert got.stats["tier"] == (TIER_CODE[tier] if case.n_taxa > 1 else 0)
    same(pan.pan_genome(table, case.n_taxa, ts, tc, device_stage=True, want_counts=False), want, counts=False)


def test_auto_tier_and_many_tiles(pan, monkeypatch):
    """no switch: few taxa take the LDS tier, more than the LDS holds the global one; more row tiles than tile ranges, so that a
    workgroup walks several tiles and the last range is short"""
    monkeypatch.delenv("SOHIT_PAN_TIER", raising=False)
    monkeypatch.setenv("SOHIT_POISON", "165")
    rng = np.random.RandomState(5)
    for n_rows, n_taxa, tier in ((64 * 300 + 7, 5, 1), (70, 900, 2)):
        m = n_rows * 2
        table = pan.MemberTable(rng.randint(n_rows, size=m).astype(np.int32), rng.randint(n_taxa, size=m).astype(np.int32), n_rows, n_rows - 3)
        want = pan.pan_genome(table, n_taxa, .3, .7, size=4)
        got = pan.pan_genome(table, n_taxa, .3, .7, size=4, device_stage=True)
        same(got, want)
        assert got.stats["tier"] == tier


def _args(pan, **change):
    t = pi.designed_table(60, 5, 3)
    S, Cc = pan.step_thresholds(.05, .95, 3)
    args = dict(row=t.row, taxon=t.taxon, n_rows=t.n_rows, n_file_rows=t.n_file_rows, n_taxa=3, spec_max=1, core_min=3, perm=pan.permutations(3), S=S, C=Cc)
    args.update(change)
    return args


def test_refusals(pan):
    t = pi.designed_table(60, 5, 3)
    bad_row, bad_tax = t.row.copy(), t.taxon.copy()
    bad_row[7], bad_tax[11] = t.n_rows, 3
    neg_row, neg_tax = t.row.copy(), t.taxon.copy()
    neg_row[0], neg_tax[0] = -1, -1
    # two taxa and one group of 4 orders more than the grid of k_pan_curve is high: refused before anything is launched
    limit = ci.served_size_limit(pan.device_pan_genome)
    too_high = dict(zip(ci.ARG_NAMES, ci.grid_case(limit + 1).args()))
    for change, word in ((too_high, "the largest size served is %d)" % limit),
                         (dict(row=bad_row), "a row outside"), (dict(row=neg_row), "a row outside"), (dict(taxon=bad_tax), "a taxon outside"),
                         (dict(taxon=neg_tax), "a taxon outside"), (dict(perm=np.zeros((20, 3), dtype=np.int32)), "not a permutation"),
                         (dict(n_rows=1 << 31), "2^31 rows"), (dict(n_rows=1 << 30), "count matrix of 2^31 cells"), (dict(flags=2), "flags"),
                         (dict(device=1 << 10), "device")):
        with pytest.raises(RuntimeError) as e:
            pan.device_pan_genome(**_args(pan, **change))
        assert word in str(e.value), (word, str(e.value))
        good = pan.device_pan_genome(**_args(pan))             # a refusal leaves nothing behind: the next call is served
        assert good.totals == pan.row_types(pan.count_matrix(t.row, t.taxon, t.n_rows, 3), t.n_file_rows, 1, 3)[1]


def test_nothing_to_launch(pan):
    """no rows: served without a launch (no wait), curves of zeros; rows without members: launched, every count 0"""
    S, Cc = pan.step_thresholds(.05, .95, 4)
    none = np.zeros(0, dtype=np.int32)
    r = pan.device_pan_genome(none, none, 0, 0, 4, 1, 4, pan.permutations(4), S, Cc)
    assert r.stats == {"tier": 0, "waits": 0} and r.core.shape == (20, 3) and not r.core.any() and not r.spec.any() and not r.panz.any()
    assert r.counts.shape == (0, 4) and len(r.types) == 0 and r.totals == (0, 0, 0)
    r = pan.device_pan_genome(none, none, 70, 70, 4, 1, 4, pan.permutations(4), S, Cc)
    assert r.stats["waits"] == 1 and not r.counts.any() and r.totals == (0, 0, 70) and not r.panz.any()
    r = pan.device_pan_genome(none, none, 3, 3, 0, 1, 0, np.zeros((20, 0), dtype=np.int32), none, none)
    assert r.totals == (0, 0, 3) and r.core.shape == (20, 0)


@pytest.mark.parametrize("name", ["default", "rfile", "float100", "quirks", "taxa2"])
def test_script_G_T_equals_G_F(tmp_path, monkeypatch, name):
    monkeypatch.setenv("PYTHONHASHSEED", "0")      # both processes order the taxa alike
    (tmp_path / "f").mkdir(), (tmp_path / "t").mkdir()
    rf, xyf, _ = run_script(tmp_path / "f", name)
    rt, xyt, _ = run_script(tmp_path / "t", name, extra=("-G", "T"))
    assert rf.returncode == 0 and rt.returncode == 0, rt.stderr[-2000:]
    assert rt.stdout.replace(b"/t/in.clsr", b"/f/in.clsr") == rf.stdout and xyt == xyf and xyt is not None
    assert pi.golden(name)["number"].encode() in rt.stdout


SEARCH_KW = dict(ssd="111111", nr="AST,CFILMVY,DN,EQ,G,H,KR,P,W", ht=12000017, chk=50000, step=1, v=500, expect=1e-5, flt="T")


def test_pipeline_against_the_script(pan, tmp_path):
    """pan_genome_from_search == the script on the groups file groups_from_search yields for the same search, in the same column order"""
    from swiftortho_amd import pipeline, synthprot
    fa = synthprot.synthprot(600, 200, 61)
    p, gr = str(tmp_path / "x.fsa"), str(tmp_path / "x.clsr")
    open(p, "wb").write(fa)
    groups, _ = pipeline.groups_from_search(p, **SEARCH_KW)
    open(gr, "w").write("".join("\t".join(g) + "\n" for g in groups))
    for device in (True, False):
        taxa, types, totals, curves, t = pipeline.pan_genome_from_search(p, pan_device=device, **SEARCH_KW)
        assert len(taxa) >= 2 and t["groups"] == len(groups) and "pan" in t and "pan_host" in t
        lines = pan.run(p, gr, taxa=taxa)
        table = pan.member_table(fa.decode(), open(gr).read(), taxa)
        assert pan.number_line(totals, table.n_rows, table.n_file_rows, len(taxa)) in lines
        assert [l.split("\t")[1] for l in lines[lines.index("\t".join(["#family", "type"] + taxa)) + 1:]] == [pan.TYPE_NAMES[k] for k in types.tolist()]
        assert open(gr + "_xy.txt").read() == pan.xy_text(*curves) and len(types) > len(groups) > 20
