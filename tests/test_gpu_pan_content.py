"""The shared-family counts on the GPU (csrc/pan.hip, include/sohit.h so_pan_shared) against the numpy definitions (swiftortho_amd/pan.py
shared_counts, boot_shared) integer for integer, on designed tables (tests/pan_content_inputs.py) at the kernels' edges: a 64-row word, the
64 x 64 tile of taxon pairs and its 4 x 4 register blocks, the chunk of 32 row words, forced word ranges with a short last one, the four
draw tiles of a workgroup of k_pan_draw and its eight blocks of 64 taxa, every batch edge of the replicates; device memory poisoned, twice in
one process; every refusal; content_tree, scripts/pan_genome.py -t -d -B and pipeline.gene_content_tree_from_search with and without the
device, byte for byte.

Run on the GPU box:  python -m pytest tests/test_gpu_pan_content.py -m gpu -q
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import pan_content_inputs as ci
from conftest import ROOT

pytestmark = pytest.mark.gpu

SCRIPT = os.path.join(ROOT, "scripts", "pan_genome.py")
ROWS = (1, 63, 64, 65, 127, 128, 129, 64 * 40 + 7)
TAXA = (1, 2, 3, 63, 64, 65, 128, 129, 193)
# one unit either side of: the register block (4 taxa), the chunk (32 words = 2048 rows), a workgroup of draw tiles (4 x 64 rows)
EDGE_TAXA = (4, 5, 67, 68, 69)
EDGE_ROWS = (64 * 31, 64 * 32 - 1, 64 * 32, 64 * 32 + 1, 64 * 33)
SEED = 20260101


@pytest.fixture(scope="module")
def pan():
    from swiftortho_amd import pan
    return pan


@pytest.fixture(autouse=True)
def poisoned(monkeypatch):
    monkeypatch.setenv("SOHIT_POISON", "165")
    monkeypatch.delenv("SOHIT_PAN_BOOT_BATCH", raising=False)
    monkeypatch.delenv("SOHIT_PAN_SHARED_RANGES", raising=False)


@functools.lru_cache(maxsize=None)
def table(R, T):
    """(counts, row, taxon, S by numpy): computed once, shared, left unchanged.  Some members are listed twice"""
    from swiftortho_amd import pan
    counts = ci.ramp(R, T)
    counts[::3] *= 2
    row, tax = ci.members(counts)
    return counts, row, tax, pan.shared_counts(counts)


@functools.lru_cache(maxsize=None)
def replicate(R, T, seed, b):
    from swiftortho_amd import pan
    return pan.boot_shared(table(R, T)[0], seed, b)


def same(got, want):
    assert got.dtype == want.dtype == np.int64 and got.shape == want.shape and got.tolist() == want.tolist()


@pytest.mark.parametrize("R", ROWS + EDGE_ROWS)
def test_matrix_shapes(pan, R):
    for T in TAXA + (EDGE_TAXA if R in (65, ROWS[-1]) else ()):
        _, row, tax, want = table(R, T)
        stats = {}
        got = pan.device_shared_counts(row, tax, R, T, stats=stats)
        same(got, want)
        assert stats["waits"] == 1 and stats["batches"] == 1 and stats["bytes"] == 4 * T * T
        same(pan.device_shared_counts(row, tax, R, T), want)        # twice in one process


def test_ramp_tables(pan):
    for R, T in ci.RAMP_CHECKED:
        _, row, tax, want = table(R, T)
        ci.ramp_facts(want)                                          # no two genomes alike: a shifted or swapped tile cannot hide
        same(pan.device_shared_counts(row, tax, R, T), want)


def test_many_tiles(pan):
    """more tiles of taxon pairs than one row of tiles: 5 x 5 tiles, the upper triangle walked and mirrored"""
    R, T = 70, 64 * 4 + 3
    _, row, tax, want = table(R, T)
    same(pan.device_shared_counts(row, tax, R, T), want)


@pytest.mark.parametrize("forced,R,ranges", [(4, 64 * 40 + 7, 4), (3, 64 * 40 + 7, 3), (41, 64 * 40 + 7, 41), (8, 130, 3), (2, 129, 2), (5, 1, 1)])
def test_forced_word_ranges(pan, monkeypatch, forced, R, ranges):
    """SOHIT_PAN_SHARED_RANGES: a small input walks several ranges (41 words in 4: 11, 11, 11 and a short last range of 8), each flushing
    with integer adds -- the same integers"""
    monkeypatch.setenv("SOHIT_PAN_SHARED_RANGES", str(forced))
    for T in (65, 3):
        _, row, tax, want = table(R, T)
        stats = {}
        same(pan.device_shared_counts(row, tax, R, T, stats=stats), want)
        assert stats["ranges"] == ranges
        stats = {}
        got = pan.device_boot_shared(row, tax, R, T, SEED, 2, 2, stats=stats)
        assert stats["ranges"] == ranges
        for k in range(2):
            same(got[k], replicate(R, T, SEED, 2 + k))


@pytest.mark.parametrize("batch", [None, 1, 2, 100])
@pytest.mark.parametrize("R,T", [(64 * 3 + 17, 65), (257, 513)])
def test_replicates(pan, monkeypatch, R, T, batch):
    """n_reps of 1, 3 and 8 from replicate 0 and from replicate 5, a last draw tile of 17 rows (and of 1 row behind a full workgroup of
    draw tiles, with a ninth block of 64 taxa), the batch forced to 1, to 2 and beyond n_reps: every replicate is boot_shared's"""
    if batch is not None:
        monkeypatch.setenv("SOHIT_PAN_BOOT_BATCH", str(batch))
    _, row, tax, _ = table(R, T)
    fifth = []
    for b0 in (0, 5):
        for nb in (1, 3, 8):
            stats = {}
            got = pan.device_boot_shared(row, tax, R, T, SEED, b0, nb, stats=stats)
            assert got.shape == (nb, T, T) and stats["waits"] == 1 and stats["bytes"] == 4 * nb * T * T
            assert stats["batches"] == (1 if batch is None else -(-nb // min(batch, nb)))
            for k in range(nb):
                same(got[k], replicate(R, T, SEED, b0 + k))
            if b0 + nb > 5:
                fifth.append(got[5 - b0].tolist())
    assert len(fifth) == 4 and all(f == fifth[0] for f in fifth)      # replicate 5 is the same matrix in every call that holds it
    assert replicate(R, T, SEED, 0).tolist() != replicate(R, T, SEED, 1).tolist()


def test_replicates_of_small_tables(pan):
    for R, T in ((1, 1), (1, 3), (63, 2), (64, 64), (65, 129)):
        _, row, tax, _ = table(R, T)
        got = pan.device_boot_shared(row, tax, R, T, 2 ** 64 - 1, 2 ** 31 - 3, 3)
        for k in range(3):
            same(got[k], replicate(R, T, 2 ** 64 - 1, 2 ** 31 - 3 + k))


def test_refusals(pan):
    R, T = 65, 5
    _, row, tax, want = table(R, T)
    bad_row, bad_tax, neg_row, neg_tax = row.copy(), tax.copy(), row.copy(), tax.copy()
    bad_row[7], bad_tax[11], neg_row[0], neg_tax[0] = R, T, -1, -1
    call = lambda **kw: pan._device_shared("t", **dict(dict(row=row, taxon=tax, n_rows=R, n_taxa=T, seed=1, b0=0, nb=0, device=0), **kw))
    for change, word in ((dict(row=bad_row), "a row outside"), (dict(row=neg_row), "a row outside"), (dict(taxon=bad_tax), "a taxon outside"),
                         (dict(taxon=neg_tax), "a taxon outside"), (dict(row=bad_row, nb=2), "a row outside"), (dict(taxon=bad_tax, nb=2), "a taxon outside"),
                         (dict(n_taxa=0), "1 .. 4096"), (dict(n_taxa=4097), "1 .. 4096"), (dict(n_rows=1 << 31), "2^31 rows"), (dict(nb=-1), "n_reps"),
                         (dict(nb=32769), "32768"), (dict(nb=2, b0=2 ** 31 - 1), "2^31 - 1"), (dict(nb=1, n_rows=0, row=row[:0], taxon=tax[:0]), "no row to draw from"),
                         (dict(n_rows=0), "a row outside"), (dict(n_taxa=4096, nb=32768), "bytes"), (dict(device=1 << 10), "device")):
        with pytest.raises(RuntimeError) as e:
            call(**change)
        assert word in str(e.value), (change, str(e.value))
        same(pan.device_shared_counts(row, tax, R, T), want)         # a refusal leaves nothing behind: the next call is served
    with pytest.raises(RuntimeError) as e:
        call(n_taxa=4096, nb=32768)
    assert str(4 * 32768 * 4096 * 4096) in str(e.value)              # the message gives the bytes
    import ctypes as C
    from swiftortho_amd import _lib
    L, res = _lib.load(), _lib.SoPanSharedResult()
    assert L.so_pan_shared(0, 0, None, None, 5, 3, C.c_uint64(0), 0, 0, 4, C.byref(res)) == 1 and b"unknown flag bits" in L.so_pan_last_error()


def test_nothing_to_launch_and_flags(pan):
    """no rows: served without a launch (no wait), zeros; rows without members: launched, zeros; flags: no matrix, events"""
    none = np.zeros(0, dtype=np.int32)
    stats = {}
    S = pan.device_shared_counts(none, none, 0, 4, stats=stats)
    assert S.shape == (4, 4) and not S.any() and stats["waits"] == 0
    S = pan.device_shared_counts(none, none, 70, 4, stats=stats)
    assert S.shape == (4, 4) and not S.any() and stats["waits"] == 1
    assert not pan.device_boot_shared(none, none, 70, 4, 1, 0, 2).any()
    R, T = 129, 65
    _, row, tax, _ = table(R, T)
    stats = {}
    assert pan._device_shared("t", row, tax, R, T, 1, 0, 3, 0, stats, want=False, timed=True) is None
    assert stats["waits"] == 1 and stats["draw_ms"] > 0. and stats["product_ms"] > 0.


# ---------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["jaccard", "overlap"])
def test_content_tree_with_and_without_the_device(pan, metric):
    for counts in (ci.ramp(200, 9), ci.with_rare_genome(), ci.planted()[0], ci.ramp(40, 3), ci.ramp(40, 2), ci.ramp(130, 70)):
        T = counts.shape[1]
        names, tb = ci.names_of(T), ci.table_of(pan, counts)
        for boot in (0, 16):
            hs, ds = {}, {}
            host = pan.content_tree(tb, names, metric, boot, 3, stats=hs)
            dev = pan.content_tree(tb, names, metric, boot, 3, device_stage=True, stats=ds)
            assert dev[0] == host[0] and dev[1].dtype == np.int64 and dev[1].tolist() == host[1].tolist() and dev[2].tobytes() == host[2].tobytes()
            if boot:
                assert ds["boot_valid"] == hs["boot_valid"] and ds["calls"] == (2 if T > 3 else 1)
                if counts.shape == (70, 7):
                    assert 1 <= hs["boot_valid"] < 16               # the numpy path drops a replicate at least, and keeps one at least
    with pytest.raises(ValueError) as e:
        pan.content_tree(ci.table_of(pan, ci.lonely()), ci.names_of(8), metric, 4, 1, device_stage=True)
    assert "none of the 4 replicates" in str(e.value)


def run_script(d, fasta, groups, extra):
    os.makedirs(str(d), exist_ok=True)
    fa, gr = str(d / "in.fsa"), str(d / "in.clsr")
    open(fa, "w").write(fasta), open(gr, "w").write(groups)
    env = dict(os.environ, PYTHONHASHSEED="0")                       # every run orders the columns of the report alike
    r = subprocess.run([sys.executable, SCRIPT, "-i", fa, "-g", gr] + list(extra), capture_output=True, cwd=str(d), env=env)
    read = lambda p: open(p, "rb").read() if os.path.isfile(p) else None
    return r, read(gr + "_xy.txt"), read(str(d / "t.nwk")), read(str(d / "d.tsv"))


@pytest.mark.parametrize("metric", ["jaccard", "overlap"])
def test_script_G_T_equals_G_F(tmp_path, metric):
    counts = ci.with_rare_genome()
    counts = counts[counts.any(1)]
    fasta, groups = ci.files_of(counts, ci.names_of(counts.shape[1]))
    plain = run_script(tmp_path / "p", fasta, groups, ())
    flags = ("-t", "t.nwk", "-d", "d.tsv", "-B", "16", "-m", metric)
    f = run_script(tmp_path / "f", fasta, groups, flags + ("-G", "F"))
    t = run_script(tmp_path / "t", fasta, groups, flags + ("-G", "T"))
    assert f[0].returncode == 0 and t[0].returncode == 0, t[0].stderr[-2000:]
    assert t[1:] == f[1:] and None not in t[1:] and t[2].count(b")0.") + t[2].count(b")1.") == counts.shape[1] - 3
    assert t[0].stdout.replace(b"/t/in.clsr", b"/p/in.clsr") == plain[0].stdout == f[0].stdout.replace(b"/f/in.clsr", b"/p/in.clsr") and t[1] == plain[1]


def test_run_all_fast_C_T(tmp_path):
    """scripts/run_all_fast.py -P T -C T: <name>.gc.nwk and <name>.gc.tsv beside <name>.pan, the same bytes with and without -G T (the two
    new files whatever the hash seed: they list the taxa in sorted order)"""
    import shutil
    files = {}
    for g in "FT":
        d = tmp_path / g
        d.mkdir()
        fas = str(d / "p.fsa")
        shutil.copy(os.path.join(ROOT, "tests", "golden", "nr_dups.fsa"), fas)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_all_fast.py"), "-i", fas, "-s", "111111", "-a", "1", "-v", "500", "-y", "0", "-P", "T",
                            "-C", "T", "-B", "8", "-S", "3", "-G", g], capture_output=True, text=True,
                           env=dict(os.environ, PYTHONHASHSEED="0"))      # the report's columns stand in Python's set order: both runs order them alike
        assert p.returncode == 0, p.stderr[-3000:]
        read = lambda e: open(fas + "_results/p.fsa." + e, "rb").read() if os.path.isfile(fas + "_results/p.fsa." + e) else None
        files[g] = {e: read(e) for e in ("gc.nwk", "gc.tsv", "clsr_xy.txt")}
        files[g]["pan"] = read("pan").replace(("/%s/p.fsa" % g).encode(), b"/F/p.fsa")
    assert files["T"] == files["F"] and files["F"]["gc.nwk"].startswith(b"(tx0") and files["F"]["gc.tsv"].count(b"\n") == 3
    assert files["F"]["pan"] and files["F"]["clsr_xy.txt"]


SEARCH_KW = dict(ssd="111111", nr="AST,CFILMVY,DN,EQ,G,H,KR,P,W", ht=12000017, chk=50000, step=1, v=500, expect=1e-5, flt="T")


def test_pipeline_against_the_script(pan, tmp_path):
    """gene_content_tree_from_search == the script on the groups file groups_from_search yields for the same search"""
    from swiftortho_amd import pipeline, synthprot
    fa = synthprot.synthprot(600, 200, 61)
    p, gr = str(tmp_path / "x.fsa"), str(tmp_path / "x.clsr")
    open(p, "wb").write(fa)
    groups, _ = pipeline.groups_from_search(p, **SEARCH_KW)
    open(gr, "w").write("".join("\t".join(g) + "\n" for g in groups))
    r = subprocess.run([sys.executable, SCRIPT, "-i", p, "-g", gr, "-t", str(tmp_path / "t.nwk"), "-d", str(tmp_path / "d.tsv"), "-B", "8", "-S", "5"], capture_output=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for device in (True, False):
        taxa, newick, S, D, t = pipeline.gene_content_tree_from_search(p, boot=8, boot_seed=5, pan_device=device, **SEARCH_KW)
        assert len(taxa) >= 2 and taxa == sorted(taxa) and t["groups"] == len(groups) and "content" in t and "pan_host" in t
        assert open(str(tmp_path / "t.nwk"), "rb").read() == newick + b"\n"
        assert open(str(tmp_path / "d.tsv")).read() == pan.content_table_text(taxa, S, D)
