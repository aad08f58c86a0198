"""Phyletic profiles on the GPU (csrc/phyletic.hip, include/sohit.h so_phyletic_pairs) against the numpy definition
(swiftortho_amd/phyletic.py linked_pairs) integer for integer and dtype for dtype, on the designed inputs of tests/phyletic_inputs.py
(whose promises tests/test_phyletic.py asserts) at the kernels' edges: 0 .. 323 eligible rows among ineligible ones -- the 64-row tile,
its 4 x 4 register blocks, a last tile of one row, several tiles a side --, 1 .. 193 taxa and the chunk of PP_CHUNK taxon words from
both sides, a tile in which every cell is a pair, results without a pair, both products of the test at 4096 x (2^20 - 1), 4465 tile pairs on the fixed grid (two and more a workgroup); device memory
poisoned, twice in one process; every refusal; scripts/phyletic_links.py with and without the device, byte for byte;
scripts/run_all_fast.py -G T with and without -L T; pipeline.family_links_from_search.

Run on the GPU box:  python -m pytest tests/test_gpu_phyletic.py -m gpu -q
"""
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import phyletic_inputs as pi
from conftest import ROOT

pytestmark = pytest.mark.gpu

SCRIPT = os.path.join(ROOT, "scripts", "phyletic_links.py")
PP_CHUNK = pi.tune_define("PP_CHUNK")


@pytest.fixture(scope="module")
def ph():
    from swiftortho_amd import phyletic
    return phyletic


@pytest.fixture(autouse=True)
def poisoned(monkeypatch):
    monkeypatch.setenv("SOHIT_POISON", "165")


@functools.lru_cache(maxsize=None)
def want_shaped(E, T):
    """the definition's answer: computed once, shared, left unchanged"""
    from swiftortho_amd import phyletic
    s = pi.shaped(E, T)
    return phyletic.linked_pairs(s.table, T, *s.args)


def same(got, want):
    for name in ("a", "b", "shared", "present"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype == np.int32 and np.array_equal(g, w), name
    assert got.n_eligible == want.n_eligible


def tiles_of(E):
    nt = (E + 63) // 64
    return nt * (nt + 1) // 2 if E >= 2 else 0


@pytest.mark.parametrize("E", pi.SHAPE_E)
def test_shapes(ph, E):
    for T in pi.SHAPE_T:
        s, want = pi.shaped(E, T), want_shaped(E, T)
        stats = {}
        same(ph.device_linked_pairs(s.table, T, *s.args, stats=stats), want)
        assert stats["n_eligible"] == E and stats["n_pairs"] == len(want.a) and stats["tiles"] == tiles_of(E)
        assert stats["waits"] == (2 if len(want.a) else 1)          # the count that sizes the output, then the result


@pytest.mark.parametrize("T", [64 * PP_CHUNK - 1, 64 * PP_CHUNK, 64 * PP_CHUNK + 1])
def test_chunk_edge(ph, T):
    """the last taxon in the last bit of a chunk's last word, and in the first bit of the next chunk's only word"""
    tb = pi.module_table(65, T)
    want = ph.linked_pairs(tb, T, 1, T, 2, 3, 4)
    assert len(want.a) > 200 and want.present.max() > T // 2 and pi.module_bits(65, T)[:, T - 1].any()
    same(ph.device_linked_pairs(tb, T, 1, T, 2, 3, 4), want)


def test_module_tables(ph):
    for E, T in pi.MODULE_CHECKED:
        tb = pi.module_table(E, T)
        same(ph.device_linked_pairs(tb, T, 1, T, 2, 3, 4), ph.linked_pairs(tb, T, 1, T, 2, 3, 4))


def test_dense_tile_twice(ph):
    """130 families of one profile at num = den = 1: all 8385 pairs, 16 per lane in the full tile; the same arrays from call to call"""
    tb, T, args = pi.dense()
    want = ph.linked_pairs(tb, T, *args)
    first, second = ph.device_linked_pairs(tb, T, *args), ph.device_linked_pairs(tb, T, *args)
    assert len(first.a) == 8385
    same(first, want), same(second, want)


def test_empty_results(ph):
    tb, T, args = pi.lonely()
    stats = {}
    got = ph.device_linked_pairs(tb, T, *args, stats=stats)
    same(got, ph.linked_pairs(tb, T, *args))
    assert len(got.a) == 0 and stats == {"waits": 1, "tiles": 6, "n_eligible": 129, "n_pairs": 0}
    got = ph.device_linked_pairs(tb, T, 5, 4, 1, 1, 1, stats=stats)                  # n_max < n_min: served, nothing is eligible
    same(got, ph.linked_pairs(tb, T, 5, 4, 1, 1, 1))
    assert stats == {"waits": 1, "tiles": 0, "n_eligible": 0, "n_pairs": 0} and got.present.sum() > 0
    none = pi.Table(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), 0, 0)
    got = ph.device_linked_pairs(none, 4, 1, 4, 1, 1, 1, stats=stats)                # no rows: nothing is launched
    same(got, ph.linked_pairs(none, 4, 1, 4, 1, 1, 1))
    assert stats == {"waits": 0, "tiles": 0, "n_eligible": 0, "n_pairs": 0} and len(got.present) == 0
    rows = pi.Table(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), 70, 70)      # rows without members
    same(ph.device_linked_pairs(rows, 4, 1, 4, 1, 1, 1), ph.linked_pairs(rows, 4, 1, 4, 1, 1, 1))
    one = pi.Table(np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), 1, 1)          # one file row: no pair, no grid of 0 blocks
    same(ph.device_linked_pairs(one, 4, 1, 4, 1, 1, 1), ph.linked_pairs(one, 4, 1, 4, 1, 1, 1))


def test_width_probe(ph):
    """both sides of the test reach 4096 x (2^20 - 1), just under 2^32: equality links, a taxon fewer does not"""
    big = (1 << 20) - 1
    tb, T = pi.full_rows()
    for num in (big, 1):
        got = ph.device_linked_pairs(tb, T, 1, T, 1, num, big)
        assert pi.as_lists(got) == ([0, 0, 1], [1, 2, 2], [4096] * 3)
    tb, T = pi.full_rows(short=True)
    got = ph.device_linked_pairs(tb, T, 1, T, 1, big, big)
    assert pi.as_lists(got) == ([0], [2], [4096]) and got.present.tolist() == [4096, 4095, 4096]
    same(got, ph.linked_pairs(tb, T, 1, T, 1, big, big))


def test_larger_case(ph):
    """about 2000 eligible rows x 500 taxa: 31 tiles a side and eight taxon words, several rows of tiles (a workgroup a tile pair here:
    test_grid_stride walks more)"""
    tb, T, args = pi.larger()
    want = ph.linked_pairs(tb, T, *args)
    stats = {}
    same(ph.device_linked_pairs(tb, T, *args, stats=stats, timed=True), want)
    assert stats["tiles"] == tiles_of(want.n_eligible) >= 31 * 32 // 2 and stats["waits"] == 2
    assert stats["count_ms"] > 0. and stats["emit_ms"] > 0. and stats["sort_ms"] > 0.
    got = ph.device_linked_pairs(tb, T, *args, stats=stats, want=False)              # flags bit 0: no pair arrays
    assert got.a is None and stats["n_pairs"] == len(want.a) and np.array_equal(got.present, want.present)


def test_grid_stride(ph):
    """more than two tile pairs per workgroup of the fixed grid, every one of them with pairs to emit: the stride over the pairs, the steps
    from row to row of tiles, the LDS counter's reset and the cursor's second and later reservations, array for array; twice"""
    tb, T, args = pi.strided()
    want = pi.strided_facts(ph)
    stats = {}
    same(ph.device_linked_pairs(tb, T, *args, stats=stats), want)
    grid = 8 * 256                                                 # what the grid can at most be: eight workgroups (a wave a SIMD each) on each of the MI355X's 256 CUs
    assert stats["tiles"] == 4465 > 2 * grid and stats["n_pairs"] == len(want.a) and stats["waits"] == 2
    same(ph.device_linked_pairs(tb, T, *args), want)


def test_refusals(ph):
    s = pi.shaped(65, 64)
    tb, T, args = s.table, s.T, s.args
    want = want_shaped(65, 64)
    n_min, n_max, k_min, num, den = args

    def call(table=tb, T=T, **kw):
        a = dict(n_min=n_min, n_max=n_max, k_min=k_min, num=num, den=den)
        dev = kw.pop("device", 0)
        a.update(kw)
        return ph.device_linked_pairs(table, T, a["n_min"], a["n_max"], a["k_min"], a["num"], a["den"], device=dev)

    def changed(**kw):
        t = pi.Table(tb.row.copy(), tb.taxon.copy(), tb.n_rows, tb.n_file_rows)
        for k, v in kw.items():
            if k in ("row", "taxon"):
                getattr(t, k)[v[0]] = v[1]
            else:
                setattr(t, k, v)
        return t

    cases = ((dict(table=changed(row=(7, tb.n_rows))), "a row outside"), (dict(table=changed(row=(0, -1))), "a row outside"),
             (dict(table=changed(taxon=(11, T))), "a taxon outside"), (dict(table=changed(taxon=(0, -1))), "a taxon outside"),
             (dict(T=0), "1 .. 4096"), (dict(T=4097), "1 .. 4096"), (dict(table=changed(n_rows=1 << 31, n_file_rows=0)), "2^31 rows"),
             (dict(table=changed(n_file_rows=tb.n_rows + 1)), "n_file_rows"), (dict(table=changed(n_file_rows=-1)), "n_file_rows"),
             (dict(table=changed(n_rows=0, n_file_rows=0)), "a row outside"),
             (dict(n_min=0), "n_min"), (dict(k_min=0), "k_min"), (dict(num=0), "0 < num <= den < 2^20"), (dict(num=5, den=4), "0 < num <= den < 2^20"),
             (dict(num=1, den=1 << 20), "0 < num <= den < 2^20"), (dict(device=1 << 10), "device"))
    for change, word in cases:
        with pytest.raises(RuntimeError) as e:
            call(**change)
        assert word in str(e.value), (change, str(e.value))
        same(call(), want)                                             # a refusal leaves nothing behind: the next call is served
    import ctypes as C
    from swiftortho_amd import _lib
    L, res = _lib.load(), _lib.SoPhyleticResult()
    assert L.so_phyletic_pairs(0, 0, None, None, 5, 5, 3, 1, 3, 1, 1, 2, 4, C.byref(res)) == 1 and b"unknown flag bits" in L.so_phyletic_last_error()
    assert L.so_phyletic_pairs(0, 1 << 31, None, None, 5, 5, 3, 1, 3, 1, 1, 2, 0, C.byref(res)) == 1 and b"2^31 members" in L.so_phyletic_last_error()
    assert L.so_phyletic_pairs(0, 3, None, None, 5, 5, 3, 1, 3, 1, 1, 2, 0, C.byref(res)) == 1 and b"NULL" in L.so_phyletic_last_error()


def test_refusals_by_size(ph):
    """2^31 linked pairs: 65 537 families of one genome are 65 537 x 65 536 / 2 = 2^31 + 32 768 pairs at num = den = 1 -- the count pass
    finds them, nothing is emitted.  More than 64 x 65 535 eligible rows: refused after the first wait, no tile is multiplied.  (The
    third size limit, pairs beyond half of the free device memory, lies behind the first on a device of this size: 2^31 pairs take 77 GB.)"""
    n = 65537
    tb = pi.Table(np.arange(n, dtype=np.int32), np.zeros(n, dtype=np.int32), n, n)
    with pytest.raises(RuntimeError) as e:
        ph.device_linked_pairs(tb, 1, 1, 1, 1, 1, 1)
    assert str(n * (n - 1) // 2) in str(e.value) and "2^31" in str(e.value)
    stats = {}
    ph.device_linked_pairs(tb, 1, 1, 1, 2, 1, 1, stats=stats)                        # k_min 2: the same rows, no pair
    assert stats == {"waits": 1, "tiles": 1025 * 1026 // 2, "n_eligible": n, "n_pairs": 0}
    n = 64 * 65535 + 1
    tb = pi.Table(np.arange(n, dtype=np.int32), np.zeros(n, dtype=np.int32), n, n)
    with pytest.raises(RuntimeError) as e:
        ph.device_linked_pairs(tb, 1, 1, 1, 1, 1, 1)
    assert "%d eligible rows" % n in str(e.value)


# ---------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------
def test_script_G_T_equals_G_F(tmp_path):
    import pan_content_inputs as ci
    counts = np.concatenate([pi.module_bits(150, 40, 7, seed=4).astype(np.int32), np.eye(40, dtype=np.int32)[:6]])
    counts[:150:4] *= 2                                      # members listed twice
    fasta, groups = ci.files_of(counts, ci.names_of(40), 150)
    out = {}
    for g in "FT":
        d = tmp_path / g
        d.mkdir()
        fa, gr = str(d / "in.fsa"), str(d / "in.clsr")
        open(fa, "w").write(fasta), open(gr, "w").write(groups)
        r = subprocess.run([sys.executable, SCRIPT, "-i", fa, "-g", gr, "-j", "3/4", "-k", "3", "-x", str(d / "o.xyz"), "-G", g], capture_output=True, cwd=str(d))
        assert r.returncode == 0, r.stderr[-2000:]
        out[g] = (r.stdout, open(str(d / "o.xyz"), "rb").read())
    assert out["T"] == out["F"] and out["F"][0].count(b"\n") > 1000 and out["F"][1].count(b"\n") == out["F"][0].count(b"\n") - 1
    # a device refusal (more taxa than a call takes; the numpy path serves them): exit code 2, one line, nothing written
    d = tmp_path / "many"
    d.mkdir()
    ids = ["t%04d|g" % k for k in range(4097)]
    open(str(d / "in.fsa"), "w").write("".join(">%s\nMKV\n" % i for i in ids)), open(str(d / "in.clsr"), "w").write("\t".join(ids[:9]) + "\n" + "\t".join(ids[:9]) + "\n")
    for g, code in (("F", 0), ("T", 2)):
        r = subprocess.run([sys.executable, SCRIPT, "-i", str(d / "in.fsa"), "-g", str(d / "in.clsr"), "-x", str(d / (g + ".xyz")), "-l", "1", "-u", "100", "-G", g],
                           capture_output=True, cwd=str(d))
        assert r.returncode == code, r.stderr[-2000:]
    assert r.stdout == b"" and not os.path.exists(str(d / "T.xyz")) and r.stderr.startswith(b"phyletic_links: so_phyletic_pairs: the taxa number") and r.stderr.count(b"\n") == 1
    assert open(str(d / "F.xyz")).read() == "group_000000000\tgroup_000000001\t1.0\n"


def run_all_fast(d, extra):
    d.mkdir()
    fas = str(d / "p.fsa")
    shutil.copy(os.path.join(ROOT, "tests", "golden", "nr_dups.fsa"), fas)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_all_fast.py"), "-i", fas, "-s", "111111", "-a", "1", "-v", "500", "-y", "0"] + list(extra),
                       capture_output=True, text=True, env=dict(os.environ, PYTHONHASHSEED="0"))
    assert p.returncode == 0, p.stderr[-3000:]
    res = fas + "_results"
    return {f: open(os.path.join(res, f), "rb").read() for f in sorted(os.listdir(res))}


def test_run_all_fast_L_T(tmp_path):
    """-L T -G T leaves <name>.links.tsv, <name>.links.xyz and <name>.links.clsr; without -L every file is what it was and no other exists.
    (-l 1 -u 4: of the three genomes' families those of two and of three genomes take part; only the new step reads the two flags.  Linked
    at 0.8 are then the families of one profile, two genomes or all three)"""
    plain = run_all_fast(tmp_path / "plain", ("-G", "T"))
    dev = run_all_fast(tmp_path / "dev", ("-L", "T", "-l", "1", "-u", "4", "-G", "T"))
    new = {"p.fsa.links.tsv", "p.fsa.links.xyz", "p.fsa.links.clsr"}
    assert set(dev) == set(plain) | new and not new & set(plain)
    for f in plain:
        assert dev[f] == plain[f], f
    tsv = dev["p.fsa.links.tsv"].decode().split("\n")
    assert tsv[0] == "#family_a\tfamily_b\ttaxa_a\ttaxa_b\tshared\tjaccard\tp" and tsv[-1] == "" and len(tsv) > 2
    rows = [l.split("\t") for l in tsv[1:-1]]
    assert all(c[2] == c[3] == c[4] in ("2", "3") and c[5] == "1.0" for c in rows)
    assert dev["p.fsa.links.xyz"].count(b"\n") == len(rows) and dev["p.fsa.links.clsr"].count(b"\n") >= 1
    members = dev["p.fsa.links.clsr"].decode().split()
    assert len(members) == len(set(members)) and set(members) <= {c[k] for c in rows for k in (0, 1)}


SEARCH_KW = dict(ssd="111111", nr="AST,CFILMVY,DN,EQ,G,H,KR,P,W", ht=12000017, chk=50000, step=1, v=500, expect=1e-5, flt="T")


def test_pipeline_against_the_script(ph, tmp_path):
    """family_links_from_search == the script on the groups file groups_from_search yields for the same search"""
    from swiftortho_amd import pipeline, synthprot
    fa = synthprot.synthprot(600, 200, 61)
    p, gr = str(tmp_path / "x.fsa"), str(tmp_path / "x.clsr")
    open(p, "wb").write(fa)
    groups, _ = pipeline.groups_from_search(p, **SEARCH_KW)
    open(gr, "w").write("".join("\t".join(g) + "\n" for g in groups))
    flags = ["-j", "1/2", "-k", "1", "-l", "0", "-u", "1000"]
    r = subprocess.run([sys.executable, SCRIPT, "-i", p, "-g", gr] + flags, capture_output=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for device in (True, False):
        taxa, links, t = pipeline.family_links_from_search(p, jaccard="1/2", k_min=1, ts=0, tc=1000, pan_device=device, **SEARCH_KW)
        assert taxa == sorted(taxa) and t["groups"] == len(groups) and "links" in t and "pan_host" in t
        assert ph.links_text(links, len(taxa)).encode() == r.stdout
