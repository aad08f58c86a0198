"""The record expansion on the GPU (libsohit so_nr_expand, swiftortho_amd/csrc/nr.hip) against its numpy definition nr.expand_records():
the whole 80-byte records, byte for byte, on every designed input of tests/nr_inputs.py; the count-only call; under stale device memory;
every refusal; then the one-process route pipeline.*_from_search(collapse=True) and scripts/run_all_fast.py -G T against the script chain
nr.search_collapsed() -> find_orth -> find_cluster on the same files."""
import ctypes as C
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import nr_inputs
from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def expected(name):
    """expand_records of a designed input, once, read-only"""
    from swiftortho_amd import nr
    c = nr_inputs.BY_NAME[name]
    out = nr.expand_records(c.rec, c.qoff, c.qmem, c.soff, c.smem)
    out.setflags(write=False)
    return out


class _DeviceBytes:
    """n bytes of device memory the library owns, for torch.as_tensor (no copy)"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def device_expand(rec, qoff, qmem, soff, smem, count_only=False):
    """so_nr_expand on records uploaded with torch -> (the expanded records on the host or None, n_out, n_runs, waits)"""
    import torch
    from swiftortho_amd import nr
    raw = np.ascontiguousarray(rec).view(np.uint8)
    t = torch.from_numpy(raw.copy()).cuda() if len(raw) else torch.empty(0, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    e = nr.expand_device_pointer(t.data_ptr() if len(raw) else 0, len(rec), 0, qoff, qmem, soff, smem, count_only=count_only)
    try:
        out = None
        if not count_only:
            assert (e.device_pointer() != 0) == (len(e) > 0)
            nbytes = len(e) * nr_inputs.HIT.itemsize
            out = torch.as_tensor(_DeviceBytes(e.device_pointer(), nbytes), device="cuda").cpu().numpy().view(nr_inputs.HIT) if nbytes else np.zeros(0, dtype=nr_inputs.HIT)
        else:
            assert e.device_pointer() == 0
        return out, len(e), e.n_runs, e.waits
    finally:
        e.close()
        assert e.device_pointer() == 0


def check(name, what=""):
    c, want = nr_inputs.BY_NAME[name], expected(name)
    got, n_out, n_runs, waits = device_expand(c.rec, c.qoff, c.qmem, c.soff, c.smem)
    assert n_out == len(want) == len(got), (name, what)
    assert got.tobytes() == want.tobytes(), (name, what, np.flatnonzero(got != want)[:5])
    q = c.rec["qidx"]
    assert n_runs == (1 + int((q[1:] != q[:-1]).sum()) if len(q) else 0), (name, what)
    assert waits == (0 if len(q) == 0 else 2 if n_out else 1), (name, what)


@pytest.mark.parametrize("name", [c.name for c in nr_inputs.CASES])
def test_device_equals_numpy(name):
    check(name)


@pytest.mark.parametrize("name", [c.name for c in nr_inputs.CASES])
def test_count_only(name):
    c = nr_inputs.BY_NAME[name]
    got, n_out, _, waits = device_expand(c.rec, c.qoff, c.qmem, c.soff, c.smem, count_only=True)
    assert got is None and n_out == len(expected(name)) and waits == (1 if len(c.rec) else 0)


@pytest.mark.parametrize("poison", ["0xFF", "0x5A"])
def test_stale_device_memory_changes_nothing(poison, monkeypatch):
    monkeypatch.setenv("SOHIT_POISON", poison)
    for c in nr_inputs.CASES:
        check(c.name, "SOHIT_POISON=" + poison)


def test_a_short_input_right_behind_a_long_one():
    for name in ("big_700x700", "one_row", "mixed", "empty", "piece_0"):
        check(name, "in a row")


def refused(kw, frag):
    with pytest.raises(RuntimeError) as e:
        device_expand(**kw)
    assert "so_nr_expand" in str(e.value) and frag in str(e.value), str(e.value)
    check("one_row", "after a refusal")          # the next call succeeds


@pytest.mark.parametrize("name", [b[0] for b in nr_inputs.bad_tables()])
def test_bad_tables_are_refused(name):
    _, kw, frag = [b for b in nr_inputs.bad_tables() if b[0] == name][0]
    refused(kw, frag)


@pytest.mark.parametrize("name", [b[0] for b in nr_inputs.bad_records()])
def test_bad_records_are_refused_on_the_device(name):
    _, kw, frag = [b for b in nr_inputs.bad_records() if b[0] == name][0]
    refused(kw, frag)


def test_bad_counts_and_sizes_are_refused():
    from swiftortho_amd import _lib
    L = _lib.load()
    c = nr_inputs.BY_NAME["one_row"]
    ptr = lambda a: C.c_void_p(np.ascontiguousarray(a).ctypes.data)
    res = _lib.SoNrExpandResult()
    nq, ns = len(c.qoff) - 1, len(c.soff) - 1
    for n, n_q, n_s, frag in ((-1, nq, ns, "negative"), (1, -1, ns, "negative"), (1, nq, -1, "negative"), (1 << 31, nq, ns, "2^31")):
        assert L.so_nr_expand(0, C.c_void_p(16), n, ptr(c.qoff), ptr(c.qmem), n_q, ptr(c.soff), ptr(c.smem), n_s, 0, C.byref(res)) != 0
        assert frag in L.so_nr_last_error().decode() and not res.d_out and res.n_out == 0
    assert L.so_nr_expand(0, C.c_void_p(8), 1, ptr(c.qoff), ptr(c.qmem), nq, ptr(c.soff), ptr(c.smem), ns, 0, C.byref(res)) != 0
    assert "aligned" in L.so_nr_last_error().decode()
    assert L.so_nr_expand(99, C.c_void_p(16), 1, ptr(c.qoff), ptr(c.qmem), nq, ptr(c.soff), ptr(c.smem), ns, 0, C.byref(res)) != 0
    assert "device" in L.so_nr_last_error().decode()
    check("one_row", "after the refusals")


def test_an_output_of_2_31_records_is_refused_before_it_is_allocated():
    """46341 x 46341 members: one row expands to 2^31 + 4 893 records; only the count is made"""
    m = 46341
    off = np.array([0, m], dtype=np.int64)
    mem = np.arange(m, dtype=np.int32)
    for count_only in (True, False):
        with pytest.raises(RuntimeError) as e:
            device_expand(nr_inputs.records([0], [0]), off, mem, off, mem, count_only=count_only)
        assert "2^31" in str(e.value)
    check("one_row", "after the refusal")


# ---- the one-process route against the script chain ------------------------------------------------------------------------------

def with_copies(fa, n_copies, heavy, seed):
    """FASTA bytes with n_copies more records that are exact copies of seeded earlier ones -- one sequence `heavy` times in all --,
    under new ids spread over six taxa, shuffled into the file"""
    rs = np.random.RandomState(seed)
    rec = fa.split(b">")[1:]
    seqs = [r.split(b"\n", 1)[1] for r in rec]
    src = [int(rs.randint(len(seqs)))] * (heavy - 1) + rs.randint(0, len(seqs), n_copies - (heavy - 1)).tolist()
    new = [b"t%04d|c%07d\n" % (k % 6, k) + seqs[s] for k, s in enumerate(src)]
    both = rec + new
    return b"".join(b">" + both[i] for i in rs.permutation(len(both)))


@pytest.fixture(scope="module", params=["nr_dups", "synthetic"])
def chain(request, tmp_path_factory):
    """the script chain, once per set: (FASTA path, the .sc file nr.search_collapsed() writes, find_orth's lines on it, search keywords)"""
    from swiftortho_amd import find_orth as fo, nr, synthprot
    d = tmp_path_factory.mktemp(request.param)
    fas = str(d / "p.fsa")
    if request.param == "nr_dups":
        shutil.copy(os.path.join(GOLD, "nr_dups.fsa"), fas)
    else:
        fa = with_copies(synthprot.synthprot(1700, 150, 77), 300, 40, 7)     # 2 000 records, 15 % of them copies
        assert fa.count(b">") == 2000
        open(fas, "wb").write(fa)
    full = nr.search_collapsed(fas, seed="111111", cpus="1", hits="500")
    sc = open(full, "rb").read()
    lines = fo.relations(fo.columns_from_text(sc), .5, 0., "no", "|")
    assert len(lines) > 20
    return fas, sc, lines, nr.collapsed_search_kw("111111", "500")


@pytest.mark.parametrize("stage", [True, "relations"])
def test_orthology_from_search_collapse(chain, stage, tmp_path):
    from swiftortho_amd import pipeline
    fas, sc, lines, kw = chain
    got, t = pipeline.orthology_from_search(fas, device_stage=stage, collapse=True, **kw)
    assert got == lines
    assert {"collapse", "load", "search", "expand", "rows_collapsed", "rows", "find_orth"} <= set(t) and "write_sc" not in t
    assert t["rows"] == sc.count(b"\n") > t["rows_collapsed"] > 0


def test_sc_path_receives_the_chain_s_file(chain, tmp_path):
    from swiftortho_amd import pipeline
    fas, sc, lines, kw = chain
    out = str(tmp_path / "x.sc")
    got, t = pipeline.orthology_from_search(fas, sc_path=out, device_stage="relations", collapse=True, **kw)
    assert got == lines and open(out, "rb").read() == sc and "write_sc" in t
    assert sorted(os.listdir(str(tmp_path))) == ["x.sc"]


def test_groups_from_search_collapse(chain):
    from swiftortho_amd import find_cluster as fc, pipeline
    fas, sc, lines, kw = chain
    text = b"".join(l + b"\n" for l in lines)
    groups, t = pipeline.groups_from_search(fas, collapse=True, **kw)
    assert groups == fc.cnc(text, 1.5) and len(groups) > 3
    assert {"collapse", "expand", "rows_collapsed"} <= set(t) and t["relations"] == len(lines)
    groups, _ = pipeline.groups_from_search(fas, collapse=True, algorithm="apc", **kw)
    assert groups == fc.apc(text, 0.5)


def test_the_device_route_names_the_id_it_refuses(tmp_path):
    from swiftortho_amd import pipeline
    p = str(tmp_path / "x.fsa")
    open(p, "wb").write(b">a|1\nMKVLLAGG\n>b|2\nMKVLLAGG\n>a|1\nGGGMKVLL\n")
    with pytest.raises(ValueError) as e:
        pipeline.orthology_from_search(p, device_stage=True, collapse=True)
    assert "a|1" in str(e.value)


def test_run_all_fast_G_T_writes_the_files_of_G_F(tmp_path):
    """scripts/run_all_fast.py -G T and -G F on nr_dups.fsa: the same .sc, .opc, .xyz and .clsr bytes"""
    files = {}
    for g in "FT":
        d = tmp_path / g
        d.mkdir()
        fas = str(d / "p.fsa")
        shutil.copy(os.path.join(GOLD, "nr_dups.fsa"), fas)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_all_fast.py"), "-i", fas, "-s", "111111", "-a", "1", "-v", "500", "-y", "0", "-G", g],
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        files[g] = {e: open(fas + "_results/p.fsa." + e, "rb").read() for e in ("sc", "opc", "xyz", "clsr")}
        assert not os.path.exists(fas + "_results/p.fsa.grp")
    assert files["T"] == files["F"] and files["F"]["opc"].count(b"\n") > 20 and files["F"]["clsr"]
