"""CPU tests of the CIGAR side: the library's formatter (so_format_cigar, no device), fsearch.cigar_to_strings against the fixtures'
own string builder, find_orth on a 17-column file, and the entry points without a device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLD

from test_aln_fixtures import NAMES, aln_edge_cases, aln_strings, records

M, I, D = 0, 1, 2


@pytest.fixture(scope="module")
def fs():
    from swiftortho_amd import build
    build.build(verbose=False)
    from swiftortho_amd import fsearch
    return fsearch


def runs(*pairs):
    return np.array([n << 4 | op for n, op in pairs], dtype=np.uint32)


def test_format_cigar(fs):
    assert fs.format_cigar(runs((35, M), (2, D), (10, M))) == "35M2D10M"
    assert fs.format_cigar(runs((1, I))) == "1I"
    assert fs.format_cigar(runs()) == ""
    assert fs.format_cigar(runs(((1 << 28) - 1, M))) == "268435455M"
    assert fs.format_cigar(runs(((1 << 28) - 1, D), (1, M), ((1 << 28) - 1, I))) == "268435455D1M268435455I"
    # the text is what the runs say, canonical or not; a run of no columns or an unknown operation is no CIGAR
    assert fs.format_cigar(runs((3, M), (4, M))) == "3M4M"
    for bad in (runs((0, M)), runs((5, 3)), runs((5, M), (7, 15))):
        with pytest.raises(ValueError):
            fs.format_cigar(bad)


def test_format_cigar_c_interface(fs):
    """the size it needs, at most cap - 1 characters and a NUL, NULL buffers"""
    L = fs._lib.load()
    r = runs((35, M), (2, D), (10, M))
    assert L.so_format_cigar(r.ctypes.data, 3, None, 0) == 8
    buf = C.create_string_buffer(b"#" * 16, 16)
    assert L.so_format_cigar(r.ctypes.data, 3, buf, 16) == 8 and buf.raw[:9] == b"35M2D10M\0" and buf.raw[9:] == b"#" * 7
    buf = C.create_string_buffer(b"#" * 16, 16)
    assert L.so_format_cigar(r.ctypes.data, 3, buf, 4) == 8 and buf.raw[:5] == b"35M\0#"
    assert L.so_format_cigar(None, 0, None, 0) == 0
    assert L.so_format_cigar(None, 2, None, 0) == -1 and L.so_format_cigar(r.ctypes.data, -1, None, 0) == -1


def test_cigar_to_strings(fs):
    q, s = b"ACDEFGHIKL", b"ACDFGHWWIKL"
    assert fs.cigar_to_strings("3M1I3M2D3M", q, s, 1, 1) == (b"ACDEFGH--IKL", b"ACD-FGHWWIKL")
    assert fs.cigar_to_strings(runs((3, M), (1, I), (3, M), (2, D), (3, M)), q, s, 1, 1) == (b"ACDEFGH--IKL", b"ACD-FGHWWIKL")
    assert fs.cigar_to_strings(b"2M", "ACDEFGHIKL", "ACDFGHWWIKL", 9, 10) == (b"KL", b"KL")
    assert fs.cigar_to_strings("", q, s, 1, 1) == (b"", b"") == fs.cigar_to_strings(runs(), q, s, 4, 4)
    # non-canonical input is accepted: split runs, runs of no columns
    assert fs.cigar_to_strings("1M2M0D1I0M3M1D1D3M", q, s, 1, 1) == fs.cigar_to_strings("3M1I3M2D3M", q, s, 1, 1)
    # a literal '-' residue is a residue
    assert fs.cigar_to_strings("2M1D2M", b"A-CD", b"A-WCD", 1, 1) == (b"A--CD", b"A-WCD")
    # a long run only needs its sequences
    big = (1 << 28) - 1
    for bad in ("11M", "%dM" % big, "3M9I", "3M10D", runs((big, M))):
        with pytest.raises(ValueError):
            fs.cigar_to_strings(bad, q, s, 1, 1)
    for bad in ("3", "M", "3X", "3M4", "3=", "-3M"):
        with pytest.raises(ValueError):
            fs.cigar_to_strings(bad, q, s, 1, 1)
    with pytest.raises(ValueError):
        fs.cigar_to_strings("3M", q, s, 0, 1)
    assert fs.format_cigar(runs(*[(n, "MID".index(op)) for n, op in fs.parse_cigar("3M1I3M2D3M")])) == "3M1I3M2D3M"


@pytest.mark.parametrize("name", NAMES)
def test_cigar_to_strings_on_every_golden_cigar(fs, oracle, name):
    """every CIGAR of the aln_<name>.json fixtures: the strings test_aln_fixtures.aln_strings builds, column for column"""
    gold = json.load(open(os.path.join(GOLD, "aln_%s.json" % name)))
    meta = json.load(open(os.path.join(GOLD, name + ".json")))
    ref = open(os.path.join(GOLD, name + ".ref.fsa"), "rb").read()
    qry = open(os.path.join(GOLD, name + ".qry.fsa"), "rb").read() if meta.get("separate_query") else ref
    seg = dict(zip(meta["flags"][0::2], meta["flags"][1::2])).get("-F", "T") == "T"
    qs, ss = records(qry), records(ref)
    rows = [r for r in open(os.path.join(GOLD, name + ".sc"), "rb").read().split(b"\n") if r]
    assert len(gold["rows"]) > 0
    for k, cig in gold["rows"]:
        c = rows[k].split(b"\t")
        q = qs[c[0]][0]
        q = oracle.seg(q) if seg else q
        q = q if isinstance(q, bytes) else q.encode("latin-1")
        got = fs.cigar_to_strings(cig, q, ss[c[1]][0], int(c[6]), int(c[8]))
        assert got == aln_strings(cig, q, ss[c[1]][0], int(c[6]), int(c[8])), (name, k)
        assert len(got[0]) == len(got[1]) == int(c[3]), (name, k)
        # the three length sums of a row's CIGAR
        p = fs.parse_cigar(cig)
        assert sum(n for n, op in p if op != "D") == int(c[7]) - int(c[6]) + 1 and sum(n for n, op in p if op != "I") == int(c[9]) - int(c[8]) + 1


def test_cigar_to_strings_on_the_edge_fixture(fs):
    cases = aln_edge_cases()
    n = 0
    for c in cases:
        if c["out"] is None:
            assert not c["cigar"]
            continue
        assert fs.cigar_to_strings(c["cigar"], c["qw"], c["sw"], c["out"][4] + 1, c["out"][6] + 1) == c["strings"]
        n += 1
    assert n >= 180


def test_find_orth_reads_a_17_column_file(fs, oracle, tmp_path):
    """a golden .sc with the golden CIGARs appended as a 17th column gives the relations of the 16-column file"""
    from swiftortho_amd import find_orth as fo
    total = 0
    for name in ("toy_default", "het_w6"):
        gold = json.load(open(os.path.join(GOLD, "aln_%s.json" % name)))
        sc = os.path.join(GOLD, name + ".sc")
        rows = [r for r in open(sc, "rb").read().split(b"\n") if r]
        cig = dict((k, c) for k, c in gold["rows"])
        assert len(cig) == len(rows)
        wide = tmp_path / (name + ".sc17")
        wide.write_bytes(b"".join(r + b"\t" + cig[k].encode() + b"\n" for k, r in enumerate(rows)))
        assert all(l.count(b"\t") == 16 for l in wide.read_bytes().split(b"\n") if l)
        for extra in ([], ["-c", "0.3", "-y", "10"]):
            a = fo.parse(["find_orth.py", "-i", sc] + extra)
            want = fo.find_orth(open(sc), float(a["-c"]), float(a["-y"]), a["-n"], a["-s"])
            got = fo.find_orth(open(str(wide)), float(a["-c"]), float(a["-y"]), a["-n"], a["-s"])
            assert got == want
            total += len(want)
    assert total > 20


def test_cigar_entry_points_without_a_context(fs):
    """no context -- which is what a machine without a HIP device leaves a caller with -- : the CIGAR entry points fail like
    so_search_loaded does, and the message is so_create's"""
    import torch
    L = fs._lib.load()
    hits, n = C.POINTER(fs._lib.SoHit)(), C.c_int64(0)
    ops, off = C.c_void_p(), C.c_void_p()
    want = L.so_search_loaded(None, -1, -1, C.byref(hits), C.byref(n))
    assert want != 0
    assert L.so_search_loaded_cigar(None, -1, -1, C.byref(hits), C.byref(n), C.byref(ops), C.byref(off)) == want
    assert L.so_write_sc_cigar(None, hits, 0, None, None, b"/nonexistent/x", b"w") == want
    assert L.so_align_pairs_cigar(None, 3, 0, None, None, None, C.byref(ops), C.byref(off)) == want
    if not torch.cuda.is_available():
        with pytest.raises(fs.SohitError) as e:
            fs.Searcher(ht=1000003)
        assert "HIP" in str(e.value)
        assert L.so_last_error(None).decode() == str(e.value)


def test_flag_table_carries_the_cigar_switch():
    from swiftortho_amd import find_hit as fh
    assert fh.DEFAULTS["-C"] == "F"
    base = ["find_hit.py", "-p", "blastp", "-i", "q.fsa", "-d", "r.fsa", "-o", "x.sc"]
    assert fh.resolve(fh.parse(base))["cigar"] is False
    assert fh.resolve(fh.parse(base + ["-C", "T"]))["cigar"] is True and fh.resolve(fh.parse(base + ["-Ct"]))["cigar"] is True
    assert fh.resolve(fh.parse(base + ["-C", "F"]))["cigar"] is False


def test_one_emission_state_per_search(fs):
    """alignments=True and cigar=True in one call are refused before anything runs (no context needed to say so)"""
    s = fs.Searcher.__new__(fs.Searcher)
    with pytest.raises(ValueError):
        fs.Searcher.search(s, alignments=True, cigar=True)
    with pytest.raises(ValueError):
        fs.Searcher.align_pairs(s, [(0, 0, 0, 0, -1, -1)], 3, alignments=True, cigar=True)
