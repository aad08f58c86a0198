"""The collapse / expand TABLES of swiftortho_amd/nr.py (CPU): collapse_tables() against the output of the REAL nr_flt.py, expand_records()
-- the numpy definition the device stage is compared with in test_gpu_nr.py -- against the output of the REAL nr2full.py (the goldens
of tools/refharness/make_nr_goldens.py) and against the text nr2full() on every designed input of nr_inputs.py."""
import inspect
import os
import re

import numpy as np
import pytest

import nr_inputs
from conftest import GOLD, ROOT
from swiftortho_amd import nr


def _name(side, ordinal):
    return "%s%d|x" % (side, ordinal)


def _mid(rec_row):
    return [repr(rec_row[f].item()) for f in nr_inputs.MID]


def collapsed_text(case):
    """the case as the 16-column rows of a collapsed search (a helper of the test: ids q<ordinal>|x / s<ordinal>|x)"""
    rows = []
    for r in case.rec:
        q, s = int(r["qidx"]), int(r["sidx"])
        qh = nr.JOIN.join(_name("q", m) for m in case.qmem[case.qoff[q]:case.qoff[q + 1]])
        sh = nr.JOIN.join(_name("s", m) for m in case.smem[case.soff[s]:case.soff[s + 1]])
        rows.append("\t".join([qh, sh] + _mid(r) + [str(q), sh]) + "\n")
    return rows


def expanded_text(rec, case):
    """the expanded records as nr2full's rows.  The twelve middle columns are rendered once per SOURCE row and looked up through the
    record's aln (= 12 * row + 1, nr_inputs.records) -- after checking that every middle field of every record is that row's"""
    src = rec["aln"] // 12
    for f in nr_inputs.MID:
        assert np.array_equal(rec[f], case.rec[f][src]), f
    mids = ["\t".join(_mid(r)) for r in case.rec]
    names = [(_name("q", a), _name("s", b)) for a, b in zip(rec["qidx"].tolist(), rec["sidx"].tolist())]
    return ["\t".join([q, s, mids[j], q, s]) for (q, s), j in zip(names, src.tolist())]


def closed_form(case, deviation=None):
    """position -> (qidx, sidx, source row) by the closed form, one record at a time; `deviation` breaks it in one place"""
    rec, out = case.rec, {}
    q = rec["qidx"].tolist()
    s = rec["sidx"].tolist()
    nj = [int(case.soff[x + 1] - case.soff[x]) for x in s]
    base = P = 0
    i = 0
    while i < len(q):
        e = i
        while e < len(q) and q[e] == q[i]:
            e += 1
        members = case.qmem[case.qoff[q[i]]:case.qoff[q[i] + 1]].tolist()
        k, S = len(members), sum(nj[i:e])
        if deviation != "P_not_reset":
            P = 0
        for j in range(i, e):
            subj = case.smem[case.soff[s[j]]:case.soff[s[j] + 1]].tolist()
            for a in range(k):
                for b in range(nj[j]):
                    pos = base + (k * P + a * nj[j] + b if deviation == "row_major" else a * S + P + b)
                    out[pos] = (members[a], subj[b], j)
            P += nj[j]
        base += S if deviation == "base_from_nj" else k * S
        i = e
    return out


def as_positions(rec):
    return {p: (int(r["qidx"]), int(r["sidx"]), int(r["aln"]) // 12) for p, r in enumerate(rec)}   # (aln = 12 * row + 1: nr_inputs.records)


@pytest.fixture(scope="module")
def expanded():
    return {c.name: nr.expand_records(c.rec, c.qoff, c.qmem, c.soff, c.smem) for c in nr_inputs.CASES}


def test_collapse_tables_give_the_real_nr_flt_output():
    data = open(os.path.join(GOLD, "nr_dups.fsa"), "rb").read()
    t = nr.collapse_tables(data)
    assert t.fasta == open(os.path.join(GOLD, "nr_dups.nr.fsa"), "rb").read()
    assert t.fasta == "".join(l + "\n" for l in nr.nr_flt(data.decode().splitlines(True))).encode()
    t2 = nr.collapse_tables(data.decode().splitlines(True))
    assert t2.fasta == t.fasta and t2.ids == t.ids and np.array_equal(t2.mem, t.mem)
    recs = list(nr.fasta_records(data.decode().splitlines(True)))
    assert t.ids == [h.split()[0].encode() for h, _ in recs]
    n_distinct = len(t.off) - 1
    assert n_distinct == len({s for _, s in recs}) < len(recs) == len(t.rep_of) == len(t.mem)
    assert t.off.dtype == np.int64 and t.mem.dtype == np.int32 and t.off[0] == 0 and t.off[-1] == len(recs)
    first = [int(np.flatnonzero(t.rep_of == d)[0]) for d in range(n_distinct)]
    assert first == sorted(first)                                    # numbered by first appearance
    for d in range(n_distinct):
        m = t.mem[t.off[d]:t.off[d + 1]]
        assert m.tolist() == np.flatnonzero(t.rep_of == d).tolist()  # file order
        assert len({recs[i][1] for i in m}) == 1


def test_collapse_tables_by_hand():
    fa = b">a|1 first protein\nMKV\nLLA\n>b|2\nGGG\n>c|3 same as a\nMKVLLA\n>d|4\nGGG\n>e|5\nMKVLLa\n"
    t = nr.collapse_tables(fa)
    assert t.fasta == b">a|1;;;c|3\nMKVLLA\n>b|2;;;d|4\nGGG\n>e|5\nMKVLLa\n"       # case-sensitive
    assert t.ids == [b"a|1", b"b|2", b"c|3", b"d|4", b"e|5"]
    assert t.rep_of.tolist() == [0, 1, 0, 1, 2] and t.off.tolist() == [0, 2, 4, 5] and t.mem.tolist() == [0, 2, 1, 3, 4]
    e = nr.collapse_tables(b"")
    assert e.fasta == b"" and e.ids == [] and e.off.tolist() == [0] and len(e.mem) == 0
    assert "host" in nr.collapse_tables.__doc__ and "device" in nr.collapse_tables.__doc__   # why the grouping is not a kernel


@pytest.mark.parametrize("fasta, what", [(b">a|1\nMK\n> \nGG\n", "empty"), (b">a|1\nMK\n>\nGG\n", "empty"), (b">a|1\nMK\n>b;;;c|2\nGG\n", "b;;;c|2"),
                                         (b">a|1 x\nMK\n>b|2\nGG\n>a|1 y\nMKK\n", "a|1")])
def test_ids_the_device_route_refuses(fasta, what):
    """nr2full keys on id strings, the device on record numbers: where the two stop agreeing the tables are refused, and the id is named;
    the text route keeps serving the file"""
    with pytest.raises(ValueError) as e:
        nr.collapse_tables(fasta)
    assert what in str(e.value)
    assert nr.nr_flt(fasta.decode().splitlines(True))


def test_expand_records_pinned_to_the_real_nr2full():
    """nr_dups.nr.sc (rows of the collapsed search) -> records, collapsed names mapped to ordinals -> expand_records -> compared with
    nr_dups.full.sc, the output of the REAL nr2full.py, row for row IN ORDER: the two ids, columns 3-14, and the number of rows"""
    t = nr.collapse_tables(open(os.path.join(GOLD, "nr_dups.fsa"), "rb").read())
    header = {nr.JOIN.join(t.ids[m].decode() for m in t.mem[t.off[d]:t.off[d + 1]]): d for d in range(len(t.off) - 1)}
    rows = [l[:-1].split("\t") for l in open(os.path.join(GOLD, "nr_dups.nr.sc"))]
    rec = nr_inputs.records([header[r[0]] for r in rows], [header[r[1]] for r in rows])   # aln = 12 * row + 1 names the source row
    assert len({r[0] for r in rows}) > 20 and any(nr.JOIN in r[0] for r in rows) and any(nr.JOIN in r[1] for r in rows)
    out = nr.expand_records(rec, t.off, t.mem, t.off, t.mem)
    want = [l[:-1].split("\t") for l in open(os.path.join(GOLD, "nr_dups.full.sc"))]
    assert len(out) == len(want) > len(rows)
    for r, w in zip(out, want):
        src = rows[int(r["aln"]) // 12]
        assert [t.ids[r["qidx"]].decode(), t.ids[r["sidx"]].decode()] + src[2:14] == w[:14]
    for f in nr_inputs.MID:                                         # every other field is the source row's
        assert np.array_equal(out[f], rec[f][out["aln"] // 12])


@pytest.mark.parametrize("name", [c.name for c in nr_inputs.CASES if c.text])
def test_expand_records_equal_the_text_nr2full(name, expanded):
    case = nr_inputs.BY_NAME[name]
    assert expanded_text(expanded[name], case) == nr.nr2full(collapsed_text(case))


@pytest.mark.parametrize("name", [c.name for c in nr_inputs.CASES])
def test_expand_records_equal_the_closed_form(name, expanded):
    case, out = nr_inputs.BY_NAME[name], expanded[name]
    want = closed_form(case)
    assert len(out) == len(want) and as_positions(out) == want
    src = out["aln"] // 12
    for f in nr_inputs.MID:
        assert np.array_equal(out[f], case.rec[f][src])
    assert out.dtype == nr_inputs.HIT


def test_the_designed_inputs_cover_what_they_claim(expanded):
    assert len(expanded["empty"]) == 0 and len(expanded["one_row"]) == 1
    ones = nr_inputs.BY_NAME["ones"]
    assert len(expanded["ones"]) == len(ones.rec) > 256 * 256 and np.array_equal(expanded["ones"]["evalue"], ones.rec["evalue"])
    assert np.array_equal(expanded["ones"]["qidx"], ones.qmem[ones.rec["qidx"]]) and not np.array_equal(expanded["ones"]["qidx"], ones.rec["qidx"])
    assert len(expanded["big_700x700"]) == 490000
    mixed = nr_inputs.BY_NAME["mixed"]
    k = (mixed.qoff[1:] - mixed.qoff[:-1])[mixed.rec["qidx"]]
    n = (mixed.soff[1:] - mixed.soff[:-1])[mixed.rec["sidx"]]
    assert {(a, b) for a in (1, 2, 3, 65) for b in (1, 2, 63, 64, 65, 700)} <= set(zip(k.tolist(), n.tolist()))
    assert len(expanded["empty_groups"]) == 2 * 3 + 1 * 4


# one deviation of the closed form at a time, and the designed input that catches it (base_from_nj shows behind a run with k > 1)
DEVIATIONS = [("row_major", "mixed"), ("row_major", "row_edges"), ("P_not_reset", "row_edges"), ("P_not_reset", "piece_p1"), ("base_from_nj", "mixed"),
              ("base_from_nj", "row_edges")]


@pytest.mark.parametrize("deviation, name", DEVIATIONS)
def test_single_deviations_are_caught(deviation, name, expanded):
    """member-major swapped with row-major, P not reset at a run start, base from n_j instead of k * n_j: each gives other records on
    the named input than expand_records does"""
    assert closed_form(nr_inputs.BY_NAME[name], deviation) != as_positions(expanded[name])


def test_bad_tables_and_records_are_refused():
    for name, kw, frag in nr_inputs.bad_tables() + nr_inputs.bad_records():
        with pytest.raises(ValueError) as e:
            nr.expand_records(**kw)
        assert frag[:4] in str(e.value), name


def test_piece_constant_is_the_kernels():
    src = open(os.path.join(ROOT, "swiftortho_amd", "csrc", "nr.hip")).read()
    assert int(re.search(r"#define NR_PIECE (\d+)", src).group(1)) == nr.EXPAND_PIECE == nr_inputs.PIECE


def test_the_pipeline_has_the_new_keyword(tmp_path):
    from swiftortho_amd import pipeline
    for f in (pipeline.orthology_from_search, pipeline.groups_from_search):
        assert inspect.signature(f).parameters["collapse"].default is False
    with pytest.raises(ValueError):                                  # refused before the file is opened
        pipeline.orthology_from_search(str(tmp_path / "missing.fsa"), collapse=True)
    assert "nothing here touches the device" not in nr.__doc__
