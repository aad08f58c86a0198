"""CPU-only: the operon stage (swiftortho_amd/operon.py) against what the REAL scripts/operon_cluster.py printed (tests/golden/operon_*.json,
made by tools/refharness/make_operon_goldens.py), byte for byte, through run() and the script; the two facts the module builds on (the
integer form of the filter, the set order of a list with repeats); order='index'; a literal restatement of the reference's loop against
candidate_pairs() on the designed tables; the refusals so_operon_pairs makes before it looks for a device."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import operon_inputs as oi
from conftest import ROOT

SCRIPT = os.path.join(ROOT, "scripts", "operon_cluster.py")


@pytest.fixture(scope="module")
def operon():
    from swiftortho_amd import operon
    return operon


def write_case(tmp_path, name):
    groups, operons = oi.case_texts(name)
    gr, op = str(tmp_path / "in.groups"), str(tmp_path / "in.operon")
    with open(gr, "w") as f:
        f.write(groups)
    with open(op, "w") as f:
        f.write(operons)
    return gr, op


@pytest.mark.parametrize("name", oi.golden_names())
def test_run_equals_the_reference(operon, tmp_path, name):
    gr, op = write_case(tmp_path, name)
    assert "".join(l + "\n" for l in operon.run(gr, op)) == oi.golden(name)["stdout"]


@pytest.mark.parametrize("name", oi.golden_names())
def test_script_equals_the_reference(tmp_path, name):
    gr, op = write_case(tmp_path, name)
    for argv in (["-g", gr, "-p", op], ["-p" + op, "-g" + gr]):
        r = subprocess.run([sys.executable, SCRIPT] + argv, capture_output=True)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.decode() == oi.golden(name)["stdout"]


def test_script_manual(tmp_path):
    for argv in ([], ["-g", "x.groups"], ["-p", "x.operon"], ["-G", "T"]):
        r = subprocess.run([sys.executable, SCRIPT] + argv, capture_output=True, cwd=str(tmp_path))
        assert r.returncode == 0 and b"Usage:" in r.stdout and b" -g:" in r.stdout and b" -p:" in r.stdout


def golden_rows(operon, name):
    """the golden's lines as (i, j, score text); names are told apart by their place, so this needs distinct operon strings"""
    table = operon.operon_table(*oi.case_texts(name))
    where = {s: k for k, s in enumerate(table.names)}
    assert len(where) == table.n_ops
    rows = [l.split("\t") for l in oi.golden(name)["stdout"].split("\n")[:-1]]
    return table, [(where[a], where[b], s) for a, b, s in rows]


def test_goldens_cover_what_they_claim(operon):
    table, rows = golden_rows(operon, "taxa30")
    assert table.n_ops == 180 and sum(1 for a, b in zip(rows, rows[1:]) if a[0] == b[0] and b[1] < a[1]) >= 2      # the set order is not ascending
    table, rows = golden_rows(operon, "wrap600")
    c = operon.candidate_pairs(table)
    assert np.diff(c.cand_start).max() == 600 and sum(1 for a, b in zip(rows, rows[1:]) if a[0] == b[0] and b[1] < a[1]) > 100
    t = operon.operon_table(*oi.case_texts("fam0"))
    c = operon.candidate_pairs(t)
    assert t.has0.tolist() == [1, 1, 0, 1, 1, 1, 1, 0, 1] and 3 not in c.i.tolist() and 4 not in c.i.tolist()      # family-0 genes alone: no candidates
    assert c.nshr[(c.i == 0) & (c.j == 1)].tolist() == [3] and c.nshr[(c.i == 2) & (c.j == 0)].tolist() == [2]      # N == 3 through family 0 alone
    t = operon.operon_table(*oi.case_texts("header_mid"))
    assert t.n_ops == 3 and t.names[1].startswith("a2")
    t = operon.operon_table(*oi.case_texts("no_newline"))
    assert t.names[-1].endswith("a") and t.length.tolist() == [4, 4, 4, 5]
    t = operon.operon_table(*oi.case_texts("empty_tokens"))
    assert t.length.tolist() == [4, 5, 3, 1, 2, 3, 2] and t.fam[t.start[3]:t.start[4]].tolist() == [5]
    t = operon.operon_table(*oi.case_texts("mixed"))
    assert t.length.tolist() == [3, 3, 3, 3, 2, 4]
    t = operon.operon_table(*oi.case_texts("dups"))
    assert len(set(t.names)) < t.n_ops


def test_filter_is_an_integer_test():
    """for 1 <= len < 400: N / len > .5 in doubles exactly when 2 * N > len, so max(cv0, cv1) > .5 is 2 * N > min(len_i, len_j)"""
    for ln in range(1, 400):
        for n in range(0, ln + 2):
            assert (n * 1. / ln > .5) == (2 * n > ln), (n, ln)


def test_set_order_ignores_repeats():
    """list(set(l)) == list(set(first occurrences of l, in order)): a repeated add changes nothing"""
    rng = random.Random(7)
    for trial in range(3000):
        top = rng.choice((10, 100, 5000, 10 ** 6))
        l = [rng.randrange(top) for _ in range(rng.randint(0, 80))]
        l += [rng.choice(l) for _ in range(rng.randint(0, 80))] if l else []
        rng.shuffle(l)
        assert list(set(l)) == list(set(list(dict.fromkeys(l))))      # (a LIST of them: a set made from a dict is sized ahead and may order otherwise)


@pytest.mark.parametrize("name", oi.golden_names())
def test_index_order_is_the_sorted_reference(operon, name):
    table = operon.operon_table(*oi.case_texts(name))
    i, j, s = operon.operon_pairs(table, "reference")
    a, b, t = operon.operon_pairs(table, "index")
    o = np.lexsort((j, i))
    assert a.tolist() == i[o].tolist() and b.tolist() == j[o].tolist() and t.tolist() == s[o].tolist()
    assert list(zip(a.tolist(), b.tolist())) == sorted(zip(a.tolist(), b.tolist()))
    with pytest.raises(ValueError):
        operon.operon_pairs(table, "ascending")


def reference_loop(t):
    """the reference's loop on a table: dicts, lists and sets -> [(i, j, N, rank)] per operon in order of first occurrence"""
    slices = [t.fam[a:b].tolist() for a, b in zip(t.start[:-1], t.start[1:])]
    operondb = {}
    for i, fams in enumerate(slices):
        for k in fams:
            operondb.setdefault(k, []).append(i)
    rows = []
    for i, fams in enumerate(slices):
        idxs = sum([operondb[k] for k in fams], [])
        group0 = fams + ([0] if t.has0[i] else [])
        for j in dict.fromkeys(idxs):
            group1 = slices[j] + ([0] if t.has0[j] else [])
            rank = min(r for r, k in enumerate(fams) if j in operondb[k])
            rows.append((i, j, len(set(group0).intersection(group1)), rank))
    return rows


@pytest.mark.parametrize("key", sorted(oi.designed()))
def test_candidate_pairs_equal_the_reference_loop(operon, key):
    t = oi.designed()[key][0]
    c = operon.candidate_pairs(t)
    rows = reference_loop(t)
    assert list(zip(c.i.tolist(), c.j.tolist(), c.nshr.tolist(), c.rank.tolist())) == rows
    assert c.cand_start.tolist() == [0] + np.cumsum(np.bincount(np.asarray([r[0] for r in rows], dtype=np.int64), minlength=t.n_ops)).tolist()
    for budget in oi.designed()[key][1]:       # the budgets under which the table calls for more than one batch
        assert oi.expected_batches(t, budget) > 1, (key, budget)


def test_designed_tables_cover_what_they_claim(operon):
    d = oi.designed()
    t = d["lists"][0]
    assert sorted(np.bincount(t.fam)[1:8].tolist()) == [1, 63, 64, 65, 255, 256, 257] and oi.expansion_totals(t)[0] > 1000
    tot = oi.expansion_totals(d["exact"][0])
    assert tot == [0, 3, 4, 0, 4, 4, 0, 0, 17, 32, 0, 32, 33, 1, 0] and sum(tot[:10]) == 64
    # budget 7: 0 3 4 0 | 4 | 4 0 0 | 17 | 32 | 0 | 32 | 33 | 1 0 (an operon above the budget stays alone); 64: .. 32 0 | 32 | 33 1 0
    assert [oi.expected_batches(d["exact"][0], b) for b in (7, 64, 1000)] == [9, 3, 1]
    c = operon.candidate_pairs(d["edges"][0])
    ln = d["edges"][0].length
    n2 = 2 * c.nshr.astype(np.int64) - np.minimum(ln[c.i], ln[c.j])
    assert {2, 3} <= set(c.nshr.tolist()) and ((n2 == 0) & (c.nshr > 2)).any() and ((n2 == 1) & (c.nshr > 2)).any()
    c = operon.candidate_pairs(d["rank_ties"][0])
    assert c.j[c.cand_start[0]:c.cand_start[1]].tolist() == [0, 3, 9, 1, 5]


def test_refusals_that_need_no_device(operon):
    """what so_operon_pairs refuses before it looks for a device; and without a device the call fails loudly: no CPU fallback"""
    import torch
    from swiftortho_amd import build
    build.build(verbose=False)
    t = oi.designed()["rank_ties"][0]
    args = dict(start=t.start, fam=t.fam, length=t.length, has0=t.has0, n_fam=t.n_fam)
    down, late, big, zero, twice, short = t.start.copy(), t.start.copy(), t.fam.copy(), t.fam.copy(), t.fam.copy(), t.length.copy()
    down[3], late[0], big[4], zero[0], twice[1], short[2] = down[2] - 1, 1, t.n_fam, 0, t.fam[0], 0
    for change, word in ((dict(flags=2), "flags"), (dict(flags=-1), "flags"), (dict(start=down), "does not rise"), (dict(start=late), "does not rise"),
                         (dict(fam=big), "a family outside"), (dict(fam=zero), "a family outside"), (dict(fam=-big), "a family outside"),
                         (dict(fam=twice), "repeated"), (dict(length=short), "below 1"), (dict(n_fam=-1), "bad arguments"),
                         (dict(n_ops=-1), "bad arguments"), (dict(n_ops=1 << 31), "2^31 operons"), (dict(start=None, n_ops=3), "NULL"),
                         (dict(length=None, n_ops=3), "NULL"), (dict(has0=None, n_ops=3), "NULL"), (dict(fam=None, n_ops=t.n_ops), "NULL")):
        with pytest.raises(RuntimeError) as e:
            operon.device_operon_pairs(**dict(args, **change))
        assert word in str(e.value), (change, str(e.value))
    many = np.zeros(3, dtype=np.int64)
    many[1:] = 1 << 31
    with pytest.raises(RuntimeError) as e:
        operon.device_operon_pairs(start=many, fam=None, length=t.length[:2], has0=t.has0[:2], n_fam=3, n_ops=2)
    assert "2^31 entries" in str(e.value)
    if not torch.cuda.is_available():
        for flags in (0, 1):
            with pytest.raises(RuntimeError) as e:
                operon.device_operon_pairs(flags=flags, **args)
            assert "HIP" in str(e.value)
        with pytest.raises(RuntimeError):
            operon.operon_pairs(t, device_stage=True)
