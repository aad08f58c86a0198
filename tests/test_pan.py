"""CPU-only: the pan-genome stage (swiftortho_amd/pan.py) against what the REAL scripts/pan_genome.py printed and wrote
(tests/golden/pan_*.json, made by tools/refharness/make_pan_goldens.py): the `# Number` line, the family table and the _xy.txt text, byte
for byte, with the taxon order the reference's own process had; the quirks of the member table; the script; and a table of single
deviations from the definition, each shown to change the output of a named golden."""
import os
import random
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import pan_inputs as pi
from conftest import ROOT

SCRIPT = os.path.join(ROOT, "scripts", "pan_genome.py")


@pytest.fixture(scope="module")
def pan():
    from swiftortho_amd import pan
    return pan


def library_result(pan, name, device_stage=False):
    """-> (taxa, MemberTable, PanResult) of a golden's input with the golden's taxon order"""
    fasta, groups, allow_text, flags = pi.case_texts(name)
    meta = pi.golden(name)
    allow = set(l.strip() for l in allow_text.split("\n")[:-1]) if allow_text else None
    taxa = meta["taxa"]
    assert sorted(taxa) == sorted(pan.taxa_of_fasta(fasta, allow))
    table = pan.member_table(fasta, groups, taxa, allow)
    ts, tc = pi.flag_values(flags)
    return taxa, table, pan.pan_genome(table, len(taxa), ts, tc, device_stage=device_stage)


def check_against_golden(pan, name, taxa, table, res):
    meta = pi.golden(name)
    assert pan.number_line(res.totals, table.n_rows, table.n_file_rows, len(taxa)) == meta["number"]
    assert "\n".join(pan.table_lines(taxa, res.types, res.counts)) + "\n" == meta["table"]
    assert pan.xy_text(res.core, res.spec, res.panz) == meta["xy"]
    lines = pan.report_lines(taxa, res, table.n_file_rows, "x_xy.txt")
    assert meta["number"] in lines and "\n".join(lines[lines.index("\t".join(["#family", "type"] + taxa)):]) + "\n" == meta["table"]


@pytest.mark.parametrize("name", pi.golden_names())
def test_numpy_definitions_equal_the_reference(pan, name):
    taxa, table, res = library_result(pan, name)
    check_against_golden(pan, name, taxa, table, res)


def test_goldens_cover_what_they_claim(pan):
    """the regimes the fixtures are there for do occur in them"""
    assert 0.07 * 100 > 7 and 0.29 * 100 < 29                      # floats and fractions part at j = 100 ...
    S, Cc = pan.step_thresholds(.29, .07, 100)
    assert (S[99], Cc[99]) == (27, 8) and (S[49], Cc[49]) == (13, 4)   # ... (exact: 28 and 7) and agree elsewhere (j = 50: 14.5 - 1, 3.5)
    assert pan.type_thresholds(0., .95, 7) == (1, 7) and pan.type_thresholds(.05, 1., 7) == (1, 1) and pan.type_thresholds(2., 5., 9) == (2, 5)
    _, table, res = library_result(pan, "rfile")
    assert (res.counts[:table.n_file_rows].sum(1) == 0).any()      # the -r file empties rows
    _, table, res = library_result(pan, "quirks")
    assert res.counts.max() == 2 and table.n_rows - table.n_file_rows == 3
    for name in ("default", "frac", "abs", "float100", "wide65"):
        _, table, res = library_result(pan, name)
        assert len(set(res.types[:table.n_file_rows].tolist())) >= 2, name
    assert pi.golden("taxa2")["xy"].count("\n") == 20 and not pi.case_texts("no_newline")[1].endswith("\n")
    # u0: Tc = 0, so every row is core at every step of every order, also those no genome so far holds, and nothing behind the last
    # row of the last tile
    taxa, table, res = library_result(pan, "u0")
    S, Cc = pan.step_thresholds(*pi.flag_values(pi.case_texts("u0")[3]), n_taxa=len(taxa))
    assert table.n_rows % 64 != 0 and (table.n_rows, len(taxa)) == (75, 7) and not Cc[1:].any()
    assert res.core.shape == (20, 6) and (res.core == table.n_rows).all() and (res.panz[:, :-1] < table.n_rows).all()
    assert [l.split("\t")[1] for l in pi.golden("u0")["xy"].split("\n")[:-1]] == [str(table.n_rows)] * 120
    assert pan.type_thresholds(.05, 0., 7) == (1, 0) and pi.golden("u0")["number"] == "# Number\t44\t0\t31\t7"
    # l_huge: S is the 32-bit clamp at every step, so every row the next genome holds is new
    taxa, table, res = library_result(pan, "l_huge")
    S, Cc = pan.step_thresholds(*pi.flag_values(pi.case_texts("l_huge")[3]), n_taxa=len(taxa))
    assert (S[1:] == 2147483647).all() and pan.type_thresholds(1e12, .95, 7)[0] == 2147483647 and res.totals == (0, 0, table.n_file_rows)
    present = res.counts > 0
    assert res.spec.tolist() == [[int(present[:, t].sum()) for t in order[1:]] for order in pan.permutations(7).tolist()]


def test_member_table_quirks(pan):
    fasta, groups = pi.QUIRKS_FASTA, pi.QUIRKS_GROUPS
    assert pan.taxa_of_fasta(fasta) == ["a", "b", "c"] and pan.fasta_ids(fasta)[:4] == ["a|1", "a|2", "b|1", "b|2"]
    t = pan.member_table(fasta, groups, ["c", "a", "b"])
    counts = pan.count_matrix(t.row, t.taxon, t.n_rows, 3)
    # a member listed twice counts twice; b|1 stands in two groups; the rows behind the file rows: a|3, c|3, b|3 in file order
    assert counts.tolist() == [[1, 2, 1], [1, 0, 1], [0, 1, 1], [0, 1, 0], [1, 0, 0], [0, 0, 1]] and t.n_file_rows == 3
    # no final newline: the last member loses its last character, so the gene it named gets a row of its own
    t2 = pan.member_table(fasta, groups[:-1], ["a", "b", "c"])
    assert t2.n_rows == t.n_rows + 1 and pan.group_lists(groups[:-1])[-1] == ["a|2", "b|"]
    # a filtered-out taxon: its members are skipped, its genes get no row, the file rows stay
    t3 = pan.member_table(fasta, groups, ["a", "c"], {"a", "c", "nobody"})
    assert t3.n_file_rows == 3 and t3.n_rows == 5 and pan.count_matrix(t3.row, t3.taxon, 5, 2).tolist() == [[2, 1], [0, 1], [1, 0], [1, 0], [0, 1]]
    assert pan.taxa_of_fasta(fasta, {"a", "c", "nobody"}) == ["a", "c"]
    # a member of a taxon the FASTA does not have: refused (the script raises KeyError)
    with pytest.raises(ValueError) as e:
        pan.member_table(fasta, "a|1\tz|9\n", ["a", "b", "c"])
    assert "z|9" in str(e.value) and "KeyError" in str(e.value)
    # a header line that ends the file without a newline loses its last character as a taxon, not as an id
    assert pan.taxa_of_fasta(">abc") == ["ab"] and pan.fasta_ids(">abc") == ["abc"]
    assert pan.permutations(5, 3).tolist() == pan.permutations(5, 20)[:3].tolist() and sorted(pan.permutations(5, 1)[0].tolist()) == list(range(5))
    with pytest.raises(ValueError):
        pan.thresholds(float("nan"), .95, 3)


def run_script(tmp_path, name, extra=()):
    fasta, groups, allow, flags = pi.case_texts(name)
    fa, gr = str(tmp_path / "in.fsa"), str(tmp_path / "in.clsr")
    open(fa, "w").write(fasta), open(gr, "w").write(groups)
    argv = ["-i", fa, "-g", gr] + flags
    if allow is not None:
        open(str(tmp_path / "taxa.txt"), "w").write(allow)
        argv += ["-r", str(tmp_path / "taxa.txt")]
    r = subprocess.run([sys.executable, SCRIPT] + argv + list(extra), capture_output=True, cwd=str(tmp_path))
    xy = open(gr + "_xy.txt").read() if os.path.isfile(gr + "_xy.txt") else None
    return r, xy, gr + "_xy.txt"


def script_equals_library(pan, tmp_path, name, extra=()):
    r, xy, xy_name = run_script(tmp_path, name, extra)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.decode()
    head = [l for l in out.split("\n") if l.startswith("#family")]
    taxa = head[0].split("\t")[2:]
    fasta, groups, allow_text, flags = pi.case_texts(name)
    allow = set(l.strip() for l in allow_text.split("\n")[:-1]) if allow_text else None
    table = pan.member_table(fasta, groups, taxa, allow)
    res = pan.pan_genome(table, len(taxa), *pi.flag_values(flags))
    assert out == "".join(l + "\n" for l in pan.report_lines(taxa, res, table.n_file_rows, xy_name))
    assert xy == pan.xy_text(res.core, res.spec, res.panz)     # (the orders shuffle COLUMNS: the curves belong to the order this process had)
    assert pi.golden(name)["number"] in out.split("\n")
    return out, xy


@pytest.mark.parametrize("name", ["default", "desc", "rfile", "float100", "quirks"])
def test_script_equals_the_library_in_the_order_it_printed(pan, tmp_path, name):
    script_equals_library(pan, tmp_path, name)


def test_script_manual_and_bad_numbers(tmp_path):
    for argv in ([], ["-i", "x.fsa"], ["-g", "x.clsr"], ["-i", "x.fsa", "-g", "x.clsr", "-l", "much"]):
        r = subprocess.run([sys.executable, SCRIPT] + argv, capture_output=True, cwd=str(tmp_path))
        assert r.returncode == 0 and r.stdout.startswith(b"Usage:") and b" -g:" in r.stdout and b" -r:" in r.stdout


def test_refusals_that_need_no_device(pan):
    """what so_pan_genome refuses before it looks for a device; and without a device the call fails loudly: no CPU fallback"""
    import torch
    from swiftortho_amd import build
    build.build(verbose=False)
    t = pi.designed_table(60, 5, 3)
    args = dict(row=t.row, taxon=t.taxon, n_rows=t.n_rows, n_file_rows=t.n_file_rows, n_taxa=3, spec_max=1, core_min=3, perm=pan.permutations(3),
                S=np.zeros(3, dtype=np.int32), C=np.zeros(3, dtype=np.int32))
    for change, word in ((dict(flags=1), "flags"), (dict(perm=np.zeros((20, 3), dtype=np.int32)), "not a permutation"),
                         (dict(perm=np.tile(np.array([0, 1, 3], dtype=np.int32), (20, 1))), "not a permutation"),
                         (dict(n_rows=1 << 31, n_file_rows=0), "2^31 rows"), (dict(n_rows=(1 << 30), n_file_rows=0), "count matrix of 2^31 cells")):
        with pytest.raises(RuntimeError) as e:
            pan.device_pan_genome(**dict(args, **change))
        assert word in str(e.value), (change, str(e.value))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError) as e:
            pan.device_pan_genome(**args)
        assert "HIP" in str(e.value)


# ---------------------------------------------------------------------------------------------------------
# single deviations: the definition is pinned only if each of them shows
# ---------------------------------------------------------------------------------------------------------
def curves_text(pan, counts, ts, tc, variant=None):
    """_xy.txt by a plain loop; `variant` names ONE deviation from the definition"""
    x = (np.asarray(counts) > 0).astype(np.int64)
    d = x.shape[1]
    if variant == "mask":             # core counted over whole tiles of 64 rows: the rows behind the table count as zeros
        x = np.concatenate([x, np.zeros((-len(x) % 64, d), dtype=np.int64)])
    if variant == "fresh_idx":        # every shuffle starts from 0 .. d - 1 instead of from the last order
        rng = random.Random(42)
        perm = []
        for _ in range(20):
            idx = list(range(d))
            rng.shuffle(idx)
            perm.append(idx)
    else:
        perm = pan.permutations(d).tolist()
    rows = {}
    for p, order in enumerate(perm):
        ys = x[:, order[0]].copy()
        for i in range(1, d):
            j = i + 1
            if variant == "exact":    # thresholds from exact fractions of the flags' decimal text
                fs, fc = Fraction(repr(ts)), Fraction(repr(tc))
                Ts, Tc = (max(fs * j, 1) if fs < 1 else fs), (fc * j if fc < 1 else fc)
            else:
                Ts, Tc = pan.thresholds(ts, tc, j)
            yn = x[:, order[i]]
            cut = Ts if variant == "numexpr" else Ts - 1          # the branch the script takes with numexpr
            if variant == "exact":    # (integers on both sides: numpy never meets a Fraction)
                cut, Tc = cut.__floor__(), Tc.__ceil__()
            old = (ys < cut) if variant == "less" else (ys <= cut)
            spec = int((old & (yn > 0)).sum())
            ys = ys + yn
            if variant == "spec_after_add":
                spec = int(((ys <= cut) & (yn > 0)).sum())
            core = int((ys > Tc).sum()) if variant == "core_greater" else int((ys >= Tc).sum())
            rows[(j, p)] = (core, spec, int((ys > 0).sum()))
    return "".join("%d\t%d\t%d\t%d\n" % ((j,) + rows[(j, p)]) for j in range(2, d + 1) for p in range(20))


DEVIATIONS = [("numexpr", "default"), ("less", "frac"), ("spec_after_add", "default"), ("exact", "float100"), ("fresh_idx", "default"),
              ("mask", "u0"), ("core_greater", "u0")]


@pytest.mark.parametrize("variant,name", DEVIATIONS)
def test_single_deviations_change_the_output(pan, variant, name):
    taxa, table, res = library_result(pan, name)
    ts, tc = pi.flag_values(pi.case_texts(name)[3])
    want = pi.golden(name)["xy"]
    assert curves_text(pan, res.counts, ts, tc) == want
    assert curves_text(pan, res.counts, ts, tc, variant) != want


def test_exact_fractions_part_only_where_the_floats_do(pan):
    """on float100 the exact-fraction thresholds change the lines of j = 100 (0.07 * 100 and 0.29 * 100) and of the other j at which a
    float product misses its fraction -- and leave the default case alone"""
    taxa, table, res = library_result(pan, "float100")
    a, b = pi.golden("float100")["xy"].split("\n"), curves_text(pan, res.counts, .29, .07, "exact").split("\n")
    diff = sorted(set(int(x.split("\t")[0]) for x, y in zip(a, b) if x != y))
    assert 100 in diff
    for j in range(2, 101):
        parts = (Fraction("0.29") * j - 1).__floor__() != int(np.floor(.29 * j - 1)) or (Fraction("0.07") * j).__ceil__() != int(np.ceil(.07 * j))
        assert parts or j not in diff, j
    taxa, table, res = library_result(pan, "default")
    assert curves_text(pan, res.counts, .05, .95, "exact") == pi.golden("default")["xy"]
