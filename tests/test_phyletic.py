"""Phyletic profiles without a GPU: the numpy definition swiftortho_amd/phyletic.py `linked_pairs()` against a literal double loop over
Python sets, the promise of every designed input of tests/phyletic_inputs.py (what the GPU tests rely on), the hand tables for the
threshold, k_min, a member listed twice, the file-row bound and the bounds on the taxa of a family, the hypergeometric tail against exact
fractions, scripts/phyletic_links.py under -G F, and three single deviations of the definition, each caught by a named input."""
import fractions
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import pan_content_inputs as ci
import phyletic_inputs as pi
from conftest import ROOT

SCRIPT = os.path.join(ROOT, "scripts", "phyletic_links.py")


@pytest.fixture(scope="module")
def ph():
    from swiftortho_amd import phyletic
    return phyletic


def random_table(seed, R, T, density):
    bits = np.random.RandomState(seed).rand(R, T) < density
    return pi.table_of_bits(bits, R - R // 5)


def test_linked_pairs_against_the_double_loop(ph):
    for seed, (R, T, density) in enumerate([(40, 9, .5), (70, 5, .6), (33, 70, .3), (90, 3, .7), (12, 1, .8), (1, 4, .5), (0, 4, .5)]):
        tb = random_table(seed, R, T, density)
        for args in ((1, T, 1, 1, 2), (2, max(T - 1, 1), 2, 2, 3), (1, T, 1, 1, 1), (3, 2, 1, 1, 2)):
            L = ph.linked_pairs(tb, T, *args)
            assert pi.as_lists(L) == pi.loop_links(tb, T, *args)
            assert L.a.dtype == L.b.dtype == L.shared.dtype == L.present.dtype == np.int32 and len(L.present) == R
            assert L.present.tolist() == ph.profile_bits(tb, T).sum(1).tolist()
    assert len(ph.linked_pairs(random_table(1, 70, 5, .6), 5, 1, 5, 1, 1, 2).a) > 50         # (the comparison is not of empty lists)


def test_designed_inputs_keep_their_promises(ph):
    pi.module_facts(ph)
    pi.dense_facts(ph)
    pi.width_facts(ph)
    pi.strided_facts(ph)
    for E in pi.SHAPE_E:
        for T in pi.SHAPE_T:
            L = pi.shaped_facts(ph, E, T)
            if E <= 65:
                assert pi.as_lists(L) == pi.loop_links(pi.shaped(E, T).table, T, *pi.shaped(E, T).args)
    tb, T, args = pi.larger()
    L = ph.linked_pairs(tb, T, *args)
    assert 1900 <= L.n_eligible <= 2050 and len(L.a) > 10000 and ((L.a % 150) == (L.b % 150)).all()
    assert pi.tune_define("PP_CHUNK") in (8, 16, 32)          # the chunk-edge cases of the GPU test stay below 4096 taxa


def test_threshold_by_hand(ph):
    tb, T = pi.hand_threshold()
    for k_min, want in pi.HAND_THRESHOLD_LINKS.items():
        assert pi.as_lists(ph.linked_pairs(tb, T, 1, T, k_min, 3, 4)) == want == pi.loop_links(tb, T, 1, T, k_min, 3, 4)
    L = ph.linked_pairs(tb, T, 1, T, 2, 3, 4)
    assert L.present.tolist() == [3, 4, 4, 3]                 # row 3: every member listed twice, counted once
    assert ph.jaccard(L.present, L.a, L.b, L.shared).tolist() == [.75, 1., .75]
    assert pi.as_lists(ph.linked_pairs(tb, T, 1, T, 2, 3001, 4000)) == ([0], [3], [3])      # just above 3/4: the equality is gone
    tb, T, args = pi.hand_bounds()
    assert pi.as_lists(ph.linked_pairs(tb, T, *args)) == pi.HAND_BOUNDS_LINKS == pi.loop_links(tb, T, *args)
    assert pi.as_lists(ph.linked_pairs(tb, T, 1, 5, *args[2:])) == ([0, 1, 2], [1, 2, 3], [1, 2, 4])      # what the bounds keep out
    tb.n_file_rows = 5
    assert pi.as_lists(ph.linked_pairs(tb, T, *args)) == ([1, 1, 2], [2, 4, 4], [2, 2, 2])                # what the file-row bound keeps out
    for bad in ((0, 4, 1, 1, 2), (2, 4, 0, 1, 2), (2, 4, 1, 0, 2), (2, 4, 1, 3, 2), (2, 4, 1, 1, 1 << 20)):
        with pytest.raises(ValueError):
            ph.linked_pairs(tb, T, *bad)


@pytest.mark.parametrize("deviate", pi.DEVIATIONS)
def test_single_deviations_are_caught(ph, deviate):
    """each single change of the literal model parts from the definition on a named input (and the model without a change does not)"""
    hand, T = pi.hand_threshold()
    s = pi.shaped(65, 64)
    named = {"> for >=": (hand, T, 1, T, 2, 3, 4), "u without - k": (hand, T, 1, T, 2, 3, 4), "compacted rows": (s.table, s.T) + s.args}[deviate]
    want = pi.as_lists(ph.linked_pairs(*named))
    assert pi.loop_links(*named) == want and pi.loop_links(*named, deviate=deviate) != want


def exact_tail(T, na, nb, k):
    total = sum(fractions.Fraction(math.comb(na, i) * math.comb(T - na, nb - i)) for i in range(max(k, 0), min(na, nb) + 1) if nb - i <= T - na)
    return total / math.comb(T, nb)


def test_enrichment(ph):
    for T in (1, 2, 7, 40):
        for na in range(T + 1):
            for nb in range(T + 1):
                last = 1.
                for k in range(0, min(na, nb) + 2):
                    got, want = ph.enrichment(T, na, nb, k), exact_tail(T, na, nb, k)
                    assert abs(got - float(want)) <= 1e-9 * float(want), (T, na, nb, k)
                    assert got <= last and got == ph.enrichment(T, nb, na, k)
                    last = got
                assert ph.enrichment(T, na, nb, 0) == 1. and last == 0.
    # the same Jaccard of 1 means less between two families of 2 genomes than between two of 250
    assert ph.enrichment(500, 250, 250, 250) < 1e-100 < 1e-6 < ph.enrichment(500, 2, 2, 2) < 1e-5
    with pytest.raises(ValueError):
        ph.enrichment(5, 6, 1, 1)


def test_jaccard_fraction(ph):
    assert ph.jaccard_fraction("0.8") == ph.jaccard_fraction("4/5") == ph.jaccard_fraction(" 8/10 ") == (4, 5) and ph.jaccard_fraction("1") == (1, 1)
    assert ph.jaccard_fraction("1/1048575") == (1, 1048575)
    for bad in ("0", "-0.5", "1.01", "5/4", "x", "", "1/0", "1/1048576", "0.3333333", "nan"):
        with pytest.raises(ph.BadThreshold):
            ph.jaccard_fraction(bad)


# ---------------------------------------------------------------------------------------------------------
# the script (-G F)
# ---------------------------------------------------------------------------------------------------------
def script_files(d):
    """36 families in 4 modules x 12 genomes as files, then rows 36 .. 39: single genes no group line lists"""
    os.makedirs(str(d), exist_ok=True)
    bits = pi.module_bits(36, 12, 4, seed=2).astype(np.int32)
    counts = np.concatenate([bits, np.eye(12, dtype=np.int32)[:4]])
    counts[::5] *= 2                                          # members listed twice
    fasta, groups = ci.files_of(counts, ci.names_of(12), 36)
    fa, gr = str(d / "in.fsa"), str(d / "in.clsr")
    open(fa, "w").write(fasta), open(gr, "w").write(groups)
    return fa, gr, counts


def run_script(d, fa, gr, extra):
    x = str(d / "out.xyz")
    r = subprocess.run([sys.executable, SCRIPT, "-i", fa, "-g", gr, "-x", x] + list(extra), capture_output=True, cwd=str(d))
    return r, (open(x, "rb").read() if os.path.isfile(x) else None)


def test_script_G_F(ph, tmp_path):
    fa, gr, counts = script_files(tmp_path)
    r, xyz = run_script(tmp_path / "a", *script_files(tmp_path / "a")[:2], ("-j", "0.8", "-l", "1", "-u", "12"))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.decode().split("\n")
    assert lines[0] == "#family_a\tfamily_b\ttaxa_a\ttaxa_b\tshared\tjaccard\tp" == ph.HEADER and lines[-1] == "" and len(lines) > 10
    # the same pairs from the table itself: Share at -l 1 -u 12 is 2 .. 11 genomes
    from swiftortho_amd import pan
    tb = ci.table_of(pan, counts)
    tb.n_file_rows = 36
    L = ph.linked_pairs(tb, 12, 2, 11, 2, 4, 5)
    assert len(L.a) == len(lines) - 2 > 0
    rows = [l.split("\t") for l in lines[1:-1]]
    assert [(int(c[0][6:]), int(c[1][6:]), int(c[4])) for c in rows] == list(zip(*pi.as_lists(L)))
    assert all(c[0].startswith("group_") and len(c[0]) == 15 and len(c) == 7 for c in rows)
    for c in rows:
        k, na, nb = int(c[4]), int(c[2]), int(c[3])
        assert c[5] == repr(k / (na + nb - k)) and c[6] == repr(ph.enrichment(12, na, nb, k))
    assert xyz.decode() == "".join("%s\t%s\t%s\n" % (c[0], c[1], c[5]) for c in rows)
    # -j 4/5 and glued flags: the same bytes
    r2, xyz2 = run_script(tmp_path / "b", *script_files(tmp_path / "b")[:2], ("-j4/5", "-l1", "-u12", "-GF"))
    assert r2.returncode == 0 and r2.stdout == r.stdout and xyz2 == xyz
    # every refusal: exit code 2, one line on stderr, nothing written
    for n, bad in enumerate((("-j", "0"), ("-j", "1.5"), ("-j", "abc"), ("-j", "1/1048576"), ("-k", "0"), ("-k", "1.5"), ("-k", "-2"), ("-k", "two"))):
        d = tmp_path / ("r%d" % n)
        rb, xb = run_script(d, *script_files(d)[:2], bad)
        assert rb.returncode == 2 and rb.stdout == b"" and xb is None and rb.stderr.count(b"\n") == 1 and rb.stderr.startswith(b"phyletic_links: "), (bad, rb.stderr)
