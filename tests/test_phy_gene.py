"""CPU-only: the numpy definitions of the gene concordance factors (swiftortho_amd/phy.py family_ranges .. gene_concordance, gcf_table,
tree(concordance=True)) against literal restatements and against the closed form of tests/phy_gene_inputs.py, whose guarantees -- how
many families each input drops -- are asserted here; then the labels, scripts/rbh2phy.py -K / -k and every exit code, and a table of
single deviations from the definition, each caught by a named input."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import phy_boot_inputs as bin_
import phy_gene_inputs as gin
import phy_inputs as pin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def phy():
    from swiftortho_amd import phy
    return phy


def host(phy, case, model="p"):
    return phy.gene_concordance(case, model, want_splits=True)


# ---------------------------------------------------------------------------------------------------------
# counts, presence, distances
# ---------------------------------------------------------------------------------------------------------
def test_family_ranges_and_counts_equal_the_triple_loop(phy):
    case = gin.width_case(9)
    r = phy.family_ranges(case.keep, case.col_off)
    assert r.dtype == np.int64 and np.diff(r).tolist() == list(gin.WIDTHS) and r[0] == 0 and r[-1] == len(case.keep)
    cmp_, same = phy.family_counts(case.matrix, case.keep, case.col_off)
    assert cmp_.dtype == same.dtype == np.int64 and cmp_.shape == (len(gin.WIDTHS), 9, 9)
    for f in range(len(gin.WIDTHS)):
        cols = [c for c in case.keep.tolist() if case.col_off[f] <= c < case.col_off[f + 1]]
        for a in range(9):
            for b in range(9):
                c = s = 0
                for k in cols:
                    x, y = case.matrix[a, k], case.matrix[b, k]
                    if x != 45 and y != 45:
                        c, s = c + 1, s + (x == y)
                assert (cmp_[f, a, b], same[f, a, b]) == (c, s)
    whole = phy.pair_counts(case.matrix, case.keep)
    assert (cmp_.sum(0) == whole[0]).all() and (same.sum(0) == whole[1]).all()


def test_presence_is_taken_from_the_kept_columns(phy):
    case = gin.width_case(9)
    cmp_, _ = phy.family_counts(case.matrix, case.keep, case.col_off)
    pres = phy.family_present(cmp_)
    assert pres.dtype == np.uint64 and pres.shape == (len(gin.WIDTHS), 1)
    assert pres[gin.WIDTHS.index(0), 0] == 0                                   # its one column is not kept
    assert pres[gin.WIDTHS.index(1), 0] == (1 << 4) - 1                        # taxa 0 .. 3 of nine hold the one kept column
    for f in range(len(gin.WIDTHS)):
        want = sum(1 << t for t in range(9) if (case.matrix[t, case.keep[(case.keep >= case.col_off[f]) & (case.keep < case.col_off[f + 1])]] != 45).any())
        assert int(pres[f, 0]) == want
    wide = np.zeros((130, 130), dtype=np.int64)
    wide[[0, 63, 64, 129], [0, 63, 64, 129]] = 1
    assert phy.family_present(wide).tolist() == [1 | 1 << 63, 1, 2]


def test_gene_distances_are_boot_distances_among_the_present(phy):
    case, fams = gin.hand_case()
    cmp_, same = phy.family_counts(case.matrix, case.keep, case.col_off)
    pres = phy.family_present(cmp_)
    for f, name in enumerate(case.names):
        idx = sorted(fams[f][0])
        for model in phy.GENE_MODELS:
            D, ok = phy.gene_distances(cmp_[f], same[f], pres[f], model)
            want, wok = phy.boot_distances(cmp_[f][np.ix_(idx, idx)], same[f][np.ix_(idx, idx)], model)
            assert ok == bool(wok) == (name != "disjoint"), (name, model)
            assert D.shape == (8, 8) and (D[np.ix_(idx, idx)] == want)[np.isfinite(want)].all()
    with pytest.raises(ValueError):
        phy.gene_distances(cmp_[0], same[0], pres[0], "logdet")


# ---------------------------------------------------------------------------------------------------------
# the walk over a subset
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,present", [(9, [1, 2, 4, 5, 7, 8]), (9, [0, 3, 4, 6]), (9, [2, 5, 6]), (70, [1, 5, 9, 63, 64, 65, 69]), (130, list(range(3, 130, 2)))])
def test_nj_splits_subset_equals_the_compacted_walk(phy, T, present):
    D = bin_.random_symmetric(T, seed=T)
    words = np.zeros((T + 63) // 64, dtype=np.uint64)
    for t in present:
        words[t >> 6] |= np.uint64(1 << (t & 63))
    got = phy.nj_splits_subset(D, words)
    assert got.dtype == np.uint64 and got.shape == (T - 3, (T + 63) // 64)
    n = len(present)
    want = [[0] * ((T + 63) // 64) for _ in range(T - 3)]
    if n >= 4:
        small = phy.nj_splits(D[np.ix_(present, present)])
        for k in range(n - 3):
            for pos in range(n):                         # bit `pos` of the compacted walk is taxon present[pos]
                if (int(small[k][pos >> 6]) >> (pos & 63)) & 1:
                    want[k][present[pos] >> 6] |= 1 << (present[pos] & 63)
    assert got.tolist() == want
    for k in range(max(n - 3, 0)):
        assert min(present) not in gin.words_sets(got[k:k + 1], T)[0] and gin.words_sets(got[k:k + 1], T)[0] < set(present)


@pytest.mark.parametrize("T", (4, 5, 64, 65))
def test_nj_splits_subset_with_every_taxon_is_nj_splits(phy, T):
    D = bin_.random_symmetric(T, seed=3)
    full = np.zeros((T + 63) // 64, dtype=np.uint64)
    for t in range(T):
        full[t >> 6] |= np.uint64(1 << (t & 63))
    assert (phy.nj_splits_subset(D, full) == phy.nj_splits(D)).all()


# ---------------------------------------------------------------------------------------------------------
# concordance: the closed form, the literal loop
# ---------------------------------------------------------------------------------------------------------
def literal_concordance(ref, present, gene, ok, T):
    """the definition family by family, in Python integers"""
    as_int = lambda row: sum(int(v) << (64 * w) for w, v in enumerate(row))
    dec, con = [0] * len(ref), [0] * len(ref)
    for f in range(len(present)):
        if not ok[f]:
            continue
        P = as_int(present[f])
        trees = {as_int(r) for r in gene[f]}
        for s in range(len(ref)):
            C = as_int(ref[s])
            A, B = C & P, P & ~C
            if bin(A).count("1") >= 2 and bin(B).count("1") >= 2:
                dec[s] += 1
                low = P & -P
                con[s] += (B if A & low else A) in trees
    return dec, con


def test_hand_table_closed_form(phy):
    case, fams = gin.hand_case()
    dec, con, ok, npres, splits = host(phy, case)
    assert dec.dtype == con.dtype == np.int32 and ok.dtype == bool and npres.dtype == np.int32
    assert dict(zip(case.names, ok.tolist())) == {n: n != "disjoint" for n in case.names} and int((~ok).sum()) == case.dropped == 1
    assert npres.tolist() == [len(p) for p, _, _ in fams]
    ref = phy.tree_splits(phy.distances(case.cmp, case.same))
    sides = gin.words_sets(ref, 8)
    assert set(sides) == {gin.canonical(s, range(8)) for s in gin.caterpillar(list(range(8)))}, "the printed tree is tree A"
    want = gin.expected_concordance(sides, fams)
    assert (dec.tolist(), con.tolist()) == want
    for f, (present, planted, dropped) in enumerate(fams):      # every family's tree is its planted tree, in the canonical form
        n = len(present)
        held = gin.words_sets(splits[f], 8)
        assert set(held[:max(n - 3, 0)]) == ({gin.canonical(s, present) for s in planted} if not dropped else {frozenset()})
        assert all(not s for s in held[max(n - 3, 0):])
    by = {frozenset(s): k for k, s in enumerate(sides)}
    k01 = by[gin.canonical({0, 1}, range(8))]
    # {0, 1}: A_all, A_all2, B_all and B_no_2 decide it (no_taxon0 and no_1 see a single taxon on that side, three has three taxa);
    # B_all holds {0, 2} instead, B_no_2 holds it again
    assert (dec[k01], con[k01]) == (4, 3)
    k = by[gin.canonical({0, 1, 2, 3, 4}, range(8))]
    assert (dec[k], con[k]) == (6, 6)                           # everyone but three, empty and the dropped family
    assert (dec.tolist(), con.tolist()) == literal_concordance(ref, phy.family_present(phy.family_counts(case.matrix, case.keep, case.col_off)[0]), splits, ok, 8)


@pytest.mark.parametrize("T", gin.GPU_TAXA)
def test_edge_cases_closed_form_and_drops(phy, T):
    case, fams = gin.edge_case(T)
    dec, con, ok, npres, splits = host(phy, case)
    assert int((~ok).sum()) == case.dropped == 1 and not ok[case.names.index("dropped")]
    assert npres.tolist() == [len(p) for p, _, _ in fams] and npres[case.names.index("three")] == 3 and npres[case.names.index("four")] == 4
    ref = phy.tree_splits(phy.distances(case.cmp, case.same))
    assert (dec.tolist(), con.tolist()) == gin.expected_concordance(gin.words_sets(ref, T), fams)
    if T <= 65:
        cmp_, _ = phy.family_counts(case.matrix, case.keep, case.col_off)
        assert (dec.tolist(), con.tolist()) == literal_concordance(ref, phy.family_present(cmp_), splits, ok, T)
    if T >= 5:
        assert (con < dec).sum() == 1                           # tree B misses one split of A


def test_the_other_inputs_drop_nothing(phy):
    for case in (gin.width_case(), gin.batch_case(1), gin.batch_case(gin.FORCED_BATCH), gin.batch_case(gin.FORCED_BATCH + 1)):
        ok = host(phy, case)[2]
        assert ok.all() and case.dropped == 0
    for T in gin.WIDE_TAXA:                                      # (without their walks: what drops a family is its distances)
        case = gin.wide_case(T)
        cmp_, same = phy.family_counts(case.matrix, case.keep, case.col_off)
        pres = phy.family_present(cmp_)
        assert all(phy.gene_distances(cmp_[f], same[f], pres[f])[1] for f in range(len(pres))) and case.dropped == 0
        assert phy._popcount(pres).tolist() == [T, 200, 70]


def test_poisson_and_kimura_decide_the_same_here(phy):
    case, _ = gin.hand_case()
    want = host(phy, case)
    for model in ("poisson", "kimura"):
        got = host(phy, case, model)
        assert got[2].tolist() == want[2].tolist() and got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist()
    with pytest.raises(phy.ConcordanceRefused):
        phy.gene_concordance(case, "logdet")


# ---------------------------------------------------------------------------------------------------------
# single deviations, each caught by a named input
# ---------------------------------------------------------------------------------------------------------
def raw_walk(D, idx):
    """neighbour joining over the taxa idx in Python floats, row sums left to right -> the clade (a set of taxa) every join makes, as
    made: no canonical form yet"""
    D = [[float(D[a][b]) for b in idx] for a in idx]
    clades, out = [{t} for t in idx], []
    while len(D) > 3:
        n = len(D)
        r = []
        for a in range(n):
            s = 0.
            for b in range(n):
                s = s + D[a][b]
            r.append(s)
        best = None
        for a in range(n):
            for b in range(a + 1, n):
                q = ((n - 2) * D[a][b] - r[a]) - r[b]
                if best is None or q < best[0]:
                    best = (q, a, b)
        _, i, j = best
        dij = D[i][j]
        new = [((D[i][k] + D[j][k]) - dij) / 2. for k in range(n)]
        for k in range(n):
            D[i][k] = D[k][i] = new[k]
        D[i][i] = 0.
        del D[j]
        for row in D:
            del row[j]
        clades[i] = clades[i] | clades[j]
        del clades[j]
        out.append(frozenset(clades[i]))
    return out


def literal_gene(case, ref_sides, deviation=None):
    """the whole definition in Python sets and floats, family by family, with at most ONE deviation -> (decisive, concordant)"""
    T = len(case.taxa)
    dec, con = [0] * len(ref_sides), [0] * len(ref_sides)
    for f in range(len(case.col_off) - 1):
        block = range(int(case.col_off[f]), int(case.col_off[f + 1]))
        cols = [c for c in case.keep.tolist() if c in block]
        seen = list(block) if deviation == "presence_from_all_columns" else cols
        present = [t for t in range(T) if any(case.matrix[t, c] != 45 for c in seen)]
        D, dropped = {}, False
        for a in present:
            D[a] = {}
            for b in present:
                shared = [c for c in cols if case.matrix[a, c] != 45 and case.matrix[b, c] != 45]
                dropped = dropped or not shared
                D[a][b] = 1. - sum(1 for c in shared if case.matrix[a, c] == case.matrix[b, c]) / float(len(shared)) if shared else 0.
        if dropped and deviation != "dropped_counted":
            continue
        held = set()
        if not dropped and len(present) >= 4:
            for clade in raw_walk(D, present):
                if deviation == "complement_by_taxon_0":
                    held.add(frozenset(present) - clade if 0 in clade else clade)
                else:
                    held.add(frozenset(present) - clade if min(present) in clade else clade)
        need = 1 if deviation == "one_for_two" else 2
        for k, side in enumerate(ref_sides):
            a, b = frozenset(side) & frozenset(present), frozenset(present) - frozenset(side)
            if len(a) >= need and len(b) >= need:
                dec[k] += 1
                con[k] += (b if min(present) in a else a) in held
    return dec, con


DEVIATIONS = (("complement_by_taxon_0", "hand", "no_taxon0: its first join holds taxon 1, the lowest it has"),
              ("one_for_two", "hand", "no_1: the split {0, 1} leaves it taxon 0 alone on one side"),
              ("dropped_counted", "hand", "disjoint: it would decide the splits among taxa 3 .. 7"),
              ("presence_from_all_columns", "ghost", "ghost: a column that is not kept holds the only residue of taxon 5"))


def test_deviation_table(phy):
    cases = {"hand": gin.hand_case()[0], "ghost": gin.ghost_case()}
    good = {}
    for key, case in cases.items():
        dec, con, ok, _, _ = host(phy, case)
        sides = gin.words_sets(phy.tree_splits(phy.distances(case.cmp, case.same)), len(case.taxa))
        good[key] = (dec.tolist(), con.tolist())
        assert literal_gene(case, sides) == good[key], key
        assert int((~ok).sum()) == case.dropped
        for deviation, caught_by, why in DEVIATIONS:
            assert (literal_gene(case, sides, deviation) != good[key]) == (caught_by == key), (deviation, key, why)


# ---------------------------------------------------------------------------------------------------------
# labels and the table
# ---------------------------------------------------------------------------------------------------------
def test_labels_gcf_boot_and_na(phy):
    case, _ = gin.hand_case()
    bare = phy.tree(case)
    assert phy.tree(case, concordance=False) == bare and not re.search(rb"\)[0-9NA./]+:", bare)
    stats = {}
    lab = phy.tree(case, concordance=True, stats=stats)
    dec, con = stats["gcf"]["decisive"], stats["gcf"]["concordant"]
    found = re.findall(rb"\)([0-9NA.]+):", lab)
    assert sorted(found) == sorted(b"%.3f" % (c / float(d)) for d, c in zip(dec.tolist(), con.tolist())) and re.sub(rb"\)[0-9NA.]+:", b"):", lab) == bare
    assert b"0.750" in found
    both = phy.tree(case, boot=5, concordance=True)
    pairs = re.findall(rb"\)([01]\.[0-9]{3})/([0-9NA.]+):", both)
    assert len(pairs) == 5 and [g for _, g in pairs] == found and re.sub(rb"\)[01]\.[0-9]{3}/[0-9NA.]+:", b"):", both) == bare
    assert [b for b, _ in pairs] == re.findall(rb"\)([01]\.[0-9]{3}):", phy.tree(case, boot=5))
    assert phy.gcf_labels([0, 4, 3], [0, 3, 3]) == ["NA", "0.750", "1.000"]
    D = phy.distances(case.cmp, case.same)
    assert phy.neighbor_joining(D, case.taxa) == bare
    assert b")x1:" in phy.neighbor_joining(D, case.taxa, labels=["x%d" % k for k in range(5)])
    for bad in (dict(labels=["a"]), dict(labels=["a"] * 5, support=[1.] * 5)):
        with pytest.raises(ValueError):
            phy.neighbor_joining(D, case.taxa, **bad)
    # branches nobody decides
    T = 6
    only = gin.Case(T, [gin.planted_block(T, list(range(T)))])
    only.keep = only.keep[:0]                                 # nothing kept for the families: every taxon absent, nobody decides
    dec, con, ok, npres, _ = phy.gene_concordance(only)
    assert dec.tolist() == [0] * 3 and ok.all() and npres.tolist() == [0]
    assert phy.gcf_labels(dec, con) == ["NA"] * 3
    table = phy.gcf_table(only.taxa, phy.tree_splits(phy.distances(only.cmp, only.same)), dec, con).decode().splitlines()
    assert table[0].split("\t") == ["join", "taxa_in_clade", "decisive", "concordant", "gcf", "taxa"] and all(l.split("\t")[4] == "NA" for l in table[1:])


def test_gcf_table(phy):
    case, _ = gin.hand_case()
    dec, con = host(phy, case)[:2]
    ref = phy.tree_splits(phy.distances(case.cmp, case.same))
    lines = phy.gcf_table(case.taxa, ref, dec, con).decode().splitlines()
    assert len(lines) == 6
    for k, line in enumerate(lines[1:]):
        f = line.split("\t")
        inside = sorted(gin.words_sets(ref[k:k + 1], 8)[0])
        assert f[:4] == [str(k), str(len(inside)), str(dec[k]), str(con[k])] and f[4] == repr(int(con[k]) / float(dec[k])) and f[5] == ",".join("t%d" % t for t in inside)


# ---------------------------------------------------------------------------------------------------------
# scripts/rbh2phy.py -K, -k
# ---------------------------------------------------------------------------------------------------------
def run_script(tmp_path, extra=(), kind="plain"):
    fasta, sc = gin.script_case(kind)
    p, f = str(tmp_path / ("%s.sc" % kind)), str(tmp_path / ("%s.fsa" % kind))
    open(p, "wb").write(sc), open(f, "wb").write(fasta)
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "rbh2phy.py"), "-i", p, "-f", f, "-A", "T"] + list(extra), capture_output=True)


def test_script_files(tmp_path):
    tree, tsv = str(tmp_path / "x.nwk"), str(tmp_path / "x.tsv")
    bare = run_script(tmp_path, ("-t", tree))
    assert bare.returncode == 0, bare.stderr
    today = open(tree, "rb").read()
    assert b"4 core families" in bare.stderr
    for flags in (("-K", "F"), ("-KF",)):
        r = run_script(tmp_path, ("-t", tree) + flags)
        assert r.returncode == 0 and r.stdout == bare.stdout and r.stderr == bare.stderr and open(tree, "rb").read() == today and not os.path.exists(tsv)
    r = run_script(tmp_path, ("-t", tree, "-K", "T", "-k", tsv))
    assert r.returncode == 0, r.stderr
    lab = open(tree, "rb").read()
    labels = re.findall(rb"\)([0-9NA.]+):", lab)
    assert r.stdout == bare.stdout and len(labels) == 7 and re.sub(rb"\)[0-9NA.]+:", b"):", lab) == today
    rows = [l.split("\t") for l in open(tsv).read().splitlines()]
    assert rows[0] == ["join", "taxa_in_clade", "decisive", "concordant", "gcf", "taxa"] and [r_[0] for r_ in rows[1:]] == [str(k) for k in range(7)]
    assert sorted(labels) == sorted(b"NA" if int(r_[2]) == 0 else b"%.3f" % (int(r_[3]) / float(r_[2])) for r_ in rows[1:])      # (the text nests the joins)
    for row in rows[1:]:
        d, c = int(row[2]), int(row[3])
        assert 0 <= c <= d <= 4 and row[4] == ("NA" if d == 0 else repr(c / float(d)))
        assert len(row[5].split(",")) == int(row[1]) and "A" not in row[5].split(",")
        # a branch that sets {J, x} or {B, x} apart is not decided by the family that lacks J or B
        assert d == 4 - sum(1 for miss in ("J", "B") if len(set(row[5].split(",")) - {miss}) < 2 or len(set("ABCDEFGHIJ") - set(row[5].split(",")) - {miss}) < 2)
    os.remove(tsv)
    r = run_script(tmp_path, ("-t", tree, "-K", "T", "-B", "6", "-m", "kimura"))
    assert r.returncode == 0 and len(re.findall(rb"\)[01]\.[0-9]{3}/[0-9NA.]+:", open(tree, "rb").read())) == 7 and not os.path.exists(tsv)


def test_script_exit_codes(tmp_path):
    tree, tsv = str(tmp_path / "x.nwk"), str(tmp_path / "x.tsv")
    for flags, kind, word in ((("-K", "T"), "plain", b"-K"), (("-K", "T", "-k", tsv), "plain", b"-K"), (("-t", tree, "-k", tsv), "plain", b"-k"),
                              (("-t", tree, "-K", "T", "-m", "logdet"), "plain", b"logdet"), (("-t", tree, "-K", "T", "-k", tsv), "all_dropped", b"none of the 2 families")):
        r = run_script(tmp_path, flags, kind)
        assert r.returncode == 2 and r.stdout == b"" and r.stderr.startswith(b"rbh2phy: ") and word in r.stderr and r.stderr.count(b"\n") == 1, (flags, r.stderr)
        assert not os.path.exists(tree) and not os.path.exists(tsv)
    r = run_script(tmp_path, ("-t", tree), "all_dropped")
    assert r.returncode == 0 and os.path.exists(tree)                  # the supermatrix as a whole has a tree: only the families have none
