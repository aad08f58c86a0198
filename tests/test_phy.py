"""The numpy definitions of the supermatrix stage (swiftortho_amd/phy.py) against independent restatements: project() against
fsearch.cigar_to_strings, pick_rows() and pair_counts() against literal Python loops, neighbor_joining() against the random additive trees
it must recover, every refusal, and scripts/rbh2phy.py with and without -A.  No GPU is needed (the library, where a test formats a
CIGAR, is only asked for host functions)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import phy_inputs as pin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def phy():
    from swiftortho_amd import phy
    return phy


def strings_of(runs, q, s, qst, sst):
    """fsearch.cigar_to_strings without the library: the same walk over (length, op) runs -- used when libsohit.so is not built"""
    from swiftortho_amd import fsearch
    packed = [(n << 4) | op for n, op in runs]
    return fsearch.cigar_to_strings(packed, q, s, qst, sst)


def check_projection(phy, alen, q, s, qst, sst, runs):
    row = phy.project(alen, s, qst, sst, phy.pack_runs(runs))
    a0, a1 = strings_of(runs, q, s, qst, sst)
    placed = bytes(y for x, y in zip(a0, a1) if x != 45)          # the subject string where the query string is no '-'
    qed = qst - 1 + len(placed)
    assert len(row) == alen and row[qst - 1:qed] == placed
    assert row[:qst - 1] == b"-" * (qst - 1) and row[qed:] == b"-" * (alen - qed)
    assert sum(c != 45 for c in row) == sum(n for n, op in runs if op == 0)


def test_project_designed(phy):
    rng = np.random.RandomState(2)
    q = pin.residues(rng, 40)
    s = pin.residues(rng, 30)
    for qst, sst, runs in ((1, 1, [(30, 0)]), (11, 1, [(30, 0)]),                    # a path touching both ends of the subject / the query end
                           (1, 1, [(2, 1), (3, 2), (10, 0), (4, 2), (5, 1)]),          # leading and trailing I and D
                           (40, 30, [(1, 0)]), (40, 1, [(1, 0)]), (1, 30, [(1, 0)]),   # starts at the last residue, M of length 1
                           (1, 1, [(40, 1)]), (1, 1, [(30, 2)]), (5, 5, []),           # nothing copied
                           (3, 2, [(1, 0), (1, 1), (1, 0), (1, 2), (1, 0), (1, 0)]),   # runs of length 1, a repeated op
                           (1, 1, [(20, 0), (20, 1)]), (1, 1, [(10, 0), (20, 2)])):
        check_projection(phy, 40, q, s, qst, sst, runs)


def test_project_random(phy):
    rng = np.random.RandomState(9)
    for _ in range(300):
        alen = int(rng.randint(1, 90))
        runs = pin.random_runs(rng, int(rng.randint(0, 12)), alen)
        qs, ss = pin.spans(runs)
        qst, sst = int(rng.randint(1, alen - qs + 2)), int(rng.randint(1, 5))
        check_projection(phy, alen, pin.residues(rng, alen), pin.residues(rng, sst - 1 + ss + int(rng.randint(0, 3))), qst, sst, runs)


def test_project_refusals(phy):
    s = b"ACDEFGHIKL"
    for qst, sst, runs, word in ((0, 1, [(3, 0)], "before the first"), (1, 0, [(3, 0)], "before the first"), (1, 1, [(11, 0)], "past the anchor"),
                                 (9, 1, [(2, 0), (1, 1)], "past the anchor"), (1, 9, [(3, 0)], "past the member"), (1, 1, [(8, 0), (3, 2)], "past the member"),
                                 (1, 1, [(2, 0), (0, 1)], "length 0"), (1, 1, [(2, 3)], "unknown operation")):
        with pytest.raises(ValueError) as e:
            phy.project(10, s, qst, sst, np.asarray([(n << 4) | op for n, op in runs], dtype=np.uint32), what="row 7")
        assert word in str(e.value) and "row 7" in str(e.value)


@pytest.mark.parametrize("case", pin.row_cases(), ids=lambda c: c[0])
def test_pick_rows(phy, case):
    _, q, s, sco, pq, ps = case
    got = phy.pick_rows(q, s, sco, pq, ps)
    assert got.dtype == np.int64 and got.tolist() == pin.literal_pick(q.tolist(), s.tolist(), sco.tolist(), pq.tolist(), ps.tolist())


def test_pick_rows_expected(phy):
    """the designed answers themselves (the literal loop is held to them too)"""
    want = {"zero_signs_a": [0], "zero_signs_b": [0], "zero_signs_c": [1], "last_bit_up": [1], "last_bit_negative": [1], "tiny_and_huge": [2],
            "ungrouped": [2, 4, 3, -1], "best_in_last_row": [299]}
    cases = {c[0]: c for c in pin.row_cases()}
    for k, w in want.items():
        assert phy.pick_rows(*cases[k][1:]).tolist() == w, k
    assert phy.pick_rows(*cases["ties_first_last_row"][1:]).tolist()[0] == 0
    with pytest.raises(ValueError) as e:
        phy.pick_rows([0, 0], [1, 1], [1., float("nan")], [0], [1])
    assert "NaN" in str(e.value)


def test_pair_counts(phy):
    for T, L in ((1, 5), (2, 1), (3, 4), (5, 131), (17, 60)):
        m = pin.pair_matrix(T, L)
        for keep in (np.arange(L), np.arange(0, L, 3), np.zeros(0, dtype=np.int64)):
            cmp_, same = phy.pair_counts(m, keep)
            wc, ws = pin.literal_pair_counts(m, keep)
            assert cmp_.dtype == np.int64 and cmp_.tolist() == wc.tolist() and same.tolist() == ws.tolist()
            assert (cmp_ == cmp_.T).all() and (same == same.T).all()
    for _, m in pin.byte_cases():
        cmp_, same = phy.pair_counts(m, np.arange(m.shape[1]))
        assert same[0, 1] == m.shape[1] - 1 and same[0, 2] == m.shape[1] and (cmp_ == m.shape[1]).all()


@pytest.mark.parametrize("case", pin.gap_cases(), ids=lambda c: c[0])
def test_gaps_and_keep(phy, case):
    _, m, g = case
    T, L = m.shape
    gaps = phy.column_gaps(m)
    assert gaps.dtype == np.int32 and gaps.tolist() == [sum(1 for t in range(T) if m[t, c] == 45) for c in range(L)]
    keep = phy.kept_columns(gaps, g, T)
    assert keep.tolist() == [c for c in range(L) if gaps[c] <= int(np.floor(g * T))]
    if case[0] == "T64_on_floor":
        assert keep[:2].tolist() == [0, 1] and 2 not in keep and 199 in keep
    if case[0] == "keep_nothing":
        assert len(keep) == 0
    if g == 1.:
        assert len(keep) == L


def test_build_equals_its_parts(phy):
    """build() on designed tasks: every block is project() of its task, blocks without a task are gaps"""
    for tk in (pin.projection_case(1), pin.boundary_case()):
        matrix, gaps, keep, cmp_, same = phy.build(tk, .5)
        want = np.full_like(matrix, 45)
        res = tk.residues.tobytes()
        for t in range(len(tk.fam)):
            c0, c1 = tk.col_off[tk.fam[t]], tk.col_off[tk.fam[t] + 1]
            seq = res[tk.res_off[t]:tk.res_off[t] + tk.res_len[t]]
            row = seq if tk.kind[t] else phy.project(c1 - c0, seq, tk.qst[t], tk.sst[t], tk.runs[tk.run_off[t]:tk.run_off[t + 1]])
            want[tk.slot[t], c0:c1] = np.frombuffer(row, dtype=np.uint8)
        assert (matrix == want).all() and gaps.tolist() == phy.column_gaps(want).tolist()
        wc, ws = phy.pair_counts(want, keep)
        assert cmp_.tolist() == wc.tolist() and same.tolist() == ws.tolist()
    m = pin.boundary_case()
    row = phy.build(m)[0][0]
    assert (row[:59] == 45).all() and (row[59:159] != 45).all() and (row[159:257] == 45).all()


@pytest.mark.parametrize("case", pin.bad_task_cases(), ids=lambda c: c[0])
def test_bad_task_refused(phy, case):
    _, tk, word = case
    with pytest.raises(ValueError) as e:
        phy.build(tk)
    assert word in str(e.value) and "family 1, slot 2" in str(e.value)


def test_build_refusals(phy):
    good = pin.projection_case(1)

    def changed(**kw):
        a = dict(n_taxa=good.n_taxa, col_off=good.col_off, fam=good.fam, slot=good.slot, kind=good.kind, res_off=good.res_off, res_len=good.res_len,
                 qst=good.qst, sst=good.sst, run_off=good.run_off, runs=good.runs, residues=good.residues)
        a.update(kw)
        return phy.Tasks(**a)

    none = np.zeros(0, dtype=np.int64)
    empty = dict(fam=none, slot=none, kind=none, res_off=none, res_len=none, qst=none, sst=none, run_off=[0], runs=none)
    off = good.run_off.copy()
    off[3] += 1000
    cases = ((changed(n_taxa=0, **empty), 1., "no taxa"), (changed(col_off=[0], **empty), 1., "no families"), (good, 1.5, "gap share"), (good, -.1, "gap share"),
             (good, float("nan"), "gap share"), (changed(col_off=[0, 5, 3], **empty), 1., "inconsistent offsets"), (changed(col_off=[1, 5], **empty), 1., "inconsistent offsets"),
             (changed(col_off=[0, 2 ** 31], **empty), 1., "2^31 - 1 columns"), (changed(run_off=off), 1., "inconsistent offsets"),
             (changed(res_off=good.res_off + len(good.residues)), 1., "inconsistent offsets"), (changed(slot=np.zeros_like(good.slot)), 1., "two tasks"),
             (changed(fam=good.fam + 100), 1., "out of range"))
    for tk, g, word in cases:
        with pytest.raises(ValueError) as e:
            phy.build(tk, g)
        assert word in str(e.value), (word, str(e.value))


# ---------------------------------------------------------------------------------------------------------
# distances and neighbour joining
# ---------------------------------------------------------------------------------------------------------
def test_distances(phy):
    cmp_ = np.array([[10, 8], [8, 9]])
    same = np.array([[10, 6], [6, 9]])
    p = phy.distances(cmp_, same)
    assert p.dtype == np.float64 and p.tolist() == [[0., 1. - 6. / 8.], [1. - 6. / 8., 0.]]
    d = phy.distances(cmp_, same, "poisson")
    assert d[0, 1] == -np.log(1. - (1. - 6. / 8.)) and d[0, 0] == 0.
    for c, s, model, words in (([[1, 0], [0, 1]], [[1, 0], [0, 1]], "p", ("tA", "tB", "no compared column")),
                               ([[3, 2], [2, 3]], [[3, 0], [0, 3]], "poisson", ("tA", "tB", "poisson"))):
        with pytest.raises(ValueError) as e:
            phy.distances(np.array(c), np.array(s), model, [b"tA", b"tB"])
        assert all(w in str(e.value) for w in words)
    with pytest.raises(ValueError):
        phy.distances(cmp_, same, "jc")


@pytest.mark.parametrize("T", [3, 4, 5, 8, 33])
def test_neighbor_joining_recovers_additive_trees(phy, T):
    rng = np.random.RandomState(40 + T)
    for _ in range(6):
        edges, D = pin.random_tree(rng, T)
        names = ["x%d" % k for k in range(T)]
        nwk = phy.neighbor_joining(D.astype(np.float64), names)
        got, want = pin.newick_splits(nwk, names), pin.tree_splits(edges, T)
        assert set(got) == set(want)                      # every bipartition, leaf edges included
        tol = 1e-9 * D.max()
        assert all(abs(got[k] - want[k]) <= tol for k in want)
        assert nwk.count(b"(") == T - 2 and nwk.endswith(b");")


def test_neighbor_joining_small_and_ties(phy):
    assert phy.neighbor_joining([[0, 3], [3, 0]], [b"A", b"B"]) == b"(A:1.500000,B:1.500000);"
    assert phy.neighbor_joining([[0, 2, 4], [2, 0, 4], [4, 4, 0]], ["a", "b", "c"]) == b"(a:1.000000,b:1.000000,c:3.000000);"
    for names, D in (([], np.zeros((0, 0))), (["a"], np.zeros((1, 1)))):
        with pytest.raises(ValueError):
            phy.neighbor_joining(D, names)
    # every Q equal: the lowest (i, j) = (0, 1) is joined, the node takes position 0
    D = 2. * (1 - np.eye(4))
    assert phy.neighbor_joining(D, list("abcd")) == b"((a:1.000000,b:1.000000):0.000000,c:1.000000,d:1.000000);"
    # two cherries with equal Q: (0, 2) comes before (1, 3)
    edges = {(0, 4): 1, (2, 4): 1, (1, 5): 1, (3, 5): 1, (4, 5): 2}
    D = np.array([[0, 4, 2, 4], [4, 0, 4, 2], [2, 4, 0, 4], [4, 2, 4, 0]], dtype=float)
    assert phy.neighbor_joining(D, list("abcd")) == b"((a:1.000000,c:1.000000):2.000000,b:1.000000,d:1.000000);"
    # a negative branch as it comes
    D = np.array([[0, 1, 5, 5], [1, 0, 2, 5], [5, 2, 0, 5], [5, 5, 5, 0]], dtype=float)
    assert b":-" in phy.neighbor_joining(D, list("abcd"))


def test_supermatrix_fasta(phy):
    m = np.frombuffer(b"AC-DE-GH", dtype=np.uint8).reshape(2, 4)
    assert phy.supermatrix_fasta([b"t1", b"t0"], m, [0, 2, 3]) == b">t1\nA-D\n>t0\nEGH\n"
    assert phy.supermatrix_fasta([b"t1", b"t0"], m, []) == b">t1\n\n>t0\n\n"


# ---------------------------------------------------------------------------------------------------------
# the whole stage on a hand-made search result, and the script
# ---------------------------------------------------------------------------------------------------------
FASTA = (b">A|g1\nACDEFGHIKL\n>A|g2\nMNPQRSTVWY\n>A|g3\nAAAAAAAA\n>B|h1\nACDFGHIKL\n>B|h2\nMNPQRWWSTVWY\n>C|k1\nCDEFGHIK\n>C|k2\nNPQRSTVW\n")
# q, s, qst, sst, bit, cigar: g1 ~ h1 (E dropped: an I against the anchor), g2 ~ h2 (WW inserted: a D), g1 ~ k1, g2 ~ k2 (both inside), and back
HITS = [(b"A|g1", b"B|h1", 1, 1, 40, b"3M1I6M"), (b"A|g1", b"C|k1", 2, 1, 35, b"8M"), (b"A|g2", b"B|h2", 1, 1, 42, b"5M2D5M"),
        (b"A|g2", b"C|k2", 2, 1, 33, b"8M"), (b"A|g2", b"C|k2", 2, 1, 20, b"4M"), (b"B|h1", b"A|g1", 1, 1, 40, b"3M1D6M"),
        (b"B|h2", b"A|g2", 1, 1, 42, b"5M2I5M"), (b"C|k1", b"A|g1", 1, 2, 35, b"8M"), (b"C|k2", b"A|g2", 1, 2, 33, b"8M")]


def sc_text(cigar=True):
    rows = []
    for q, s, qst, sst, bit, cg in HITS:
        f = [q, s, b"90.00", b"10", b"1", b"0", b"%d" % qst, b"10", b"%d" % sst, b"10", b"1e-20", b"%d" % bit, b"10", b"10", b"30", b"9"]
        rows.append(b"\t".join(f + ([cg] if cigar else [])) + b"\n")
    return b"".join(rows)


WANT_ROWS = {b"A": b"ACDEFGHIKL" + b"MNPQRSTVWY", b"B": b"ACD-FGHIKL" + b"MNPQRSTVWY", b"C": b"-CDEFGHIK-" + b"-NPQRSTVW-"}


def test_supermatrix_from_text(phy):
    from swiftortho_amd import find_orth, rbh
    sc = sc_text()
    cols = find_orth.columns_from_text(sc)
    table = rbh.core_table(cols, FASTA)
    assert [[x.decode() for x in g] for g in rbh.core_groups(cols.names, table)] == [["A|g1", "B|h1", "C|k1"], ["A|g2", "B|h2", "C|k2"]]
    nm = cols.names.tolist()
    assert [(nm[a], [nm[m] for _, m in mem]) for a, mem in phy.families(table)] == [(g[0], g) for g in rbh.core_groups(cols.names, table)]
    sm = phy.supermatrix(cols.names, table, rbh.fasta_records(FASTA), phy.TextRows(sc, cols.names), 1.0)
    assert sm.taxa == [b"A", b"B", b"C"] and sm.col_off.tolist() == [0, 10, 20]
    assert [sm.matrix[k].tobytes() for k in range(3)] == [WANT_ROWS[t] for t in sm.taxa]
    assert sm.gaps.tolist() == [1, 0, 0, 1, 0, 0, 0, 0, 0, 1] + [1] + [0] * 8 + [1] and sm.keep.tolist() == list(range(20))
    assert sm.cmp.tolist() == [[20, 19, 16], [19, 19, 15], [16, 15, 16]] and sm.same.tolist() == sm.cmp.tolist()
    trimmed = phy.supermatrix(cols.names, table, rbh.fasta_records(FASTA), phy.TextRows(sc, cols.names), 0.)
    assert trimmed.keep.tolist() == [1, 2, 4, 5, 6, 7, 8, 11, 12, 13, 14, 15, 16, 17, 18]
    # a member without a row is an error that names the pair
    lost = b"".join(l + b"\n" for l in sc.split(b"\n") if l and not l.startswith(b"A|g1\tC|k1"))
    cols2 = find_orth.columns_from_text(sc)
    with pytest.raises(ValueError) as e:
        phy.supermatrix(cols2.names, table, rbh.fasta_records(FASTA), phy.TextRows(lost, cols2.names))
    assert "A|g1" in str(e.value) and "C|k1" in str(e.value)


class ListRows:
    """rows held as lists: what supermatrix() asks of a row source"""

    def __init__(self, q, s, score, qst, sst, runs):
        self.q, self.s, self.score, self.qst, self.sst, self.runs = np.asarray(q), np.asarray(s), np.asarray(score, dtype=float), qst, sst, runs

    def alignment(self, rows):
        rows = np.asarray(rows).tolist()
        return np.asarray([self.qst[r] for r in rows]), np.asarray([self.sst[r] for r in rows]), [self.runs[r] for r in rows]


def test_reference_quirk(phy):
    """-r names another taxon than the largest: the reference leaves the anchor out of its own family (rbh.core_groups).  The anchor
    still gives the block its coordinates, no taxon gets its residues, the other members are projected as ever"""
    from swiftortho_amd import rbh
    T, R = 10, 3
    names = np.asarray([b"t%d|a" % t for t in range(T)])
    seqs = {b"t%d|a" % t: (b"t%d|a" % t, b"ACDEFGH"[:7 if t != 5 else 6] if t != R else b"ACDEFGHIK") for t in range(T)}
    fwd = np.asarray([[t if t != R else -1 for t in range(T)]])
    table = rbh.CoreTable([b"t%d" % t for t in range(T)], b"t3", np.asarray([R]), fwd, (fwd >= 0).astype(np.uint8))
    assert [g for g in rbh.core_groups(names, table)] == [[b"t%d|a" % t for t in range(T) if t != R]]
    fams = phy.families(table)
    assert fams == [(R, [(t, t) for t in range(T) if t != R])]
    others = [t for t in range(T) if t != R]
    rows = ListRows([R] * 9, others, [50.] * 9, [2] * 9, [1] * 9, [phy.pack_runs([(6 if t == 5 else 7, "M")]) for t in others])
    sm = phy.supermatrix(names, table, seqs, rows)
    assert sm.col_off.tolist() == [0, 9] and sm.matrix[R].tobytes() == b"-" * 9
    assert sm.matrix[0].tobytes() == b"-ACDEFGH-" and sm.matrix[5].tobytes() == b"-ACDEFG--" and sm.anchors.tolist() == [R]


def run_script(tmp_path, sc, extra=()):
    p, f = str(tmp_path / "x.sc"), str(tmp_path / "x.fsa")
    open(p, "wb").write(sc), open(f, "wb").write(FASTA)
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "rbh2phy.py"), "-i", p, "-f", f] + list(extra), capture_output=True), p


def test_script_without_A_is_unchanged(tmp_path):
    """no new flag: the family files, the -o file and the line on stderr as before -- 16 or 17 columns alike"""
    for k, cigar in enumerate((False, True)):
        d = tmp_path / str(k)
        d.mkdir()
        r, p = run_script(d, sc_text(cigar), ("-o", str(d / "g.tsv")))
        assert r.returncode == 0 and r.stdout == b""
        assert open(str(d / "g.tsv"), "rb").read() == b"A|g1\tB|h1\tC|k1\nA|g2\tB|h2\tC|k2\n"
        assert open(p + "_alns_tmp/0.fsa", "rb").read() == b">A|g1\nACDEFGHIKL\n>B|h1\nACDFGHIKL\n>C|k1\nCDEFGHIK\n"
        assert r.stderr.decode() == ("rbh2phy: 2 core families of reference taxon A written to %s_alns_tmp/ ; aligning them (famsa | mafft | muscle) and joining "
                                     "the alignments is not part of this port\n" % p)


def test_script_A_T(tmp_path, phy):
    tree = str(tmp_path / "x.nwk")
    r, p = run_script(tmp_path, sc_text(), ("-A", "T", "-G", "F", "-t", tree))
    assert r.returncode == 0, r.stderr
    assert r.stdout == b"".join(b">" + t + b"\n" + WANT_ROWS[t] + b"\n" for t in (b"A", b"B", b"C"))
    nwk = open(tree, "rb").read()
    assert nwk.endswith(b";\n") and set(pin.newick_splits(nwk.strip(), ["A", "B", "C"])) == {frozenset({1}), frozenset({2}), frozenset({1, 2})}
    assert not os.path.exists(p + "_alns_tmp")
    r, _ = run_script(tmp_path, sc_text(), ("-A", "T", "-g", "0"))
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"CDFGHIKNPQRSTVW"
    r, _ = run_script(tmp_path, sc_text(), ("-A", "T", "-t", tree, "-m", "poisson"))
    assert r.returncode == 0 and open(tree, "rb").read().endswith(b";\n")


def test_script_missing_column(tmp_path):
    r, _ = run_script(tmp_path, sc_text(False), ("-A", "T"))
    assert r.returncode == 2 and r.stdout == b"" and b"find_hit.py -C T" in r.stderr
