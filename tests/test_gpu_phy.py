"""The supermatrix stage on the GPU (csrc/phy.hip, include/sohit.h so_phy_rows / so_phy_build) against the numpy definitions
(swiftortho_amd/phy.py) array for array, on the designed cases of tests/phy_inputs.py: device memory poisoned, twice in one process, every
refusal; then end to end on a small proteome of six taxa, where the matrix is also held to the hit records' own statistics.

Run on the GPU box:  python -m pytest tests/test_gpu_phy.py -m gpu -q
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import phy_inputs as pin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def phy():
    from swiftortho_amd import phy
    return phy


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("SOHIT_POISON", "165")


def same_build(got, want, matrix=True):
    gm, gg, gk, gc, gs = got
    wm, wg, wk, wc, ws = want
    if matrix:
        assert gm.dtype == np.uint8 and gm.shape == wm.shape and (gm == wm).all()
    else:
        assert gm is None
    assert gg.dtype == np.int32 and gg.tolist() == wg.tolist()
    assert gk.dtype == np.int64 and gk.tolist() == wk.tolist()
    assert gc.dtype == np.int64 and gc.shape == wc.shape and (gc == wc).all()
    assert gs.dtype == np.int64 and (gs == ws).all()


def check_build(phy, tk, g=1.0):
    """device == numpy, twice in one process, and without the matrix"""
    want = phy.build(tk, g)
    stats = {}
    got = phy.device_build(tk, g, stats=stats)
    same_build(got, want)
    assert stats == {"waits": 1 if tk.col_off[-1] else 0}
    same_build(phy.device_build(tk, g), want)
    same_build(phy.device_build(tk, g, want_matrix=False), want, matrix=False)
    return want


# ---------------------------------------------------------------------------------------------------------
# so_phy_rows
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pin.row_cases(), ids=lambda c: c[0])
def test_rows(phy, case):
    _, q, s, sco, pq, ps = case
    want = phy.pick_rows(q, s, sco, pq, ps)
    for _ in range(2):
        got = phy.device_pick_rows(q, s, sco, pq, ps)
        assert got.dtype == np.int64 and got.tolist() == want.tolist()


def test_rows_many_pairs_and_refusals(phy):
    rng = np.random.RandomState(12)
    n = 20000
    q, s, sco = rng.randint(0, 300, size=n), rng.randint(0, 300, size=n), rng.randint(0, 50, size=n) / 4.
    pq, ps = rng.randint(0, 310, size=5000), rng.randint(0, 310, size=5000)
    assert phy.device_pick_rows(q, s, sco, pq, ps).tolist() == phy.pick_rows(q, s, sco, pq, ps).tolist()
    none = np.zeros(0, dtype=np.int64)
    assert phy.device_pick_rows(q, s, sco, none, none).tolist() == []
    bad = sco.copy()
    bad[77] = np.nan
    for args, word in (((q, s, bad, pq, ps), "NaN"), ((q, s, sco, -pq - 1, ps), "negative")):
        with pytest.raises(RuntimeError) as e:
            phy.device_pick_rows(*args)
        assert word in str(e.value)
        assert phy.device_pick_rows(q, s, sco, pq[:3], ps[:3]).tolist() == phy.pick_rows(q, s, sco, pq[:3], ps[:3]).tolist()


# ---------------------------------------------------------------------------------------------------------
# projection
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_projection(phy, seed):
    """anchors of 1, 63, 64, 65 and 257 columns; 0, 1, 64, 65 and 200 runs per task; a task that is the anchor; an empty block"""
    tk = pin.projection_case(seed)
    check_build(phy, tk, .5)


def test_projection_boundaries(phy):
    want = check_build(phy, pin.boundary_case())
    row = want[0][0]
    assert (row[:59] == 45).all() and (row[59:159] != 45).all() and (row[159:257] == 45).all()


def test_projection_many_tasks(phy):
    """more tasks than one workgroup's four waves, many families"""
    tk = pin.projection_case(5, anchor_lens=tuple(range(1, 80)), run_counts=(3, 7, 1, 0, 66), n_taxa=9)
    check_build(phy, tk, .34)


@pytest.mark.parametrize("case", pin.bad_task_cases(), ids=lambda c: c[0])
def test_bad_task_is_refused_and_nothing_is_written(phy, case):
    _, tk, word = case
    out = np.full((tk.n_taxa, int(tk.col_off[-1])), 165, dtype=np.uint8)
    with pytest.raises(RuntimeError) as e:
        phy.device_build(tk, out=out)
    assert word in str(e.value) and "family 1, slot 2" in str(e.value)
    assert (out == 165).all()                                   # the caller's buffer stays at its poison value
    good = pin.boundary_case()                                  # a refusal leaves nothing behind: the next call is served
    out = np.full((good.n_taxa, int(good.col_off[-1])), 165, dtype=np.uint8)
    got = phy.device_build(good, out=out)
    assert (out == phy.build(good)[0]).all() and (got[0] == out).all()


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
             (changed(fam=good.fam + 100), 1., "outside"), (changed(n_taxa=46341, **empty), 1., "46341 taxa"))
    want = phy.build(good)
    for tk, g, word in cases:
        with pytest.raises(RuntimeError) as e:
            phy.device_build(tk, g)
        assert word in str(e.value), (word, str(e.value))
    same_build(phy.device_build(good), want)


# ---------------------------------------------------------------------------------------------------------
# gaps / keep
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pin.gap_cases(), ids=lambda c: c[0])
def test_gaps_and_keep(phy, case):
    _, m, g = case
    want = check_build(phy, pin.tasks_from_matrix(m, 3), g)
    assert (want[0] == m).all()
    if case[0] == "keep_nothing":
        assert len(want[2]) == 0 and not want[3].any() and not want[4].any()


def test_no_columns_and_no_tasks(phy):
    """families of no columns launch nothing; taxa without any task are all gaps"""
    b = pin.Builder(3, [0, 0])
    b.anchor(0, 1, b"")
    got = phy.device_build(b.tasks())
    assert got[0].shape == (3, 0) and len(got[1]) == 0 and len(got[2]) == 0 and got[3].tolist() == [[0] * 3] * 3 and got[4].tolist() == [[0] * 3] * 3
    check_build(phy, pin.Builder(4, [70, 3]).tasks(), 1.)
    check_build(phy, pin.Builder(4, [70, 3]).tasks(), .5)


# ---------------------------------------------------------------------------------------------------------
# pair counts
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", pin.PAIR_TAXA)
def test_pair_counts(phy, T):
    """kept columns of 1, 3, 4, 5, 255, 256, 257 and one LDS chunk - 1, + 0, + 1, with gaps, an all-gap row and equal columns"""
    for L in pin.PAIR_COLS:
        m = pin.pair_matrix(T, L)
        check_build(phy, pin.tasks_from_matrix(m), 1.)


@pytest.mark.parametrize("T", [3, 65])
def test_pair_counts_keep_with_holes(phy, T):
    """columns trimmed away: the kept ones are gathered side by side, their number again around a word and a chunk"""
    rng = np.random.RandomState(T)
    for L, g in ((300, .25), (300, .15), (140, .2), (131, .18)):
        m = pin.gap_matrix(rng, T, L, .2)
        want = check_build(phy, pin.tasks_from_matrix(m, 2), g)
        assert 0 < len(want[2]) < L                 # (some columns go, some stay: the kept ones are not a prefix)


def test_pair_counts_bytes_of_a_word(phy):
    for _, m in pin.byte_cases():
        want = check_build(phy, pin.tasks_from_matrix(m))
        L = m.shape[1]
        assert want[4][0, 1] == L - 1 and want[4][0, 2] == L and (want[3] == L).all()


def test_pair_counts_ranges_of_several_chunks(phy):
    """more chunks than column ranges: a workgroup walks several chunks, and the last range is short"""
    L = pin.CHUNK_COLS * pin.RANGE_CHUNKS * 2 + pin.CHUNK_COLS + 5
    m = pin.pair_matrix(3, L)
    check_build(phy, pin.tasks_from_matrix(m))
    m = pin.pair_matrix(130, 700)                   # three tiles of taxa: the tiles above the diagonal are mirrored
    check_build(phy, pin.tasks_from_matrix(m))


# ---------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------
SEARCH_KW = dict(ssd="111111", nr="AST,CFILMVY,DN,EQ,G,H,KR,P,W", ht=12000017, chk=50000, step=1, v=500, expect=1e-5, flt="F")


@functools.lru_cache(maxsize=None)
def searched():
    """the six-taxon proteome searched once with cigar=True -> everything the end-to-end tests read (host copies)"""
    from swiftortho_amd import find_orth, fsearch, rbh
    fa = pin.six_taxa_proteome()
    ids = find_orth.fasta_ids(fa)
    s = fsearch.Searcher(**SEARCH_KW)
    try:
        s.load_ref_bytes(fa)
        s.load_queries_bytes(fa)
        hits = s.search(cigar=True)
        rec = hits.array()
        ops, off = hits.cigar_buffer()
        ops, off = ops.copy(), off.copy()
        hits.close()
    finally:
        s.close()
    cols = find_orth.columns_from_records(rec, ids, ids)
    return fa, rec, cols, ops, off, rbh.core_table(cols, fa), rbh.fasta_records(fa)


def test_end_to_end_matrix(phy):
    """device supermatrix == numpy's, and every (anchor, member) block against the record of the hit that aligned the pair: its non-gap
    columns number the M total of the row's CIGAR, and the columns that equal the anchor's residue number aln - mis.  (A record's `mis`
    counts every column whose two characters differ, gap columns included, and `gap` counts gap OPENINGS -- fsearch.aln_stats -- so the
    identical columns are aln - mis, the record's `matches`; subtracting `gap` as well would count the openings twice: on the first
    block of this proteome aln = 156, mis = 73, gap = 7, and 83 columns are identical.)"""
    fa, rec, cols, ops, off, table, records = searched()
    rows = phy.RecordRows(cols, rec["qst"], rec["sst"], ops, off)
    want = phy.supermatrix(cols.names, table, records, rows)
    got = phy.supermatrix(cols.names, table, records, rows, device_stage=True)
    assert len(want.taxa) == 6 and len(want.col_off) > 10
    assert (got.matrix == want.matrix).all() and got.gaps.tolist() == want.gaps.tolist() and got.keep.tolist() == want.keep.tolist()
    assert (got.cmp == want.cmp).all() and (got.same == want.same).all() and got.col_off.tolist() == want.col_off.tolist()
    # every (anchor, member) block against the hit record that aligned the pair -- the search's own statistics, not the code under test
    nm = cols.names.tolist()
    blocks = 0
    for f, (a, mem) in enumerate(phy.families(table)):
        c0, c1 = int(want.col_off[f]), int(want.col_off[f + 1])
        anchor = np.frombuffer(records[nm[a]][1], dtype=np.uint8)
        assert c1 - c0 == len(anchor)
        for slot, m in mem:
            block = got.matrix[slot, c0:c1]
            if m == a:
                assert (block == anchor).all()
                continue
            cand = np.flatnonzero((cols.q == a) & (cols.s == m))
            r = cand[np.argmax(cols.score[cand])]
            runs = ops[off[r]:off[r + 1]]
            m_total = int(sum(int(v) >> 4 for v in runs if int(v) & 15 == 0))
            assert int((block != 45).sum()) == m_total
            assert int(rec["aln"][r]) == int(sum(int(v) >> 4 for v in runs))
            identical = int((block == anchor).sum())
            assert identical == int(rec["aln"][r]) - int(rec["mis"][r]) == int(rec["matches"][r])
            blocks += 1
    assert blocks > 40


def test_bad_row_is_named(phy):
    """a CIGAR that leads past its anchor: supermatrix() refuses on either side and names the row's pair"""
    from swiftortho_amd import find_orth, rbh
    from test_phy import FASTA, sc_text
    sc = sc_text()
    cols = find_orth.columns_from_text(sc)
    table = rbh.core_table(cols, FASTA)
    bad = sc.replace(b"\t35\t10\t10\t30\t9\t8M\n", b"\t35\t10\t10\t30\t9\t12M\n", 1)      # A|g1 ~ C|k1 from column 2 on: 1 + 12 > 10
    assert bad != sc
    for stage in (False, True):
        with pytest.raises(ValueError) as e:
            phy.supermatrix(cols.names, table, rbh.fasta_records(FASTA), phy.TextRows(bad, cols.names), device_stage=stage)
        assert "past the anchor" in str(e.value) and "A|g1" in str(e.value) and "C|k1" in str(e.value)
        good = phy.supermatrix(cols.names, table, rbh.fasta_records(FASTA), phy.TextRows(sc, cols.names), device_stage=stage)
        assert good.matrix[2].tobytes() == b"-CDEFGHIK--NPQRSTVW-"


def test_end_to_end_script_and_pipeline(phy, tmp_path):
    from swiftortho_amd import fsearch, pipeline
    fa = searched()[0]
    p, sc = str(tmp_path / "x.fsa"), str(tmp_path / "x.sc")
    open(p, "wb").write(fa)
    s = fsearch.Searcher(**SEARCH_KW)
    try:
        s.load_ref_bytes(fa)
        s.load_queries_bytes(fa)
        hits = s.search(cigar=True)
        hits.write(sc)
        hits.close()
    finally:
        s.close()
    out = {}
    for g in "TF":
        tree = str(tmp_path / ("x_%s.nwk" % g))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "rbh2phy.py"), "-i", sc, "-f", p, "-A", "T", "-G", g, "-g", ".5", "-t", tree], capture_output=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out[g] = (r.stdout, open(tree, "rb").read())
    assert out["T"] == out["F"] and out["T"][0].count(b">") == 6
    newick, sm, t = pipeline.species_tree_from_search(p, gap_share=.5, **SEARCH_KW)
    taxa = [x.decode() for x in sm.taxa]
    splits = pin.newick_splits(newick, taxa)
    assert len(taxa) == 6 and len(splits) == 2 * 6 - 3 and all(frozenset({k}) in splits for k in range(1, 6))
    assert phy.supermatrix_fasta(sm.taxa, sm.matrix, sm.keep) == out["T"][0] and newick + b"\n" == out["T"][1]
    host = pipeline.species_tree_from_search(p, gap_share=.5, device_stage=False, **SEARCH_KW)
    assert host[0] == newick and (host[1].matrix == sm.matrix).all() and (host[1].same == sm.same).all()
    assert {"load", "search", "rbh", "supermatrix", "tree", "families", "kept"} <= set(t)
