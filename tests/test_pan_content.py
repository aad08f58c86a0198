"""CPU-only: the gene-content definitions of swiftortho_amd/pan.py -- shared_counts, boot_shared, content_distances,
boot_content_distances, content_tree -- against a literal model (tests/pan_content_inputs.py: a triple loop, closed forms on hand tables, a
replicate loop), every refusal, the sorted taxon order, and scripts/pan_genome.py -t -d -m -B -S: the files' text, the unchanged standard
output, the exit codes.  The reference has no such product: the numpy functions are the definition the device is held to
(tests/test_gpu_pan_content.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pan_content_inputs as ci
from conftest import ROOT

SCRIPT = os.path.join(ROOT, "scripts", "pan_genome.py")


@pytest.fixture(scope="module")
def pan():
    from swiftortho_amd import pan
    return pan


@pytest.fixture(scope="module")
def phy():
    from swiftortho_amd import phy
    return phy


# ---------------------------------------------------------------------------------------------------------
# the integers
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,T", [(1, 1), (1, 3), (70, 7), (65, 66)])
def test_shared_counts_against_the_triple_loop(pan, phy, R, T):
    counts = ci.ramp(R, T) * np.random.RandomState(2).randint(1, 4, size=(R, T)).astype(np.int32)     # counts above 1: one presence
    S = pan.shared_counts(counts)
    assert S.dtype == np.int64 and S.shape == (T, T) and S.tolist() == ci.loop_shared(counts).tolist()
    thr = (counts > 0).sum(1)
    assert S.sum() == (thr ** 2).sum() and np.trace(S) == thr.sum()
    for seed, b in ((1, 0), (1, 5), (2 ** 64 - 1, 3)):
        draws = phy.boot_columns(seed, b, R)
        Sb = pan.boot_shared(counts, seed, b)
        assert Sb.dtype == np.int64 and Sb.tolist() == ci.loop_shared(counts, draws.tolist()).tolist()
        assert np.trace(Sb) == thr[draws].sum() and Sb.sum() == (thr[draws] ** 2).sum()
    assert pan.boot_shared(counts, 1, 5).tolist() != pan.boot_shared(counts, 1, 6).tolist() or R == 1


def test_ramp_tables_are_what_they_are_for(pan):
    for R, T in ci.RAMP_CHECKED:
        ci.ramp_facts(pan.shared_counts(ci.ramp(R, T)))


def test_rows_in_chunks(pan, phy, monkeypatch):
    """the float64 product walks the rows in chunks: the same integers whatever the chunk"""
    counts = ci.ramp(130, 9)
    want = pan.shared_counts(counts).tolist()
    monkeypatch.setattr(pan, "_ROW_STEP", 64)
    assert pan.shared_counts(counts).tolist() == want
    assert pan.boot_shared(counts, 3, 1).tolist() == ci.loop_shared(counts, phy.boot_columns(3, 1, 130).tolist()).tolist()


def test_hand_tables(pan):
    S = pan.shared_counts(ci.TWINS)
    assert S.tolist() == [[4, 4, 2], [4, 4, 2], [2, 2, 3]]              # rows 1 and 4 are held by all three
    J, O = pan.content_distances(S, "jaccard"), pan.content_distances(S, "overlap")
    assert J[0, 1] == 0. and O[0, 1] == 0. and J.dtype == np.float64
    assert J[0, 2] == 1. - 2. / (4 + 3 - 2) and O[0, 2] == 1. - 2. / 3. and J[2, 0] == J[0, 2] and O[2, 1] == O[0, 2]
    assert np.diagonal(J).tolist() == [0., 0., 0.] and np.diagonal(O).tolist() == [0., 0., 0.]
    assert pan.shared_counts(ci.LISTED_TWICE).tolist() == [[2, 1], [1, 2]]        # a member listed twice counts once
    S = pan.shared_counts(np.array([[1, 1, 1, 1]] * 3 + [[1, 0, 0, 0]]))
    assert S.tolist() == [[4, 3, 3, 3]] + [[3, 3, 3, 3]] * 3
    assert pan.content_distances(S, "overlap").tolist() == [[0.] * 4] * 4 and pan.content_distances(S, "jaccard")[0].tolist() == [0., .25, .25, .25]
    D, ok = pan.boot_content_distances(S, "jaccard")
    assert ok and D.tolist() == pan.content_distances(S, "jaccard").tolist()


def test_rows_behind_the_file_rows_count(pan):
    """the one-gene rows behind the file rows are families too: S[a, a] counts them"""
    counts = np.array([[1, 1], [1, 0], [0, 1], [0, 1]], dtype=np.int32)
    names = ["b", "a"]
    fasta, groups = ci.files_of(counts, names, n_file_rows=1)
    table = pan.member_table(fasta, groups, names)
    assert (table.n_rows, table.n_file_rows) == (4, 1)
    newick, S, D = pan.content_tree(table, names)
    assert S.tolist() == [[3, 1], [1, 2]]                   # sorted order: a (code 1) first
    assert D[0, 1] == 1. - 1. / 4. and newick == b"(a:0.375000,b:0.375000);"


def test_refusals(pan, phy):
    for counts, metric, a, b in ((ci.ZERO_GENOME, "overlap", "x", "z"), (ci.ZERO_GENOME, "jaccard", "z", "x"), (ci.ONE_ROW, "jaccard", "y", "z"),
                                 (ci.ONE_ROW, "overlap", "x", "y")):
        S = pan.shared_counts(counts)
        with pytest.raises(phy.DistanceRefused) as e:
            pan.content_distances(S, metric, ["x", "y", "z"])
        assert "taxa %s and %s" % (a, b) in str(e.value) and metric in str(e.value), str(e.value)
        D, ok = pan.boot_content_distances(S, metric)
        assert not ok and np.diagonal(D).tolist() == [0., 0., 0.]
        assert np.isfinite(D).all() == (counts is ci.ZERO_GENOME and metric == "jaccard")     # there only the empty genome's own denominator is 0
        with pytest.raises(phy.DistanceRefused):
            pan.content_tree(ci.table_of(pan, counts), ["x", "y", "z"], metric)
    with pytest.raises(phy.DistanceRefused) as e:
        pan.content_distances(np.zeros((1, 1), dtype=np.int64), "jaccard")
    assert "taxa 0 and 0" in str(e.value)
    S = pan.shared_counts(ci.TWINS)
    for call in (lambda: pan.content_distances(S, "dice"), lambda: pan.boot_content_distances(S, "simpson"), lambda: pan.content_distances(S[:2], "jaccard"),
                 lambda: pan.content_tree(ci.table_of(pan, ci.TWINS), ["x", "y", "z"], "p"),
                 lambda: pan.content_tree(ci.table_of(pan, ci.TWINS), ["x", "y", "z"], boot=-1),
                 lambda: pan.content_tree(ci.table_of(pan, ci.TWINS[:, :1]), ["x"]),
                 lambda: pan.content_tree(pan.MemberTable(np.zeros(0, np.int32), np.zeros(0, np.int32), 0, 0), [])):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(pan.TooFewTaxa):
        pan.content_tree(ci.table_of(pan, ci.TWINS[:, :1]), ["x"])


def test_no_valid_replicate(pan):
    counts, names = ci.lonely(), ["t%d" % k for k in range(8)]
    assert not any(pan.boot_content_distances(pan.boot_shared(counts, 1, b), "jaccard")[1] for b in range(4))
    assert pan.content_tree(ci.table_of(pan, counts), names)[0].count(b"t") == 8
    with pytest.raises(ValueError) as e:
        pan.content_tree(ci.table_of(pan, counts), names, boot=4, seed=1)
    assert "none of the 4 replicates" in str(e.value)


# ---------------------------------------------------------------------------------------------------------
# the tree
# ---------------------------------------------------------------------------------------------------------
def literal_tree(pan, phy, counts, names, metric, boot, seed):
    """content_tree by a plain replicate loop over a table whose codes ARE the sorted order"""
    assert names == sorted(names)
    S = ci.loop_shared(counts)
    D = pan.content_distances(S, metric, names)
    if not boot:
        return phy.neighbor_joining(D, names), S, D
    ref = [r.tobytes() for r in phy.tree_splits(D)]
    held, valid = [0] * len(ref), 0
    for b in range(boot):
        Db, ok = pan.boot_content_distances(ci.loop_shared(counts, phy.boot_columns(seed, b, len(counts)).tolist()), metric)
        if not ok:
            continue
        valid += 1
        mine = {r.tobytes() for r in phy.nj_splits(Db)}
        held = [h + (k in mine) for h, k in zip(held, ref)]
    return phy.neighbor_joining(D, names, np.asarray(held) / float(valid)), S, D


@pytest.mark.parametrize("metric", ["jaccard", "overlap"])
def test_supports_against_a_literal_replicate_loop(pan, phy, metric):
    for counts, boot, seed in ((ci.ramp(70, 9), 12, 1), (ci.with_rare_genome(), 16, 1), (ci.ramp(40, 3), 5, 9), (ci.ramp(40, 2), 3, 9)):
        T = counts.shape[1]
        names = ["s%02d" % k for k in range(T)]
        stats = {}
        got = pan.content_tree(ci.table_of(pan, counts), names, metric, boot, seed, stats=stats)
        want = literal_tree(pan, phy, counts, names, metric, boot, seed)
        assert got[0] == want[0] and got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist()
        assert got[1].dtype == np.int64 and got[2].dtype == np.float64 and stats["boot"] == boot and 1 <= stats["boot_valid"] <= boot
        assert got[0] != pan.content_tree(ci.table_of(pan, counts), names, metric)[0] or T < 4       # the labels are there
    stats = {}
    pan.content_tree(ci.table_of(pan, ci.with_rare_genome()), ["s%d" % k for k in range(7)], metric, 16, 1, stats=stats)
    assert 1 <= stats["boot_valid"] < 16                   # some replicates are dropped, some kept


@pytest.mark.parametrize("metric", ["jaccard", "overlap"])
def test_the_planted_split_holds_in_every_replicate(pan, phy, metric):
    counts, group = ci.planted()
    T = counts.shape[1]
    names = ["p%d" % k for k in range(T)]
    split = np.asarray(phy._clade_words(sum(1 << k for k in group), T), dtype=np.uint64).tobytes()
    newick, S, D = pan.content_tree(ci.table_of(pan, counts), names, metric, 16, 1)
    where = [r.tobytes() for r in phy.tree_splits(D)].index(split)
    for b in range(16):
        Db, ok = pan.boot_content_distances(pan.boot_shared(counts, 1, b), metric)
        assert ok and split in {r.tobytes() for r in phy.nj_splits(Db)}
    inner = newick.decode().replace(";", "").split(")")[1:]        # the labels stand behind the closing brackets, in join order
    assert inner[where].startswith("1.000:")


def test_taxa_are_listed_in_sorted_order_whatever_the_column_order(pan):
    counts = ci.ramp(70, 9)
    T = counts.shape[1]
    names = ["s%02d" % k for k in range(T)]
    want = pan.content_tree(ci.table_of(pan, counts), names, "jaccard", 8, 1)
    for seed in (1, 2):
        order = np.random.RandomState(seed).permutation(T)          # column c of the shuffled table is genome order[c]
        got = pan.content_tree(ci.table_of(pan, counts[:, order]), [names[k] for k in order], "jaccard", 8, 1)
        assert got[0] == want[0] and got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist()
    assert want[1].tolist() == pan.shared_counts(counts).tolist()


# ---------------------------------------------------------------------------------------------------------
# the script
# ---------------------------------------------------------------------------------------------------------
def run_script(d, counts, names, extra=(), n_file_rows=None, texts=None):
    fasta, groups = texts or ci.files_of(counts, names, n_file_rows)
    os.makedirs(str(d), exist_ok=True)
    fa, gr = str(d / "in.fsa"), str(d / "in.clsr")
    open(fa, "w").write(fasta), open(gr, "w").write(groups)
    env = dict(os.environ, PYTHONHASHSEED="0")                       # every run orders the columns of the report alike
    r = subprocess.run([sys.executable, SCRIPT, "-i", fa, "-g", gr] + list(extra), capture_output=True, cwd=str(d), env=env)
    read = lambda p: open(p, "rb").read() if os.path.isfile(p) else None
    return r, read(gr + "_xy.txt"), read(str(d / "t.nwk")), read(str(d / "d.tsv"))


def test_script_files_and_unchanged_output(pan, tmp_path):
    counts = ci.with_rare_genome()
    counts[3, :] = 0
    counts[3, 2] = 1                                                 # a row behind the file rows below
    counts = counts[np.concatenate([[k for k in range(len(counts)) if k != 3 and counts[k].any()], [3]])]     # (a group line lists a member at least)
    T = counts.shape[1]
    names = ci.names_of(T)
    plain, xy0, _, _ = run_script(tmp_path / "a", counts, names, n_file_rows=len(counts) - 1)
    assert plain.returncode == 0 and xy0
    for metric in ("jaccard", "overlap"):
        r, xy, nwk, tsv = run_script(tmp_path / metric, counts, names, ("-t", "t.nwk", "-d", "d.tsv", "-m", metric, "-B", "16", "-S", "3"), n_file_rows=len(counts) - 1)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.replace(("/%s/in.clsr" % metric).encode(), b"/a/in.clsr") == plain.stdout and xy == xy0
        fasta, groups = ci.files_of(counts, names, len(counts) - 1)
        table = pan.member_table(fasta, groups, names)
        newick, S, D = pan.content_tree(table, names, metric, 16, 3)
        assert nwk == newick + b"\n" and tsv.decode() == pan.content_table_text(sorted(names), S, D)
        lines = tsv.decode().split("\n")
        assert len(lines) == T * (T - 1) // 2 + 1 and lines[-1] == ""
        a, b, fa, fb, sh, dist = lines[0].split("\t")
        assert (a, b) == tuple(sorted(names)[:2]) and (int(fa), int(fb), int(sh)) == (S[0, 0], S[1, 1], S[0, 1]) and dist == repr(float(D[0, 1])) and float(dist) == D[0, 1]
    r, _, nwk, tsv = run_script(tmp_path / "d", counts, names, ("-d", "d.tsv"), n_file_rows=len(counts) - 1)
    assert r.returncode == 0 and nwk is None and tsv.decode() == pan.content_table_text(sorted(names), *pan.content_tree(table, names)[1:])
    r, _, nwk, tsv = run_script(tmp_path / "t", counts, names, ("-t", "t.nwk"), n_file_rows=len(counts) - 1)
    assert r.returncode == 0 and tsv is None and nwk == pan.content_tree(table, names)[0] + b"\n"


def test_script_exit_codes(tmp_path):
    counts, names = ci.ramp(20, 4), ci.names_of(4)
    counts = counts[counts.any(1)]                                   # (a group line lists a member at least)
    for k, (extra, word) in enumerate(((("-B", "4"), b"-t"), (("-B", "4", "-d", "d.tsv"), b"-t"), (("-t", "t.nwk", "-B", "many"), b"-B"),
                                        (("-t", "t.nwk", "-B", "-1"), b"-B"), (("-t", "t.nwk", "-B", str(2 ** 31)), b"-B"), (("-t", "t.nwk", "-S", "1.5"), b"-S"),
                                        (("-t", "t.nwk", "-S", str(2 ** 64)), b"-S"), (("-t", "t.nwk", "-m", "dice"), b"jaccard or overlap"),
                                        (("-m", "dice"), b"jaccard or overlap"))):
        r, xy, nwk, tsv = run_script(tmp_path / str(k), counts, names, extra)
        assert r.returncode == 2 and word in r.stderr and r.stderr.count(b"\n") == 1 and r.stdout == b"" and nwk is None and tsv is None and xy is None, (extra, r.stderr)
    r, xy, nwk, _ = run_script(tmp_path / "one", np.ones((3, 1), dtype=np.int32), names[:1], ("-t", "t.nwk"))
    assert r.returncode == 2 and b"two taxa" in r.stderr and r.stderr.count(b"\n") == 1 and nwk is None and xy is None
    for metric in ("jaccard", "overlap"):
        r, xy, nwk, tsv = run_script(tmp_path / ("empty_" + metric), None, None, ("-t", "t.nwk", "-d", "d.tsv", "-m", metric), texts=(ci.EMPTY_TAXON_FASTA, ci.EMPTY_TAXON_GROUPS))
        assert r.returncode == 2 and b"taxa a and ab" in r.stderr and metric.encode() in r.stderr and r.stderr.count(b"\n") == 1 and nwk is None and tsv is None and xy is None
    r, xy, _, _ = run_script(tmp_path / "ok", None, None, texts=(ci.EMPTY_TAXON_FASTA, ci.EMPTY_TAXON_GROUPS))
    assert r.returncode == 0 and xy is not None                     # without the new flags the same input is served as before
    r = subprocess.run([sys.executable, SCRIPT], capture_output=True)
    assert r.returncode == 0 and all(w in r.stdout for w in (b" -t:", b" -d:", b" -m:", b" -B:", b" -S:"))


def test_refusals_that_need_no_device(pan):
    """what so_pan_shared refuses before it looks for a device; and without a device the call fails loudly: no CPU fallback"""
    import torch
    from swiftortho_amd import build
    build.build(verbose=False)
    row, tax = ci.members(ci.ramp(20, 4))
    call = lambda **kw: pan._device_shared("t", **dict(dict(row=row, taxon=tax, n_rows=20, n_taxa=4, seed=1, b0=0, nb=0, device=0), **kw))
    for change, word in ((dict(n_taxa=0), "1 .. 4096"), (dict(n_taxa=4097), "1 .. 4096"), (dict(n_rows=1 << 31), "2^31 rows"), (dict(nb=-1), "n_reps"),
                         (dict(nb=32769), "32768"), (dict(nb=2, b0=2 ** 31 - 1), "2^31 - 1"), (dict(nb=1, b0=-1), "2^31 - 1"),
                         (dict(nb=1, n_rows=0, row=row[:0], taxon=tax[:0]), "no row to draw from"), (dict(n_rows=0), "a row outside")):
        with pytest.raises(RuntimeError) as e:
            call(**change)
        assert word in str(e.value), (change, str(e.value))
    import ctypes as C
    from swiftortho_amd import _lib
    L, res = _lib.load(), _lib.SoPanSharedResult()
    assert L.so_pan_shared(0, 0, None, None, 5, 3, C.c_uint64(0), 0, 0, 4, C.byref(res)) == 1 and b"unknown flag bits" in L.so_pan_last_error()
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError) as e:
            call()
        assert "HIP" in str(e.value)
