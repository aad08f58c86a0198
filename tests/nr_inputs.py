"""Designed inputs of the record expansion (swiftortho_amd/nr.py expand_records, so_nr_expand), shared by test_nr_tables.py (numpy
definition against the text nr2full) and test_gpu_nr.py (device against the numpy definition).  Member tables and record arrays are
built directly, without a search.

A case is described by its runs: (k, [n_j, ...]) = a collapsed query with k members whose rows hit subjects with n_j members.  Every run
gets a collapsed query of its own and every row a collapsed subject of its own (unless the case says otherwise); the members' ordinals
in the full file are a seeded permutation, so that neither table is the identity; every other field of a record is distinct over the
whole case, so that a copy taken from the wrong row shows."""
import collections

import numpy as np

from swiftortho_amd.nr import EXPAND_PIECE as PIECE

HIT = np.dtype([("qidx", "<i8"), ("sidx", "<i8"), ("identity", "<f8"), ("evalue", "<f8"), ("aln", "<i4"), ("mis", "<i4"), ("gap", "<i4"), ("qst", "<i4"),
                ("qed", "<i4"), ("sst", "<i4"), ("sed", "<i4"), ("bit", "<i4"), ("qlen", "<i4"), ("slen", "<i4"), ("matches", "<i4"), ("ungapped", "<i4")])
MID = HIT.names[2:]

Case = collections.namedtuple("Case", "name rec qoff qmem soff smem text")


def table(sizes, seed):
    """member table of groups with the given sizes: the members are a seeded permutation of 0 .. sum - 1"""
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(np.asarray(sizes, dtype=np.int64), out=off[1:])
    mem = np.random.RandomState(seed).permutation(int(off[-1])).astype(np.int32)
    return off, mem


def records(q, s):
    """records with the given qidx / sidx whose other fields are distinct over the array"""
    n = len(q)
    rec = np.zeros(n, dtype=HIT)
    i = np.arange(n, dtype=np.int64)
    rec["qidx"], rec["sidx"] = q, s
    rec["identity"], rec["evalue"] = i + 0.25, 1.0 / (i + 1.0)
    for f, name in enumerate(HIT.names[4:]):
        rec[name] = (i * 12 + f + 1) % (1 << 31)
    return rec


def from_runs(name, runs, seed=0, text=True, qidx_of_run=None, extra_q=(), extra_s=()):
    """runs: [(k, [n_j ...]) ...].  qidx_of_run: the collapsed query of each run (default: run r has query r); extra_q / extra_s: sizes of
    groups no record names, appended to the tables"""
    ks = [k for k, _ in runs]
    if qidx_of_run is None:
        qidx_of_run, qsizes = list(range(len(runs))), ks
    else:
        qsizes = [0] * (max(qidx_of_run) + 1)
        for r, c in enumerate(qidx_of_run):
            qsizes[c] = ks[r]
    ssizes = [n for _, ns in runs for n in ns]
    q = [qidx_of_run[r] for r, (_, ns) in enumerate(runs) for _ in ns]
    qoff, qmem = table(list(qsizes) + list(extra_q), seed + 1)
    soff, smem = table(list(ssizes) + list(extra_s), seed + 2)
    return Case(name, records(q, np.arange(len(ssizes))), qoff, qmem, soff, smem, text)


def run_edges(case):
    """the output positions at which a run of the case ends (= the next one begins)"""
    q, s = case.rec["qidx"], case.rec["sidx"]
    w = (case.qoff[q + 1] - case.qoff[q]) * (case.soff[s + 1] - case.soff[s])
    head = np.concatenate([[True], q[1:] != q[:-1]]) if len(q) else np.zeros(0, dtype=bool)
    ends = np.cumsum(w)
    last = np.concatenate([head[1:], [True]]) if len(q) else head
    return set(int(x) for x in ends[last])


def _cases():
    out = [from_runs("empty", []), from_runs("one_row", [(1, [1])], extra_q=[2], extra_s=[3])]
    # many 1 x 1 runs: the output is the input with its ordinals remapped; more than 256 scan blocks of 256 rows
    rs = np.random.RandomState(5)
    n = 70001
    qoff, qmem = table([1] * n, 11)
    soff, smem = table([1] * 500, 12)
    out.append(Case("ones", records(np.arange(n), rs.randint(0, 500, n)), qoff, qmem, soff, smem, True))
    out.append(from_runs("big_700x700", [(700, [700])], seed=3))
    # every k against every n_j, and a collapsed query that comes back in a later run
    sizes = [1, 2, 63, 64, 65, 700]
    out.append(from_runs("mixed", [(1, sizes), (2, sizes[::-1]), (3, sizes), (65, sizes), (2, [2, 1])], seed=7, qidx_of_run=[0, 1, 2, 3, 1], extra_q=[4], extra_s=[5]))
    # run boundaries at rows 255, 256 and 257 (the row kernels and the scan work in blocks of 256 rows)
    out.append(from_runs("row_edges", [(2, [1, 2] * 127 + [1]), (3, [2]), (1, [3]), (2, [1, 2, 3] * 100)], seed=9))
    # outputs that straddle the edges of the emit kernel's pieces: a run that ends at PIECE - 1, PIECE, PIECE + 1, and whole pieces
    for d, tag in ((-1, "m1"), (0, "0"), (1, "p1")):
        out.append(from_runs("piece_" + tag, [(1, [PIECE + d]), (3, [2, 1])], seed=20 + d))
        out.append(from_runs("piece_rows_" + tag, [(1, [1] * (PIECE + d)), (2, [3])], seed=30 + d))
    out.append(from_runs("piece_whole", [(2, [PIECE])], seed=40))
    out.append(from_runs("piece_last_m1", [(1, [2 * PIECE - 1])], seed=41))
    out.append(from_runs("piece_last_p1", [(1, [2 * PIECE + 1])], seed=42))
    # groups without members weigh nothing: a row of an empty subject, a run of an empty query (the text form cannot say this)
    out.append(from_runs("empty_groups", [(2, [0, 3, 0]), (0, [2, 2]), (3, [0]), (1, [0, 0, 4])], seed=50, text=False))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
_edges = set().union(*(run_edges(c) for c in CASES))
assert {PIECE - 1, PIECE, PIECE + 1} <= _edges, "no case ends a run at the piece size - 1, the size and the size + 1"
assert {2 * PIECE - 1, 2 * PIECE, 2 * PIECE + 1} <= _edges, "no case ends its output around a whole number of pieces"
_starts = set()
for _c in CASES:
    _q = _c.rec["qidx"]
    _starts |= set((np.flatnonzero(_q[1:] != _q[:-1]) + 1).tolist())
assert {255, 256, 257} <= _starts, "no run begins at rows 255, 256 and 257"


def bad_tables():
    """(name, kwargs of expand, fragment the message must hold): every table the call refuses before a device is touched"""
    c = BY_NAME["mixed"]
    base = dict(rec=c.rec, qoff=c.qoff, qmem=c.qmem, soff=c.soff, smem=c.smem)
    falls = c.soff.copy()
    falls[3] = falls[2] - 1
    late = c.qoff.copy()
    late[0] = 1
    twice = c.smem.copy()
    twice[5] = twice[4]                      # one member named twice (and so one missing)
    gone = c.qmem.copy()
    gone[0] = len(gone)                      # a member outside the file: one is missing
    return [("subject_falls", dict(base, soff=falls), "subject"), ("query_starts_late", dict(base, qoff=late), "query"),
            ("subject_twice", dict(base, smem=twice), "subject"), ("query_missing", dict(base, qmem=gone), "query")]


def bad_records():
    """(name, kwargs, fragment): records the device refuses, with the error word it reads together with the totals"""
    c = BY_NAME["row_edges"]
    base = dict(qoff=c.qoff, qmem=c.qmem, soff=c.soff, smem=c.smem)
    out = []
    for field, value, tag in (("qidx", len(c.qoff) - 1, "q_high"), ("qidx", -1, "q_neg"), ("sidx", len(c.soff) - 1, "s_high"), ("sidx", -1, "s_neg")):
        rec = c.rec.copy()
        rec[field][300] = value
        out.append((tag, dict(base, rec=rec), field))
    return out
