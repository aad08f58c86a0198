"""The phase-2 aligners task by task against the oracle's kswat_st (fsearch.py:1357-1476), through so_align_pairs.

End to end, a maximum that is a few points off changes no row unless it flips an accept / reject decision of the early-stop rule, and
k_align_lane takes only rounds of 2^18 packed tasks.  Here every aligner gets explicit windows and must return the oracle's maximum and
band cells exactly -- and the traced ones its coordinates, length, mismatches and gap openings -- at the lengths, starts, residue bytes,
ties, tile and 16-bit-range edges where they could differ.

  mode 0 k_align<false>, 1 k_align_pk<false>, 2 k_align_lane, 3 k_align<true> + k_traceback, 4 k_align_pk<true> + k_traceback

Run on the GPU box:  python -m pytest tests/test_gpu_align.py -m gpu -q
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AA = "ACDEFGHIKLMNPQRSTVWY"
ODD = "acdwy*-.0123456789BZJUOXx"   # the other residue bytes a FASTA line can carry
PK_LEN, PK_SCORE = 740, 8169          # the packed aligners' limits (k_align16.hip): min(rows, columns), or the smaller score bound
TRACED, PACKED = (3, 4), (1, 2, 4)


@pytest.fixture(scope="module")
def fs():
    from swiftortho_amd import fsearch
    return fsearch


@pytest.fixture(scope="module")
def rowmax(oracle):
    """per residue byte: max(0, its BLOSUM62 row maximum) -- what k_seq_bound adds up"""
    return np.maximum(0, oracle.b62_matrix().max(axis=1))


def fasta(seqs):
    return "".join(">x%d\n%s\n" % (i, s) for i, s in enumerate(seqs)).encode("latin-1")


class Set:
    """query and subject sequences loaded into one context; tasks (qidx, sidx, qi, qj, qe, se), qe / se = -1: the sequence's end"""

    def __init__(self, fs, qs, ss, env=None, monkeypatch=None):
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        self.qs, self.ss = list(qs), list(ss)
        self.s = fs.Searcher(ssd="111111", ht=1000003, flt="F")
        self.s.load_ref_bytes(fasta(self.ss))
        self.s.load_queries_bytes(fasta(self.qs))
        assert self.s.num_queries == len(self.qs) and self.s.num_refs == len(self.ss)

    def close(self):
        self.s.close()

    def windows(self, t):
        q, s = self.qs[t[0]], self.ss[t[1]]
        qe, se = len(q) if t[4] < 0 else t[4], len(s) if t[5] < 0 else t[5]
        return q[:qe], s[:se], t[2], t[3]

    def wide(self, t, rowmax):
        """k_task_rows's predicate recomputed: 11 * min(rows, columns) does not fit AND neither does the smaller score bound"""
        q, s, qi, qj = self.windows(t)
        bq = int(rowmax[np.frombuffer(self.qs[t[0]].encode("latin-1"), np.uint8)].sum())
        bs = int(rowmax[np.frombuffer(self.ss[t[1]].encode("latin-1"), np.uint8)].sum())
        return min(len(q) - qi, len(s) - qj) > PK_LEN and min(bq, bs) > PK_SCORE


_want_cache = {}


def expect(oracle, st, tasks):
    """oracle.kswat_st over each task's windows (the kswat_st_long tile framing for tiles): rows of
    (maxscore, aln, mis, gap, qst, qed, sst, sed, cells)"""
    out = np.zeros((len(tasks), 9), dtype=np.int64)
    for k, t in enumerate(tasks):
        key = st.windows(t)
        r = _want_cache.get(key)
        if r is None:
            g = oracle.kswat_st(*key, full=True)
            r = _want_cache[key] = (g[10], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[9])
        out[k] = r
    return out


def check(oracle, st, tasks, got, mode, what=""):
    """every task: the oracle's maximum and band cells; traced modes also aln, mismatches, gap openings and the coordinates (tasks
    without an alignment -- maximum 0, where the reference itself has no answer -- on the maximum and the cells only)"""
    tasks = [tuple(int(x) for x in t) for t in tasks]
    w = expect(oracle, st, tasks)
    g = np.stack([got["maxscore"], got["aln"], got["aln"] - got["matches"], got["gap"], got["qst"], got["qed"], got["sst"], got["sed"],
                  got["cells"]], axis=1).astype(np.int64)
    cols = [0, 8] + ([1, 2, 3, 4, 5, 6, 7] if mode in TRACED else [])
    bad = (g[:, cols] != w[:, cols]).any(axis=1)
    if mode in TRACED:
        bad &= ~((w[:, 1] == 0) & (g[:, [0, 8]] == w[:, [0, 8]]).all(axis=1))
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        q, s, qi, qj = st.windows(tasks[k])
        names = "maxscore aln mis gap qst qed sst sed cells"
        pytest.fail("%s mode %d: %d of %d tasks differ; first: task %d = %s\n q[%d] = %r\n s[%d] = %r\n gpu    %s = %s\n oracle %s = %s"
                    % (what, mode, int(bad.sum()), len(tasks), k, tasks[k], len(q), q[:120], len(s), s[:120], names, g[k].tolist(), names,
                       w[k].tolist()))


_strings_cache = {}


def expect_strings(oracle, st, tasks):
    """oracle.kswat_st's (query string, subject string) of each task's windows"""
    out = []
    for t in tasks:
        key = st.windows(t)
        w = _strings_cache.get(key)
        if w is None:
            w = _strings_cache[key] = oracle.kswat_st(*key, strings=True)[1]
        out.append(w)
    return out


def check_strings(oracle, st, tasks, got, alns, mode, what=""):
    """every task's strings byte for byte: the oracle's kswat_st al0 / al1 (none where the reference has no answer)"""
    tasks = [tuple(int(x) for x in t) for t in tasks]
    want = expect_strings(oracle, st, tasks)
    assert len(alns) == len(tasks)
    bad = [k for k in range(len(tasks)) if alns[k] != want[k]]
    if bad:
        k = bad[0]
        pytest.fail("%s mode %d: strings of %d of %d tasks differ; first: task %d = %s\n gpu    %r\n        %r\n oracle %r\n        %r"
                    % (what, mode, len(bad), len(tasks), k, tasks[k], alns[k][0][:200], alns[k][1][:200], want[k][0][:200], want[k][1][:200]))
    assert [len(a[0]) for a in alns] == got["aln"].tolist()


def run_modes(oracle, st, tasks, rowmax, modes=(0, 1, 2, 3, 4), what=""):
    """every mode on the tasks it can take; the wide flag against the predicate; packed modes refuse the others; the traced modes'
    strings (so_align_pairs_aln) against the oracle's, with the same records as without them"""
    tasks = [tuple(int(x) for x in t) for t in tasks]
    wide = np.array([st.wide(t, rowmax) for t in tasks], dtype=bool)
    res = {}
    for mode in modes:
        take = [k for k, t in enumerate(tasks) if not (mode in PACKED and wide[k])
                and not (mode == 2 and (t[4] >= 0 or t[5] >= 0 or len(st.qs[t[0]]) >= 4096 or len(st.ss[t[1]]) >= 4096))]
        sub = [tasks[k] for k in take]
        got = st.s.align_pairs(sub, mode)
        assert np.array_equal(got["wide"].astype(bool), wide[take]), "%s mode %d: wide flags differ from the predicate" % (what, mode)
        check(oracle, st, sub, got, mode, what)
        if mode in TRACED:
            got2, alns = st.s.align_pairs(sub, mode, alignments=True)
            assert np.array_equal(got2, got), "%s mode %d: asking for the strings changed the records" % (what, mode)
            check_strings(oracle, st, sub, got2, alns, mode, what)
        res[mode] = (take, got)
        if mode in PACKED and wide.any():
            k = int(np.flatnonzero(wide)[0])
            with pytest.raises(Exception, match="32-bit cells"):
                st.s.align_pairs([tasks[k]], mode)
    return res


def rnd(rng, n, alpha=AA):
    return "".join(alpha[i] for i in rng.integers(0, len(alpha), n))


def mutate(rng, a, rate, alpha=AA):
    """point changes and indels of 1-3 residues: the optimum drifts towards the band edge"""
    b = list(a)
    for _ in range(int(rng.binomial(len(a), rate))):
        p = int(rng.integers(0, len(b) + 1))
        r = rng.random()
        if r < 0.5 and p < len(b):
            b[p] = alpha[int(rng.integers(0, len(alpha)))]
        elif r < 0.75 and len(b) > 1:
            del b[p:p + int(rng.integers(1, 4))]
        else:
            b[p:p] = list(rnd(rng, int(rng.integers(1, 4)), alpha))
    return "".join(b) or a[:1]


def random_pairs(rng, n, alpha=AA, lmax=1200):
    """related (mutated copies with indels) and unrelated pairs of log-uniform lengths 1 .. lmax, either side the longer one"""
    qs, ss = [], []
    for _ in range(n):
        la = int(np.exp(rng.uniform(0, np.log(lmax))))
        a = rnd(rng, la, alpha)
        b = mutate(rng, a, float(rng.choice([0.02, 0.1, 0.25])), alpha) if rng.random() < 0.7 else rnd(rng, int(np.exp(rng.uniform(0, np.log(lmax)))), alpha)
        if rng.random() < 0.5:
            a, b = b, a
        qs.append(a), ss.append(b)
    return qs, ss


def starts(rng, la, lb):
    """0 mostly; len - 1, small offsets, equal windows"""
    r = rng.random()
    if r < 0.55:
        return 0, 0
    if r < 0.65:
        return max(0, la - 1), 0
    if r < 0.75:
        return 0, max(0, lb - 1)
    if r < 0.85:
        return (la - lb, 0) if la > lb else (0, lb - la)   # equal windows: the reference swaps the roles
    return int(rng.integers(0, max(1, min(la, 20)))), int(rng.integers(0, max(1, min(lb, 20))))


def pair_tasks(rng, qs, ss):
    return [(k, k, *starts(rng, len(qs[k]), len(ss[k])), -1, -1) for k in range(len(qs))]


def test_random_pairs_all_modes(fs, oracle, rowmax, monkeypatch):
    rng = np.random.default_rng(101)
    qs, ss = random_pairs(rng, 500)
    st = Set(fs, qs, ss)
    tasks = pair_tasks(rng, qs, ss)
    tasks += [(k, k, len(qs[k]), 0, -1, -1) for k in range(0, 500, 50)]   # an empty query window
    run_modes(oracle, st, tasks, rowmax, what="random pairs")
    st.close()


def test_ties_homopolymers_and_tandem_repeats(fs, oracle, rowmax):
    """equal values everywhere: the first maximum in row-major order and the priority diag > left > up > stop decide the coordinates"""
    rng = np.random.default_rng(102)
    qs, ss = [], []
    for period in (1, 1, 2, 2, 3, 3, 4, 5, 7):
        unit = rnd(rng, period)
        for _ in range(6):
            la, lb = int(rng.integers(1, 300)), int(rng.integers(1, 300))
            a, b = (unit * la)[:la], (unit * lb)[int(rng.integers(0, period)):][:lb] or unit
            if rng.random() < 0.4:   # one change: a tie between a gap and a mismatch
                b = list(b)
                b[int(rng.integers(0, len(b)))] = AA[int(rng.integers(0, 20))]
                b = "".join(b)
            qs.append(a), ss.append(b)
    for a, b in (("A" * 20, "A" * 27), ("W" * 9, "W" * 40), ("AG" * 15, "GA" * 15), ("ACD" * 12, "ACD" * 5 + "AC" + "ACD" * 6),
                 ("AAAAGAAAA" * 3, "AAAAAAAA" * 3), ("KR" * 30, "KKRR" * 15), ("P" * 5 + "A" * 30 + "P" * 5, "A" * 33)):
        qs += [a, b]
        ss += [b, a]
    st = Set(fs, qs, ss)
    run_modes(oracle, st, pair_tasks(rng, qs, ss), rowmax, what="ties")
    st.close()


def test_raw_residue_bytes(fs, oracle, rowmax):
    """lower case, '*', '-', '.', digits, B Z J U O X x in both sequences (the oracle scores raw bytes as the reference does)"""
    rng = np.random.default_rng(103)
    qs, ss = random_pairs(rng, 120, AA + ODD, lmax=400)
    qs += [ODD * 3, AA + ODD]
    ss += [ODD * 3, ODD + AA]
    st = Set(fs, qs, ss)
    run_modes(oracle, st, pair_tasks(rng, qs, ss), rowmax, what="raw bytes")
    st.close()


def test_packed_range_edges(fs, oracle, rowmax):
    """min(rows, columns) = 739 / 740 / 741 on W-rich pairs, and score bounds 8169 (packed: the self score is exactly the largest
    value the 16-bit cells hold) and 8171 (wide)"""
    rng = np.random.default_rng(104)
    qs, ss = [], []
    for n in (739, 740, 741, 742, 743):
        w = "".join("W" if rng.random() < 0.85 else AA[int(rng.integers(0, 20))] for _ in range(n))
        qs += [w, w, "W" * n]
        ss += [w, mutate(rng, w, 0.01)[:n + 1], "W" * n]
    for hi in ("WCHYP", "WC"):   # bounds above the limit: wide unless the shorter side is within 740
        a = rnd(rng, 1000, hi)
        qs += [a, a[:740], a[:741]]
        ss += [mutate(rng, a, 0.02), a, a]
    qs += ["W" * 742 + "P", "W" * 742 + "C"]
    ss += ["W" * 742 + "P", "W" * 742 + "C"]
    st = Set(fs, qs, ss)
    tasks = [(k, k, 0, 0, -1, -1) for k in range(len(qs))]
    wide = [st.wide(t, rowmax) for t in tasks]
    assert any(wide) and not all(wide)
    assert wide[-2:] == [False, True]
    res = run_modes(oracle, st, tasks, rowmax, what="packed range")
    take, got = res[0]
    assert got["maxscore"][-2:].tolist() == [8169, 8171]
    for mode in PACKED:   # the bound-8169 pair is packed, and scores its maximum without overflow
        take, got = res[mode]
        assert take[-1] == len(tasks) - 2 and got["maxscore"][-1] == 8169
    st.close()


def tile_tasks(st, q, s):
    """kswat_st_long's tiles (fsearch.py:1480-1498) of pair (q, s) aligned from (0, 0), as k_mktasks lays them out"""
    lq, ls = len(st.qs[q]), len(st.ss[s])
    out = []
    for i in range(0, lq, 4096):
        j = i
        t = (q, s, i, min(j, ls), min(lq, i + 4096), min(ls, j + 4096))
        if j >= ls:
            t = (q, s, i, ls, min(lq, i + 4096), ls)   # sqj[j:jed] is empty
        out.append(t)
    return out


def test_tiles(fs, oracle, rowmax):
    """sequences of 4095 / 4096 / 4097 / 8192 / 8193 residues: tiles starting at 0, 4096 and 8192, a last tile of one residue, a
    subject that ends before the query's last tile; k_align_lane refuses tiles and sequences of 4096+ residues"""
    rng = np.random.default_rng(105)
    qs, ss = [], []
    for n in (4095, 4096, 4097, 8192, 8193):
        a = rnd(rng, n)
        qs += [a, a]
        ss += [mutate(rng, a, 0.05), a[:5000] if n > 5000 else a[:3000]]
    st = Set(fs, qs, ss)
    tasks = [t for k in range(len(qs)) for t in tile_tasks(st, k, k)]
    assert {t[2] for t in tasks} == {0, 4096, 8192} and any(t[4] - t[2] == 1 for t in tasks)
    run_modes(oracle, st, tasks, rowmax, modes=(0, 1, 3, 4), what="tiles")
    with pytest.raises(Exception, match="no tile"):
        st.s.align_pairs([(6, 6, 0, 0, 4096, 4096)], 2)
    with pytest.raises(Exception, match="4096 residues or more"):
        st.s.align_pairs([(2, 2, 0, 0, -1, -1)], 2)
    st.close()


@pytest.fixture(scope="module")
def pool(fs, oracle):
    """1 100 pairs of 1-700 residues and their oracle answers, for the launch-list shapes"""
    rng = np.random.default_rng(106)
    qs, ss = random_pairs(rng, 1100, lmax=700)
    qs[:40] = [rnd(rng, 1) for _ in range(40)]   # one-row tasks
    ss[:40] = [rnd(rng, 1) for _ in range(40)]
    qs[40:80] = [rnd(rng, 700) for _ in range(40)]
    ss[40:80] = [mutate(rng, a, 0.1) for a in qs[40:80]]
    st = Set(fs, qs, ss)
    tasks = [(k, k, 0, 0, -1, -1) for k in range(len(qs))]
    expect(oracle, st, tasks)
    yield st, tasks
    st.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_launch_list_shapes(oracle, pool, mode):
    """n = 1 ... 1025 (odd n: an empty half in the last register), lists sorted by rows, reversed, 1-row and 700-row tasks interleaved,
    a task listed more than once"""
    st, tasks = pool
    rng = np.random.default_rng(107 + mode)
    rows = np.array([min(max(len(st.qs[t[0]]), len(st.ss[t[1]])), min(len(st.qs[t[0]]), len(st.ss[t[1]])) + 16) for t in tasks])
    for n in (1, 2, 3, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1025):
        pick = rng.choice(len(tasks), n, replace=False)
        sub = [tasks[int(k)] for k in pick]
        r = rows[pick]
        for name, order in (("identity", None), ("by rows", np.argsort(-r, kind="stable")), ("reversed", np.arange(n)[::-1].copy())):
            got = st.s.align_pairs(sub, mode, order=order)
            check(oracle, st, sub, got, mode, "n=%d %s" % (n, name))
    short, long_ = [t for t in tasks if len(st.qs[t[0]]) == 1][:30], tasks[40:70]
    mixed = [x for pair in zip(short, long_) for x in pair]
    check(oracle, st, mixed, st.s.align_pairs(mixed, mode), mode, "interleaved 1-row / 700-row")
    sub = tasks[100:133]
    order = np.arange(33, dtype=np.uint32)
    order[5] = order[20] = 7   # task 7 three times, tasks 5 and 20 not at all
    got = st.s.align_pairs(sub, mode, order=order)
    keep = [k for k in range(33) if k not in (5, 20)]
    check(oracle, st, [sub[k] for k in keep], got[keep], mode, "a task listed three times")
    assert (got[[5, 20]]["maxscore"] == -1).all()


@pytest.mark.parametrize("mode", TRACED)
def test_traced_launch_list_orders_with_strings(oracle, pool, rowmax, mode):
    """the traced modes on permuted launch lists (by rows, reversed, random; 1-row and 700-row tasks interleaved): the column slots,
    walks and compaction follow the list, the strings land per task -- the oracle's whatever the order"""
    st, tasks = pool
    rng = np.random.default_rng(120 + mode)
    tasks = [t for t in tasks if not (mode == 4 and st.wide(t, rowmax))]
    rows = np.array([min(max(len(st.qs[t[0]]), len(st.ss[t[1]])), min(len(st.qs[t[0]]), len(st.ss[t[1]])) + 16) for t in tasks])
    for n in (1, 17, 65, 513):
        pick = rng.choice(len(tasks), n, replace=False)
        sub = [tasks[int(k)] for k in pick]
        r = rows[pick]
        for name, order in (("by rows", np.argsort(-r, kind="stable")), ("reversed", np.arange(n)[::-1].copy()), ("random", rng.permutation(n))):
            got, alns = st.s.align_pairs(sub, mode, order=order, alignments=True)
            check(oracle, st, sub, got, mode, "n=%d %s" % (n, name))
            check_strings(oracle, st, sub, got, alns, mode, "n=%d %s" % (n, name))
    short, long_ = [t for t in tasks if len(st.qs[t[0]]) == 1][:30], tasks[40:70]
    mixed = [x for pair in zip(short, long_) for x in pair]
    got, alns = st.s.align_pairs(mixed, mode, alignments=True)
    check_strings(oracle, st, mixed, got, alns, mode, "interleaved 1-row / 700-row")


def test_edge_fixture_strings(fs, oracle, rowmax):
    """every case of tests/golden/kswat_aln_edges.json (the REAL reference's strings at the edges: indels in homopolymers and tandem
    repeats, literal '-' '*' lower-case and digit bytes, either side longer and equal lengths, the band edge, one-residue and empty
    windows, 4096-residue tiles) through both traced modes: the fixture's strings byte for byte"""
    from test_aln_fixtures import aln_edge_cases
    cases = aln_edge_cases()
    seqs = [x.decode("latin-1") for x in cases[0]["seqs"]]
    st = Set(fs, seqs, seqs)
    tasks = [(c["q"], c["s"], c["qlo"] + min(c["qst"], c["qhi"] - c["qlo"]), c["slo"] + min(c["sst"], c["shi"] - c["slo"]), c["qhi"], c["shi"])
             for c in cases]
    for mode in TRACED:
        take = [k for k, t in enumerate(tasks) if not (mode == 4 and st.wide(t, rowmax))]
        got, alns = st.s.align_pairs([tasks[k] for k in take], mode, alignments=True)
        check(oracle, st, [tasks[k] for k in take], got, mode, "edge fixture")
        for j, k in enumerate(take):
            c = cases[k]
            assert alns[j] == c["strings"], ("mode %d case %d" % (mode, k), c["cigar"], alns[j][0][:80], alns[j][1][:80])
        assert len(take) > 0.9 * len(tasks)
    st.close()


def test_lane_kernel_persistent_waves(fs, oracle, rowmax):
    """2^18 + 3 short tasks through k_align_lane twice in one context: its persistent waves take pairs from a work counter, and both
    launches must give the same results, the oracle's"""
    rng = np.random.default_rng(108)
    qs = [rnd(rng, int(rng.integers(20, 61))) for _ in range(3000)]
    ss = [mutate(rng, a, 0.15) if rng.random() < 0.5 else rnd(rng, int(rng.integers(20, 61))) for a in qs]
    st = Set(fs, qs, ss)
    n = (1 << 18) + 3
    qi = rng.integers(0, len(qs), n)
    si = np.where(rng.random(n) < 0.5, qi, rng.integers(0, len(ss), n))
    tasks = np.stack([qi, si, rng.integers(0, 4, n), rng.integers(0, 4, n), np.full(n, -1), np.full(n, -1)], axis=1)
    a = st.s.align_pairs(tasks, 2)
    b = st.s.align_pairs(tasks, 2)
    assert np.array_equal(a, b), "two launches of k_align_lane differ"
    check(oracle, st, tasks, a, 2, "2^18 + 3 tasks")
    st.close()


@pytest.mark.parametrize("poison", ["0xFF", "0x5A"])
def test_stale_device_memory(fs, oracle, rowmax, monkeypatch, poison):
    """every fresh device allocation filled with 0xFF / 0x5A: the same results, the oracle's"""
    rng = np.random.default_rng(109)
    qs, ss = random_pairs(rng, 150, lmax=900)
    st = Set(fs, qs, ss, {"SOHIT_POISON": poison}, monkeypatch)
    run_modes(oracle, st, pair_tasks(rng, qs, ss), rowmax, what="poison " + poison)
    st.close()


@pytest.mark.parametrize("env", [{"SOHIT_TRACE_WAVE_ROWS": "16", "SOHIT_TRACE_WAVE_MAX": "100000000"}, {"SOHIT_TRACE_WAVE_ROWS": "0"}],
                         ids=["every_walk_by_a_wave", "every_walk_by_a_thread"])
def test_both_traceback_walks(fs, oracle, rowmax, monkeypatch, env):
    rng = np.random.default_rng(110)
    qs, ss = random_pairs(rng, 200, lmax=1500)
    a = rnd(rng, 4400)
    qs.append(a), ss.append(mutate(rng, a, 0.05))
    st = Set(fs, qs, ss, env, monkeypatch)
    tasks = pair_tasks(rng, qs[:-1], ss[:-1]) + tile_tasks(st, len(qs) - 1, len(ss) - 1)
    run_modes(oracle, st, tasks, rowmax, modes=TRACED, what=str(env))
    st.close()


def test_refusals_write_nothing(fs, oracle):
    """tasks the search never hands a kernel are refused with a message, and the output stays untouched"""
    import ctypes as C
    st = Set(fs, ["W" * 742 + "C", "MKVLA" * 10, "A" * 4096], ["W" * 742 + "C", "MKVLA" * 9, "A" * 4100])
    cases = [((0, 0, 0, 0, -1, -1), 1, "32-bit cells"), ((0, 0, 0, 0, -1, -1), 2, "32-bit cells"), ((0, 0, 0, 0, -1, -1), 4, "32-bit cells"),
             ((1, 1, 0, 0, 40, -1), 2, "no tile"), ((2, 2, 0, 0, -1, 4096), 2, "no tile"), ((2, 1, 0, 0, -1, -1), 2, "4096 residues or more"),
             ((1, 1, 51, 0, -1, -1), 0, "out of range"), ((1, 1, 0, 0, 51, -1), 3, "out of range"), ((1, 1, 10, 0, 9, -1), 0, "out of range"),
             ((3, 1, 0, 0, -1, -1), 0, "out of range"), ((1, 3, 0, 0, -1, -1), 1, "out of range"), ((-1, 1, 0, 0, -1, -1), 0, "out of range"),
             ((2, 2, 0, 0, -1, -1), 3, "longer than 4096")]
    for task, mode, msg in cases:
        t = np.array([task, (1, 1, 0, 0, -1, -1)], dtype=np.int64)
        out = np.full(20, 12345, dtype=np.int32)
        rc = st.s.L.so_align_pairs(st.s.h, mode, 2, t.ctypes.data, None, out.ctypes.data)
        assert rc != 0 and msg in st.s.L.so_last_error(st.s.h).decode(), (task, mode)
        assert (out == 12345).all(), (task, mode)
    for order, mode in (([0, 2], 0), ([0, 0], 3), ([1, 1], 4)):
        t = np.array([(1, 1, 0, 0, -1, -1)] * 2, dtype=np.int64)
        o = np.array(order, dtype=np.uint32)
        out = np.full(20, 12345, dtype=np.int32)
        assert st.s.L.so_align_pairs(st.s.h, mode, 2, t.ctypes.data, o.ctypes.data, out.ctypes.data) != 0
        assert (out == 12345).all()
    assert st.s.L.so_align_pairs(st.s.h, 5, 1, np.zeros(6, np.int64).ctypes.data, None, np.zeros(10, np.int32).ctypes.data) != 0
    # and the pair every mode takes
    for mode in range(5):
        got = st.s.align_pairs([(1, 1, 0, 0, -1, -1)], mode)
        assert got["maxscore"][0] == oracle.kswat_st("MKVLA" * 10, "MKVLA" * 9, 0, 0, full=True)[10]
    st.close()
