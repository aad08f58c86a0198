"""Inputs for the candidate stage of find_orth (tests/test_orth_candidates.py, tests/test_gpu_orth.py): a seeded generator of HitColumns
that reaches every path of csrc/orth.hip, a plain-Python restatement of the stage (dictionaries and loops, nothing shared with the numpy
code or the kernels) and small hand-made edge inputs."""
import numpy as np

from swiftortho_amd import find_orth as fo

# tier bounds of k_orth_run, mirrored from swiftortho_amd/csrc/tune.h (test_orth_candidates.py checks the mirror against the header)
ORTH_WAVE_ROWS = 64      # ORTH_WAVE_ROWS: longest run the wave tier takes
ORTH_LDS_ROWS = 1024     # ORTH_LDS_ROWS: longest run the LDS tier takes
ORTH_LDS_TAXA = 512      # ORTH_LDS_TAXA: most taxa the LDS tier takes
ROW_BOUNDS = (ORTH_WAVE_ROWS, ORTH_LDS_ROWS)

FLAG_SETS = {"no": (.5, 0., "no"), "bsr": (.5, 0., "bsr"), "bal_c3": (.3, 0., "bal"), "c7_y30": (.7, 30., "no")}   # the goldens' four
SCORES = np.array([40, 55, 70, 85, 100, 120, 150, 200], dtype=np.float64)
N_TAXA, PER_TAXON, FAMILY = 5, 520, 10
REPEAT_EXTRA = 7         # repeated rows of the hub runs whose DISTINCT subjects sit at a bound
BIG_HUB = 2000           # one run far beyond every bound
RETURNING = 12           # query ids that come back with a second run


def hub_plan():
    """(kept rows, distinct subjects) of every hub run: B - 1, B, B + 1 rows of distinct subjects, and B - 1, B, B + 1 distinct subjects
    with REPEAT_EXTRA repeated rows on top, for every row bound B; one long run"""
    plan = []
    for B in ROW_BOUNDS:
        for d in (-1, 0, 1):
            plan.append((B + d, B + d))
            plan.append((B + d + REPEAT_EXTRA, B + d))
    plan.append((BIG_HUB, BIG_HUB))
    return plan


def make_names(n_taxa=N_TAXA, per_taxon=PER_TAXON):
    names = np.array([b"t%03d|g%04d" % (t, g) for t in range(n_taxa) for g in range(per_taxon)], dtype=np.bytes_)
    assert np.all(names[1:] > names[:-1])
    return names


def generate(seed):
    """-> HitColumns of about 34 k rows over 2 600 names in 5 taxa (see the module docstring of test_orth_candidates.py for what it holds)"""
    rng = np.random.RandomState(1000 + seed)
    names = make_names()
    M = len(names)
    code = lambda t, g: t * PER_TAXON + g
    plan = hub_plan()
    hubs = [int(x) for x in rng.choice(M, len(plan), replace=False)]
    hubset = set(hubs)
    # families of 10: two genes of every taxon; 85 % of the pairs hit each other with one score, half of the others one way only
    runs = {c: [] for c in range(M)}   # query code -> rows (s, bit, safe from every filter)
    fams = []
    for f in range(PER_TAXON // 2):
        mem = [code(t, 2 * f + k) for t in range(N_TAXA) for k in range(2)]
        fams.append(mem)
        for c in mem:
            runs[c].append((c, 250., False))
        for i in range(FAMILY):
            for j in range(i + 1, FAMILY):
                sc = float(SCORES[rng.randint(len(SCORES))])
                u = rng.rand()
                if u < .85:
                    runs[mem[i]].append((mem[j], sc, False))
                    runs[mem[j]].append((mem[i], sc, False))
                elif u < .925:
                    x, y = (i, j) if rng.rand() < .5 else (j, i)
                    runs[mem[x]].append((mem[y], sc, False))
    # six families without a hub hold a planted triangle: a and b (two taxa) are each other's best hit by far (240), a and its sibling a2
    # score 245.  a and b both come back with a second run below, so a - b is proposed four times and a - a2 three times
    planted = []
    for mem in fams:
        if len(planted) < RETURNING and not hubset & set(mem):
            a, a2, b = mem[0], mem[1], mem[2]
            for x, y, v in ((a, b, 240.), (b, a, 240.), (a, a2, 245.), (a2, a, 245.)):
                runs[x] = [r for r in runs[x] if r[0] != y] + [(y, v, True)]
            planted += [a, b]
    # hubs: `distinct` subjects (no hub among them), half of which answer with the same score; the first rows - distinct subjects again, higher
    for h, (rows, distinct) in zip(hubs, plan):
        pool = np.array([c for c in range(M) if c not in hubset])
        subj = rng.choice(pool, distinct, replace=False)
        sco = SCORES[rng.randint(len(SCORES), size=distinct)]
        hub_rows = [(int(s), float(v), True) for s, v in zip(subj, sco)]
        for s, v, _ in hub_rows[::2]:
            runs[s].append((h, v, False))
        hub_rows += [(s, v + 10., True) for s, v, _ in hub_rows[:rows - distinct]]
        order = rng.permutation(len(hub_rows))
        runs[h] = [hub_rows[k] for k in order]
    # 5 % of the other rows once more, with a higher score
    for c in range(M):
        if c in hubset:
            continue
        extra = [(s, v + 15., False) for s, v, safe in runs[c] if not safe and v < 230. and rng.rand() < .05]
        runs[c] = sorted(runs[c] + extra, key=lambda r: -r[1])
    # file order: the queries shuffled; the planted ones come back with a second run (all their rows again) right behind another query's run
    order = [int(x) for x in rng.permutation(M) if runs[int(x)]]
    again = list(planted)
    blocks = []
    for k, c in enumerate(order):
        blocks.append((c, runs[c]))
        if k % 150 == 20 and again and again[-1] != c and (k + 1 >= len(order) or order[k + 1] != again[-1]):
            a = again.pop()
            blocks.append((a, runs[a]))
    assert not again and len(planted) == RETURNING
    q = np.array([c for c, rows in blocks for _ in rows], dtype=np.int64)
    s = np.array([r[0] for _, rows in blocks for r in rows], dtype=np.int64)
    bit = np.array([r[1] for _, rows in blocks for r in rows], dtype=np.float64)
    safe = np.array([r[2] for _, rows in blocks for r in rows], dtype=bool)
    n = len(q)
    # the hubs' and the planted rows pass every filter of FLAG_SETS (the hubs' run lengths are exact); the others are filtered here and there
    qlen = rng.randint(100, 400, size=n).astype(np.float64)
    cov = np.where(safe, 1., rng.choice([.25, .45, .6, .8, 1.], size=n, p=[.05, .05, .1, .2, .6]))
    qst = np.ones(n)
    qed = np.where(safe, qlen, np.maximum(np.floor(cov * qlen), 1.))
    idy = np.where(safe, 90., rng.choice([25.5, 45.25, 66.66, 99.99], size=n, p=[.05, .15, .4, .4]))
    aln = np.where(safe, 100., rng.randint(50, 300, size=n).astype(np.float64))
    return fo.HitColumns(names, q, s, idy, aln, qst, qed, bit, qlen)


def many_taxa(n_taxa, seed=0):
    """a small input over `n_taxa` taxa, one gene each: a hub of 100 subjects (the table tiers) and short mutual runs"""
    rng = np.random.RandomState(77 + seed)
    names = make_names(n_taxa, 1)
    rows = []
    hub = 3
    subj = [int(x) for x in rng.choice(np.arange(4, n_taxa), min(100, n_taxa - 4), replace=False)]
    for s in subj:
        rows.append((hub, s, float(SCORES[rng.randint(8)])))
    for s in subj[::2]:
        rows.append((s, hub, [r[2] for r in rows if r[1] == s][0]))
        rows.append((s, (s + 1) % n_taxa, 55.))
    for c in range(0, n_taxa - 1, 2):
        rows.append((c, c + 1, 70.))
        rows.append((c + 1, c, 70.))
    q, s, bit = (np.array([r[k] for r in rows], dtype=dt) for k, dt in ((0, np.int64), (1, np.int64), (2, np.float64)))
    n = len(q)
    one = np.ones(n)
    return fo.HitColumns(names, q, s, one * 90., one * 100., one, one * 100., bit, one * 100.)


def columns(names, rows):
    """rows: (q name, s name, idy, aln, qst, qed, bit, qlen) -> HitColumns"""
    names = np.array(sorted(set(names)), dtype=np.bytes_)
    pos = {nm: k for k, nm in enumerate(names.tolist())}
    f = lambda k: np.array([r[k] for r in rows], dtype=np.float64)
    return fo.HitColumns(names, np.array([pos[r[0]] for r in rows], dtype=np.int64), np.array([pos[r[1]] for r in rows], dtype=np.int64),
                         f(2), f(3), f(4), f(5), f(6), f(7))


def edge_inputs():
    """name -> HitColumns: the corner cases of the stage"""
    names = [b"a|1", b"a|2", b"a|3", b"b|1", b"b|2", b"c|1"]
    row = lambda q, s, bit, idy=90., qed=100.: (q, s, idy, 100., 1., qed, bit, 100.)
    out = {}
    out["no_rows"] = columns(names, [])
    out["no_names"] = columns([], [])
    out["all_filtered"] = columns(names, [row(b"a|1", b"b|1", 100., qed=10.), row(b"b|1", b"a|1", 100., qed=10.)])
    out["one_row"] = columns(names, [row(b"a|1", b"b|1", 100.)])
    out["self_only"] = columns(names, [row(b"a|1", b"a|1", 200.), row(b"b|1", b"b|1", 200.)])
    out["one_taxon"] = columns(names, [row(b"a|1", b"a|2", 100.), row(b"a|2", b"a|1", 100.), row(b"a|1", b"a|3", 80.), row(b"a|3", b"a|1", 90.), row(b"a|2", b"a|2", 300.)])
    out["one_sided"] = columns(names, [row(b"a|1", b"b|1", 100.), row(b"a|2", b"b|2", 90.), row(b"b|1", b"c|1", 80.), row(b"a|1", b"a|2", 120.)])
    # a negative score never reaches the maxima that start from 0: b|2 is no ortholog candidate of a|1, a|3 no in-paralog candidate of a|2
    out["negative"] = columns(names, [row(b"a|1", b"b|2", -5.), row(b"b|2", b"a|1", -5.), row(b"a|1", b"a|2", 50.), row(b"a|2", b"a|1", 50.),
                                      row(b"a|2", b"a|3", -1.), row(b"a|3", b"a|2", -1.), row(b"a|3", b"b|1", 40.), row(b"b|1", b"a|3", 40.)])
    # a|1 comes back: its pair with b|1 is proposed three times (dropped), the one with b|2 twice, by a|1 alone
    out["second_run"] = columns(names, [row(b"a|1", b"b|1", 100.), row(b"a|1", b"c|1", 60.), row(b"b|1", b"a|1", 100.), row(b"a|1", b"b|1", 100.),
                                        row(b"a|1", b"b|2", 100.), row(b"c|1", b"a|1", 60.), row(b"a|2", b"a|1", 10.), row(b"a|1", b"b|2", 100.)])
    # two rows of one subject inside a run: one proposal with the larger score; bsr takes a|1's reference from its first KEPT row (the second)
    out["dedupe_bsr"] = columns(names, [row(b"a|1", b"b|1", 500., qed=10.), row(b"a|1", b"b|1", 80.), row(b"a|1", b"b|1", 120.), row(b"b|1", b"a|1", 120.),
                                        row(b"a|1", b"a|2", 130.), row(b"a|2", b"a|1", 130.), row(b"b|1", b"b|2", 60.), row(b"b|2", b"b|1", 200.)])
    # the last pair of each sorted list keeps the larger proposal (b|2 - c|1: 70, not 65; a|2 - a|1 is the last in-paralog key: 130 / 110)
    out["last_pair"] = columns(names, [row(b"b|2", b"c|1", 60.), row(b"c|1", b"b|2", 70.), row(b"a|1", b"b|1", 90.), row(b"b|1", b"a|1", 100.),
                                       row(b"a|1", b"a|2", 130.), row(b"a|2", b"a|1", 110.)])
    return out


# ---------------------------------------------------------------------------------------------------------
# the stage in plain Python
# ---------------------------------------------------------------------------------------------------------
def reference(cols, coverage, identity, norm, sep="|"):
    """-> dict: the proposed candidate triples before 'exactly twice' (ot, ip: lists of (a, b, score); co: list), the tables after it, and the
    counters; numbers are Python floats computed with the same single IEEE operations"""
    names = cols.names.tolist()
    M = max(len(names), 1)
    tax = [nm.split(sep.encode())[0] for nm in names]
    rows = []
    ref = {}
    for i in range(len(cols.q)):
        qlen = float(cols.qlen[i])
        num = 1. + abs(float(cols.qed[i]) - float(cols.qst[i]))
        qcv = num / qlen if qlen != 0 else (float("nan") if num == 0 else float("inf"))
        if qcv < coverage or float(cols.idy[i]) < identity:
            continue
        q, s, bit, aln = int(cols.q[i]), int(cols.s[i]), float(cols.score[i]), float(cols.aln[i])
        ref.setdefault(q, bit)
        rows.append((q, s, bit, aln))
    runs = []
    for q, s, bit, aln in rows:
        sco = bit / ref[q] if norm == "bsr" else bit / aln if norm == "bal" else bit
        if not runs or runs[-1][0] != q:
            runs.append((q, {}))
        best = runs[-1][1]
        best[s] = max(best[s], sco) if s in best else sco
    ot, ip, co = [], [], []
    for q, best in runs:
        tmax, out_max = {}, 0.
        for s, v in best.items():
            tmax[tax[s]] = max(tmax.get(tax[s], 0.), v)
            if tax[s] != tax[q]:
                out_max = max(out_max, v)
        for s, v in best.items():
            a, b = min(q, s), max(q, s)
            if tax[s] == tax[q]:
                if v >= out_max and q != s:
                    ip += [(a, b, v), (b, a, v)]
            elif v >= tmax[tax[s]]:
                ot.append((a, b, v))
            else:
                co.append((a, b, v))

    def twice(tr):
        groups = {}
        for a, b, v in tr:
            groups.setdefault((a, b), []).append(v)
        keys = sorted(groups)
        res = []
        for k in keys:
            g = groups[k]
            if len(g) == 2:
                res.append((k[0], k[1], max(g) if k == keys[-1] else ((0. + g[0]) + g[1]) / 2.))
        sizes = sorted(set(len(g) for g in groups.values()))
        return res, sizes, bool(keys) and len(groups[keys[-1]]) == 2

    ot2, ot_sizes, ot_last = twice(ot)
    ip2, ip_sizes, ip_last = twice(ip)
    cob = {}
    for a, b, v in co:
        cob[a * M + b] = max(cob.get(a * M + b, v), v)
    return dict(ot=ot2, ip=ip2, co=sorted(cob.items()), ot_sizes=ot_sizes, ip_sizes=ip_sizes, ot_last=ot_last, ip_last=ip_last,
                n_rows=len(rows), n_runs=len(runs), n_groups=sum(len(b) for _, b in runs), run_rows=_run_rows(rows), run_subjects=[len(b) for _, b in runs])


def _run_rows(rows):
    out = []
    last = None
    for r in rows:
        if r[0] != last:
            out.append(0)
            last = r[0]
        out[-1] += 1
    return out


def tables(cand):
    """Candidates -> the comparable form reference() uses"""
    z = lambda a, b, s: list(zip(a.tolist(), b.tolist(), s.tolist()))
    return dict(ot=z(cand.ot_a, cand.ot_b, cand.ot_s), ip=z(cand.ip_a, cand.ip_b, cand.ip_s), co=list(zip(cand.co_key.tolist(), cand.co_best.tolist())),
                n_rows=cand.n_rows, n_runs=cand.n_runs, n_groups=cand.n_groups)


def same_candidates(x, y):
    """two Candidates: every array equal, float64 arrays bit for bit, and the counters"""
    for k in fo.Candidates.FIELDS:
        a, b = getattr(x, k), getattr(y, k)
        if a.dtype != b.dtype or a.shape != b.shape:
            return "%s: dtype / shape %s %s vs %s %s" % (k, a.dtype, a.shape, b.dtype, b.shape)
        if not np.array_equal(a.view(np.int64), b.view(np.int64)):
            return "%s differs" % k
    for k in ("n_rows", "n_runs", "n_groups"):
        if getattr(x, k) != getattr(y, k):
            return "%s: %d vs %d" % (k, getattr(x, k), getattr(y, k))
    return ""


def records_from_columns(cols, n_dup=6, seed=0):
    """so_hit records (numpy structured array, the layout of fsearch.Hits.array()) + query / subject id lists that columns_from_records() maps
    back to `cols`-like columns: integer fields, identities with more than two decimals, and `n_dup` ids that occur twice in the query
    list -- rows of a query use either ordinal, so runs of two ordinals of one id lie side by side and merge"""
    rng = np.random.RandomState(5 + seed)
    dt = np.dtype([(n, t) for n, t in (("qidx", "<i8"), ("sidx", "<i8"), ("identity", "<f8"), ("evalue", "<f8"), ("aln", "<i4"), ("mis", "<i4"), ("gap", "<i4"),
                                       ("qst", "<i4"), ("qed", "<i4"), ("sst", "<i4"), ("sed", "<i4"), ("bit", "<i4"), ("qlen", "<i4"), ("slen", "<i4"),
                                       ("matches", "<i4"), ("ungapped", "<i4"))])
    assert dt.itemsize == 80
    names = cols.names.tolist()
    M = len(names)
    # the id lists are NOT in name order: ordinals and codes differ
    qperm, sperm = rng.permutation(M), rng.permutation(M)
    used = np.unique(cols.q)
    dup = rng.choice(used, n_dup, replace=False)
    query_ids = [names[c] for c in qperm] + [names[c] for c in dup]
    subject_ids = [names[c] for c in sperm]
    q_ord = np.empty(M, dtype=np.int64)
    q_ord[qperm] = np.arange(M)
    s_ord = np.empty(M, dtype=np.int64)
    s_ord[sperm] = np.arange(M)
    n = len(cols.q)
    rec = np.zeros(n, dtype=dt)
    rec["qidx"] = q_ord[cols.q]
    # the second half of every duplicated query's rows goes under its second ordinal
    for k, c in enumerate(dup.tolist()):
        at = np.flatnonzero(cols.q == c)
        rec["qidx"][at[len(at) // 2:]] = M + k
    rec["sidx"] = s_ord[cols.s]
    rec["identity"] = rng.choice([66.666666, 99.995, 29.9999996, 30.0000004, 45.254999, 100.0, 25.5], size=n)
    for k in ("aln", "qst", "qed", "qlen"):
        rec[k] = getattr(cols, k).astype(np.int32)
    rec["bit"] = cols.score.astype(np.int32)
    rec["evalue"] = 1e-30
    return rec, query_ids, subject_ids


KEPT_EDGES = (256, 8192, 32768)   # kept-row positions at a workgroup, a scan tile and the single-launch scan's limit (csrc/k_util.hip)


def kept_edges(seed=0):
    """generate(seed) with a row that every FLAG_SETS filter drops (coverage 1 / 400) directly before and directly after the kept rows
    number KEPT_EDGES (from 0): the compaction offsets and the run heads of the kept rows change exactly on those edges.  The dropped
    rows ask the other way round with a score above every other, so a row kept by mistake changes runs, maxima and the bsr divisor."""
    c = generate(seed)
    kept = np.flatnonzero(~(((1. + np.abs(c.qed - c.qst)) / c.qlen < .5) | (c.idy < 0.)))
    at = np.array([r + d for k in KEPT_EDGES for r in [kept[k]] for d in (0, 1)])   # np.insert: before these rows of the table as it is
    src = np.repeat(kept[list(KEPT_EDGES)], 2)
    ins = lambda a, v: np.insert(a, at, v)
    return fo.HitColumns(c.names, ins(c.q, c.s[src]), ins(c.s, c.q[src]), ins(c.idy, 90.), ins(c.aln, 100.), ins(c.qst, 1.), ins(c.qed, 1.), ins(c.score, 300.),
                         ins(c.qlen, 400.))
