"""Designed candidate lists for the chain between "candidates" and "rows" (csrc/k_phase2.hip: k_csort*, k_mktasks, k_round_counts*,
k_round_idx*, k_stop_round_w, k_final_select*, k_selected_idx).

A candidate is the best ungapped diagonal per subject with a score of 25 and more, and the reference walks a query's candidates in the
order of that score (its own quicksort by -score).  The builder therefore places subjects on ranks through their UNGAPPED scores and
decides hit or miss through their GAPPED ones:

* the query Q holds the six residues whose BLOSUM62 self score is 5 (R K Q E M T), no residue equal or similar to its neighbour, so a run
  of n identical residues scores exactly 5 n;
* every other residue of a subject is W, G or P, which score below zero against all six: an ungapped extension gains nothing outside
  what was planted;
* a DECOY ('M', a miss) is W/G/P noise around one exact copy of an n-residue window of Q, taken from different places of Q: ungapped
  score 5 n, and the gapped alignment finds no more than that -- far from `expect`;
* a low-ranked HIT ('H') is a stretch of Q cut into pieces of n - 1 residues, one of n, with ONE residue inserted at every cut.  Every
  piece lies on a diagonal of its own (the drift goes one way: pieces that came back to a diagonal would be chained through the noise
  between them, the X-drop of 30 is never reached there), so the ungapped score is that of the longest piece, 5 n, plus what chance seed hits on the same diagonal add
  (`hit_pool()` measures it); the banded alignment bridges the one-residue gaps (at most ten of them, inside the band of 16) and passes `expect`;
* a COPY ('C') is Q itself, or Q with a few substitutions: ungapped score near 600, the top ranks, equal bit scores.

A case lists its blocks in rank order, e.g. [("C", 1), ("M", 9), ("H", 1), ("M", 25)]; `family()` gives every block scores above those of
the block behind it, so the order inside a block is free (all hits, or all misses) and the order of the blocks is fixed.  `pattern(blocks)` is the
string of C/H/M the walk is expected to see.  Whether it does is decided by the oracle's walk alone, in tests/test_stop_rule.py.

Each case is (name, fasta_ref, fasta_qry, kw, label); label holds the pattern and the facts the case was built for (the rank of the stop,
`unmch` at the round ends, nsel ...), every one of them asserted there.  cm = ceil(mmiss) comes from the formula (`mmiss()`), never typed in.
"""
import math

import numpy as np

AA9 = "AST,CFILMVY,DN,EQ,G,H,KR,P,W"
CORE = "RKQEMT"
NOISE = "WGP"
# the longest decoy window: 5 n = 120 points of ungapped (and gapped) score
LEVELS = [24]
QLEN = 120
# (expect: a decoy's gapped score is its window's, at most 120 points = 50 bits; a hit of the pool reaches 75 bits and more; with
# D * li * lj between 2^17 and 2^25 the test  D li lj 2^-bit <= 1e-14  asks for 64 ... 72 bits)
EXPECT = 1e-14
BASE_KW = dict(ssd="111111", nr=AA9, ht=1000003, chk=50000, step=1, v=500, expect=EXPECT, flt="F", thr=1000000, max_miss=1e-3)

_SIM = {("R", "K"), ("Q", "E")}   # the pairs that score 2; every other pair of different core residues scores 1 at most


def _similar(a, b):
    return a == b or (a, b) in _SIM or (b, a) in _SIM


def make_query(seed, n=QLEN):
    """n residues of CORE, none equal or similar to the one before it nor equal to the one before that (what a piece meets on the
    next two diagonals)"""
    rng = np.random.default_rng(seed)
    q = []
    while len(q) < n:
        c = CORE[int(rng.integers(0, len(CORE)))]
        if (len(q) >= 1 and _similar(c, q[-1])) or (len(q) >= 2 and c == q[-2]):
            continue
        q.append(c)
    return "".join(q)


def _noise(rng, n):
    return "".join(NOISE[int(i)] for i in rng.integers(0, len(NOISE), n))


def decoy(rng, q, n):
    p = int(rng.integers(1, len(q) - n + 1))   # (not 0: the reference's extension never scores the query's first residue, fsearch.py:2466)
    return _noise(rng, int(rng.integers(30, 90))) + q[p:p + n] + _noise(rng, int(rng.integers(30, 90)))


def hit(rng, q, n, pieces=11):
    """one piece of n residues and up to pieces - 1 of n - 1 around it, a noise residue inserted at every cut"""
    k = min(pieces, 1 + (len(q) - n) // (n - 1))
    span = n + (k - 1) * (n - 1)
    a = int(rng.integers(0, len(q) - span + 1))
    big = int(rng.integers(0, k))
    out, pos = [], a
    for i in range(k):
        ln = n if i == big else n - 1
        out.append(q[pos:pos + ln])
        pos += ln
    body = out[0]
    for s in out[1:]:
        body += _noise(rng, 1) + s
    return _noise(rng, int(rng.integers(20, 60))) + body + _noise(rng, int(rng.integers(20, 60)))


def copy(rng, q, subs):
    b = list(q)
    for p in rng.choice(len(q), size=subs, replace=False) if subs else []:
        b[int(p)] = CORE[(CORE.index(b[int(p)]) + 1 + int(rng.integers(0, 5))) % 6]
    return "".join(b)


def pattern(blocks):
    return "".join(kind * n for kind, n in blocks)


_POOLS = {}


def hit_pool(q, seed):
    """hits of every piece length 7 ... 14 with their ungapped candidate scores, lowest first.  A hit's score is 5 n and what the other
    seed hits of its best diagonal add (the reference chains them, fsearch.py:2497-2509): it is measured, with the oracle's own index"""
    key = (q, seed)
    if key not in _POOLS:
        from oracle import oracle
        rng = np.random.default_rng(seed)
        seqs = [hit(rng, q, n) for n in range(7, 15) for _ in range(40)]
        ix = oracle.Index(fasta([("p%d" % i, s) for i, s in enumerate(seqs)]), BASE_KW["ssd"], AA9, 1, BASE_KW["ht"])
        ix.threshold = BASE_KW["thr"]
        sc = {int(c[0]): c for c in ix.find_msav_m(q)}
        # (kept: the hits whose banded alignment from the candidate's start reaches 75 bits, well above what `expect` asks for)
        _POOLS[key] = sorted((int(sc[i][1]), i, s) for i, s in enumerate(seqs)
                             if i in sc and oracle.kswat_st(q, s, int(sc[i][2]), int(sc[i][3]))[8] >= 75)
    return _POOLS[key]


def family(rng, q, blocks, tag, copy_subs=0, pool_seed=7):
    """-> [(name, sequence)] of one query's subjects, one per rank of pattern(blocks), in rank order.  The blocks take their scores from
    the last one upwards: a block of misses the shortest window that scores above everything below it, a block of hits the lowest
    hits of the pool that do"""
    pool = hit_pool(q, pool_seed)
    used, floor, out = set(), 40, []
    for kind, cnt in reversed(blocks):
        blk = []
        if kind == "C":
            blk = [copy(rng, q, int(rng.integers(0, copy_subs + 1))) for _ in range(cnt)]
            floor = 10 ** 9
        elif kind == "M":
            n = floor // 5 + 1
            assert n <= LEVELS[0], "the blocks need a decoy above %d points" % floor
            blk = [decoy(rng, q, n) for _ in range(cnt)]
            floor = 5 * n
        else:
            pick = [(sc, i, s) for sc, i, s in pool if sc > floor and i not in used][:cnt]
            assert len(pick) == cnt, "the pool holds too few hits above %d points" % floor
            used.update(i for _, i, _ in pick)
            blk = [s for _, _, s in pick]
            floor = max(sc for sc, _, _ in pick)
        out = [(kind, s) for s in blk] + out
    return [("%s_%s%04d" % (tag, kind.lower(), i), s) for i, (kind, s) in enumerate(out)]


def fasta(recs):
    return "".join(">%s\n%s\n" % r for r in recs).encode()


def shuffled(rng, recs):
    return [recs[int(i)] for i in rng.permutation(len(recs))]


def mmiss(n, max_miss):
    """fsearch.py:3052-3054, with -m raised to 1e-3 as blastp does on entry"""
    m = n * max(max_miss, 1e-3) + 1
    m = max(m, 100. / m)
    return min(max(m, 10.), 120.)


def vmax(v):
    return max(100, max(v + 100, int(v * 1.1)))   # fsearch.py:3059


def _family_of(spec, tag):
    """(query, its subjects in rank order, the generator behind them) of a SPECS entry"""
    rng = np.random.default_rng(spec["seed"])
    q = make_query(spec["seed"] + 1000)
    return q, family(rng, q, spec["blocks"], tag, spec.get("copy_subs", 0)), rng


def _case(name, spec):
    q, fam, rng = _family_of(spec, "s")
    recs = shuffled(rng, fam)
    kw = dict(BASE_KW)
    kw.update(spec.get("over", {}))
    n = len(recs)
    mm = mmiss(n, kw["max_miss"])
    lab = dict(patterns=[pattern(spec["blocks"])], n=[n], mmiss=[mm], cm=[math.ceil(mm)])
    label = spec.get("label")
    lab.update(label(n, math.ceil(mm)) if callable(label) else (label or {}))
    return (name, fasta(recs), fasta([("q0", q)]), kw, lab)


def _spec(blocks, seed, label=None, copy_subs=0, **over):
    return dict(blocks=blocks, seed=seed, label=label, copy_subs=copy_subs, over=over)


def _ballot_late(seed, bit, behind):
    """n = 420 candidates: rounds 1 to 4 hold cm ranks each (cm >= 64, their floor), round 5 its floor of 128.  Copies up to rank
    4 cm - 1 - k, then misses: `unmch` is k behind round 4 and the rule fires in round 5, the only round longer than what can stop it, at
    its bit cm - 1 - k = `bit`, with `behind` hits right behind the stop, aligned in the same round"""
    cm = math.ceil(mmiss(420, 1e-3))
    assert 64 <= cm <= 128 and 4 * cm + 128 <= 420
    k = cm - 1 - bit
    last = 4 * cm - 1 - k   # rank of the last copy
    blocks = [("C", last + 1), ("M", cm)] + ([("H", behind)] if behind else []) + [("M", 420 - (last + 1) - cm - behind)]
    return _spec(blocks, seed, dict(walked=[last + cm + 1], stop="miss", round_of_stop=5, bit_of_stop=bit, nsel=[last + 1],
                                    unmch_round_end=[[0, 0, 0, k]], behind=behind))


# name -> what one designed family is built from (blocks in rank order, seed, label, parameters that differ from BASE_KW)
SPECS = {
    # ---- the regimes of the mmiss clamp; the rule fires after exactly cm misses and the hit behind them is never aligned
    "clamp_n_maxmiss": _spec([("C", 2), ("M", 21), ("H", 1), ("M", 16)], 1, dict(cm_is=21, walked=[23], stop="miss", regime="n*m+1"), max_miss=0.5),
    "clamp_inverse": _spec([("C", 1), ("M", 25), ("H", 1), ("M", 3)], 2, dict(cm_is=25, walked=[26], stop="miss", regime="100/m"), max_miss=0.1),
    "clamp_floor_10": _spec([("C", 1), ("M", 10), ("H", 1), ("M", 24)], 3, dict(cm_is=10, mmiss_is=10.0, walked=[11], stop="miss", regime="floor"),
                            max_miss=0.25),
    "clamp_10_3": _spec([("C", 1), ("M", 11), ("H", 1), ("M", 18)], 4, dict(cm_is=11, walked=[12], stop="miss", regime="fraction"), max_miss=0.3),
    "clamp_ceiling_120": _spec([("C", 2), ("M", 120), ("H", 1), ("M", 7)], 5, dict(cm_is=120, mmiss_is=120.0, walked=[122], stop="miss", regime="ceiling"),
                               max_miss=1.0),
    "clamp_maxmiss_0": _spec([("C", 1), ("M", 91), ("H", 1), ("M", 17)], 6, dict(cm_is=91, walked=[92], stop="miss", regime="-m 0"), max_miss=0.0),
    # ---- one low-ranked hit after cm - 1, cm and cm + 1 misses (cm = 10)
    "hit_after_cm_minus_1": _spec([("C", 1), ("M", 9), ("H", 1), ("M", 25)], 7, dict(cm_is=10, walked=[21], stop="miss", nsel=[2]), max_miss=0.25),
    "hit_after_cm": _spec([("C", 1), ("M", 10), ("H", 1), ("M", 24)], 8, dict(cm_is=10, walked=[11], stop="miss", nsel=[1]), max_miss=0.25),
    "hit_after_cm_plus_1": _spec([("C", 1), ("M", 11), ("H", 1), ("M", 23)], 9, dict(cm_is=10, walked=[11], stop="miss", nsel=[1]), max_miss=0.25),
}
# ---- ballot steps: n = 170, cm = 86; round 1 is ranks 0 ... 85, its last hit at rank 85 - u leaves unmch = u, round 2 then holds 86 - u
# ranks and the rule fires on its last one: bit 62, bit 63 (used == 64), bit 0 and bit 15 of the second step
for _nm, _u in (("ballot_bit62", 23), ("ballot_bit63", 22), ("ballot_step2_bit0", 21), ("ballot_step2_bit15", 6)):
    SPECS[_nm] = _spec([("C", 86 - _u), ("M", 86), ("H", 1), ("M", 170 - (86 - _u) - 87)], 10 + _u,
                       dict(cm_is=86, walked=[86 - _u + 86], stop="miss", round_of_stop=2, bit_of_stop=85 - _u, nsel=[86 - _u], unmch_round_end=[[_u]]))
SPECS.update({
    # ... and in a round that goes on behind the stop, with hits there that must not reach sel
    "ballot_late_bit62_hits_behind": _ballot_late(40, 62, 10),
    "ballot_late_bit63_hits_behind": _ballot_late(41, 63, 10),
    "ballot_late_step2_bit0_hits_behind": _ballot_late(42, 64, 10),
    "ballot_late_step2_bit5": _ballot_late(43, 69, 0),
    # ---- round boundaries (cm = 11: rounds of ranks 0 ... 10, 11 ... 26, 27 ... 58, 59 ... 122)
    "rounds_carry_6_10_stop_on_last_rank": _spec(
        [("C", 1), ("M", 3), ("H", 1), ("M", 6), ("H", 1), ("M", 4), ("H", 1), ("M", 10), ("H", 1), ("M", 9), ("H", 1), ("M", 9), ("H", 1), ("M", 11)], 50,
        dict(cm_is=11, walked=[59], stop="miss", round_of_stop=3, bit_of_stop=31, nsel=[7], unmch_round_end=[[6, 10]], list_ends_at_round_end=True),
        max_miss=0.16),
    "rounds_hit_on_last_rank_list_ends_at_round_end": _spec(
        [("C", 1), ("M", 9), ("H", 1), ("M", 5), ("H", 1), ("M", 10)], 51,
        dict(cm_is=11, walked=[27], stop="end", nsel=[3], unmch_round_end=[[0]], list_ends_at_round_end=True), max_miss=0.37),
    "rounds_carry_1_6_list_ends_in_round_3": _spec(
        [("C", 1), ("M", 8), ("H", 1), ("M", 10), ("H", 1), ("M", 10), ("H", 1), ("M", 8)], 52,
        dict(cm_is=11, walked=[40], stop="end", nsel=[4], unmch_round_end=[[1, 6]]), max_miss=0.25),
    # unmch = 1, 6 and 5 behind rounds 1, 2 and 3 (minr 8, 16, 32); round 4 (ranks 59 ...) opens with 6 more misses and stops on the last
    # of them, rank 64 = bit 5 of the round: only the 5 carried over the end of round 3 make them 11
    "rounds_carry_1_6_5_stop_in_round_4": _spec(
        [("C", 1), ("M", 8), ("H", 1), ("M", 10), ("H", 1), ("M", 10), ("H", 1), ("M", 10), ("H", 1), ("M", 10), ("H", 1), ("M", 46)], 53,
        dict(cm_is=11, walked=[65], stop="miss", round_of_stop=4, bit_of_stop=5, nsel=[6], unmch_round_end=[[1, 6, 5]]), max_miss=0.095),
    # ---- quota stop, vmax, v = 0
    "quota_stop": _spec([("C", 20), ("M", 38)], 60, lambda n, cm: dict(cm_is=11, walked=[3 + cm], stop="quota", nsel=[3 + cm]), v=3, max_miss=0.17),
    "vmax_cut": _spec([("M", 50), ("H", 1), ("M", 51), ("H", 2), ("M", 26)], 61,
                      dict(cm_is=120, walked=[vmax(3)], stop="vmax", nsel=[2], ranks_listed=[vmax(3)]), v=3, max_miss=1.0),
    "v_zero": _spec([("C", 4), ("M", 5), ("H", 7), ("M", 42)], 62, lambda n, cm: dict(cm_is=11, walked=[16], stop="quota", nsel=[cm], rows=0), v=0, max_miss=0.17),
    # ---- final selection: fewer, as many and more selected rows than v; equal bit scores; more rows than the LDS sort holds
    "select_fewer_than_v": _spec([("C", 2), ("M", 3), ("H", 1), ("M", 30)], 70, dict(walked=[16], stop="miss", nsel=[3], rows=3), v=5, max_miss=0.25),
    "select_exactly_v": _spec([("C", 3), ("M", 3), ("H", 2), ("M", 28)], 71, dict(walked=[18], stop="miss", nsel=[5], rows=5), v=5, max_miss=0.25),
    "select_more_than_v_equal_bits": _spec([("C", 9), ("M", 27)], 72, dict(walked=[19], stop="miss", nsel=[9], rows=5, equal_bits=9), v=5, max_miss=0.25),
    "select_1100_rows_serial_sort": _spec([("C", 1100)], 73, dict(walked=[1100], stop="end", nsel=[1100], rows=1100, nsel_over=1024), copy_subs=2, v=2000),
})


def _rnd20(rng, n):
    aa = "ACDEFGHIKLMNPQRSTVWY"
    return "".join(aa[int(i)] for i in rng.integers(0, 20, n))


def _mutate(rng, s, rate):
    aa = "ACDEFGHIKLMNPQRSTVWY"
    return "".join(aa[int(rng.integers(0, 20))] if rng.random() < rate else ch for ch in s)


def tiles_long_query():
    """kswat_st_long: a query of 4 200 residues (two tiles per candidate that starts in its first 104 residues) against 30 subjects, two of
    them 4 500 residues long and close to the query along its whole length -- both of their tiles pass.  Ranks of two tasks: the serial
    lane-0 walk of k_stop_round_w, the only case that takes it"""
    rng = np.random.default_rng(80)
    q = _rnd20(rng, 4200)
    recs = [("long_a", _mutate(rng, q, 0.10) + _rnd20(rng, 300)), ("long_b", _mutate(rng, q, 0.25) + _rnd20(rng, 300))]
    for i in range(10):   # pieces of the query: hits of one tile (qi past residue 104) or two
        a = int(rng.integers(0, 3600))
        recs.append(("piece%02d" % i, _mutate(rng, q[a:a + int(rng.integers(200, 500))], 0.15)))
    for i in range(18):   # short windows of the query in unrelated sequences: candidates that miss
        a = int(rng.integers(0, 4180))
        recs.append(("decoy%02d" % i, _rnd20(rng, 120) + q[a:a + int(rng.integers(9, 14))] + _rnd20(rng, 120)))
    kw = dict(BASE_KW, expect=1e-5, max_miss=0.5)
    return ("tiles_long_query", fasta(shuffled(rng, recs)), fasta([("q0", q)]), kw, dict(tiled=True, two_passing_tiles=True, n=[30]))


def tiles_short_query_long_subject():
    """a short query against a subject of 4 300 residues: the long path of k_mktasks (a window of the subject) with ONE tile, so every
    rank still has one task and k_stop_round_w takes its ballot walk -- this is not serial-walk coverage"""
    rng = np.random.default_rng(81)
    sq = make_query(1081)
    fam = family(rng, sq, [("C", 1), ("M", 12), ("H", 1), ("M", 6)], "s")
    assert fam[0][0].startswith("s_c")
    fam[0] = ("s_long", _noise(rng, 2100) + sq + _noise(rng, 2080))
    return ("tiles_short_query_long_subject", fasta(shuffled(rng, fam)), fasta([("q0", sq)]), dict(BASE_KW, max_miss=0.5),
            dict(patterns=["C" + "M" * 12 + "H" + "M" * 6], n=[20], long_subject=True, one_task_per_rank=True, walked=[12], stop="miss", nsel=[1]))


# the short cases whose queries and families make up the mixed batch, in query order
MIXED = ["clamp_floor_10", "select_fewer_than_v", "ballot_bit63", "rounds_carry_6_10_stop_on_last_rank", "select_more_than_v_equal_bits",
         "quota_stop", "v_zero", "hit_after_cm_minus_1", "rounds_carry_1_6_5_stop_in_round_4"]
# What the batch leaves of each shape, per query: (ranks walked, (round, bit) of the stop, `unmch` behind every round but the last, selected
# tiles); None: the query has no rank.  All the families are written in the same six residues (no other residues share one self score,
# so the families cannot be given alphabets of their own): every query finds the other families' subjects too.  With the batch's `expect`
# they all miss (their alignments reach 81 bits at most, a family's own hits 91 and more), but their chance chains rank them above the
# query's own decoys, so a query walks its own copies and then misses: stops on the first ranks of round 2 with `unmch` 10 and 11 carried
# in, stops inside round 2 with 3 and 8 carried in, two quota stops in round 3, one of them with 7 carried in.  Read off the oracle's
# walk once, asserted against it in tests/test_stop_rule.py.
MIXED_SHAPES = [(13, (2, 0), [11], 1), (14, (2, 1), [10], 2), (31, (3, 3), [0, 0], 31), None, (13, (2, 0), [11], 1), (21, (2, 8), [3], 9),
                (31, (3, 3), [0, 7], 20), (16, (2, 3), [8], 4), (13, (2, 0), [11], 1), (12, (2, 0), [10], 1), (1, None, [], 1)]


def mixed_batch():
    """The queries and the families of the short cases in MIXED against ONE reference, in one batch, plus a query without a candidate
    (position 3) and one whose only candidate is its own copy (last): the queries finish in different rounds, so entries of rcnt = 0 sit
    between live ones, and carried `unmch`, stops on a round's first ranks and quota stops run beside other live queries.  The batch has
    one -m, one -v and one -e for all of them and every query sees the other families too, so a shape is not the one its own case has:
    MIXED_SHAPES says what it is here."""
    rng = np.random.default_rng(90)
    qs, recs = [], []
    for i, name in enumerate(MIXED):
        q, fam, _ = _family_of(SPECS[name], "f%d" % i)
        qs.append(("q%d_%s" % (i, name), q))
        recs += fam
    # two queries of residues no family holds
    other = "ACDFHILNSVY"
    qs.insert(3, ("q_none", "".join("HDN"[int(i)] for i in rng.integers(0, 3, 90))))
    single = "".join(other[int(i)] for i in rng.integers(0, len(other), 90))
    qs.append(("q_single", single))
    recs.append(("single_copy", single))
    kw = dict(BASE_KW, max_miss=0.02, v=20, expect=1.4e-19)   # (-e: 85 ... 87 bits, between the other families' subjects and a family's own hits)
    return ("mixed_batch", fasta(shuffled(rng, recs)), fasta(qs), kw,
            dict(mixed=True, no_candidate=3, single_candidate=len(qs) - 1, min_distinct_rounds=3, shapes=MIXED_SHAPES))


CASE_NAMES = list(SPECS) + ["tiles_long_query", "tiles_short_query_long_subject", "mixed_batch"]
_BUILDERS = {"tiles_long_query": tiles_long_query, "tiles_short_query_long_subject": tiles_short_query_long_subject, "mixed_batch": mixed_batch}
_CASES = {}


def case_names():
    """static: collecting the tests builds nothing"""
    return list(CASE_NAMES)


def case(name):
    """one case, built when a test first asks for it"""
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]() if name in _BUILDERS else _case(name, SPECS[name])
    return _CASES[name]


def all_cases():
    return [case(n) for n in CASE_NAMES]
