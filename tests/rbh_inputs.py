"""Designed inputs of the reciprocal-best-hit stage (swiftortho_amd/rbh.py, csrc/rbh.hip): 16-column rows and the FASTA headers that go
with them, the smallest shapes at which a kernel can go wrong.  tools/refharness/make_rbh_goldens.py feeds exactly these bytes to the
REAL scripts and stores what they print (tests/golden/rbh_<name>.json), so every edge is pinned to the reference and not to a restatement.

    designed()  ->  {name: Case(sc bytes, fasta bytes, refs)}     refs: the -r values the golden holds ('' = the default)

What each input holds is said at its builder.  Everything is deterministic (seeded)."""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "sc fasta refs")

WAVE_ROWS = 64   # csrc/tune.h RBH_WAVE_ROWS: the longest run one wave holds


def row(q, s, score):
    """one 16-column find_hit row; only the ids and column 12 matter to the stage"""
    return "\t".join([q, s, "90.00", "100", "5", "0", "1", "100", "1", "100", "1e-30", str(score), "100", "100", "0", s + " d"]) + "\n"


def fasta_of(rows_text, extra=(), first=()):
    """a FASTA naming every id of the rows (in order of first appearance, `first` before them, `extra` behind)"""
    seen, out = set(), []
    ids = list(first)
    for l in rows_text.splitlines():
        ids += l.split("\t")[:2]
    for i in ids + list(extra):
        if i not in seen:
            seen.add(i)
            out.append(">%s some description\nACDEFGHIKL\nMNPQRSTVWY\n" % i)
    return "".join(out).encode()


def _case(rows, refs=("",), **kw):
    text = "".join(rows)
    return Case(text.encode(), fasta_of(text, **kw), list(refs))


SCORES = ["0", "-0.0", "1", "2", "3", "5", "7", "7.0", "7e0", "12.5"]   # ('7', '7.0' and '7e0' are one number; 0 and -0.0 tie)


def random_runs(seed, run_lens, n_taxa=5, genes=12):
    """runs of the given lengths over a small gene pool, so that best hits are reciprocated, queries come back in later runs and equal
    scores abound; subjects of the query's own taxon and self hits occur"""
    rng = np.random.default_rng(seed)
    pool = ["%s|g%02d" % (chr(97 + t), g) for t in range(n_taxa) for g in range(genes - t)]   # taxon a is the largest, then b, ...
    rows, prev = [], None
    for L in run_lens:
        q = prev
        while q == prev:
            q = pool[int(rng.integers(0, len(pool)))]
        prev = q
        for _ in range(L):
            rows.append(row(q, pool[int(rng.integers(0, len(pool)))], SCORES[int(rng.integers(0, len(SCORES)))]))
    return rows


def edge_runs():
    """runs of 1, 2, 63, 64, 65, 128, 129, 256 and 257 rows; the run of 64 covers rows 224 .. 287, across the boundary of the
    256-row workgroups of the per-row kernels, with runs of 30 and 65 rows around it"""
    lens = [1, 2, 63, 128, 30, 64, 65, 129, 256, 257] + [3, 1, 5, 2] * 8 + [1]   # (the short runs bring every gene back as a query)
    assert sum(lens[:5]) == 224
    return _case(random_runs(5, lens, n_taxa=4, genes=5), refs=("", "b", "zz"))


def edge_taxa():
    """1, 2, 63, 64, 65 and 300 subject taxa in one run, one row each (the first two sizes a second time with a tie on every taxon);
    every subject answers, so every pair prints; taxon q is the largest, and the run of 300 taxa gives the one complete core family"""
    rows = []
    for k, K in enumerate((1, 2, 63, 64, 65, 300)):
        q = "q|x%d" % k
        for t in range(K):
            rows.append(row(q, "t%03d|g%d" % (t, k), 10 + (t * 7) % 13))
        if K <= 2:
            for t in range(K):
                rows.append(row(q, "t%03d|h%d" % (t, k), 10 + (t * 7) % 13))    # an equal score later: the first row stays
        for t in range(K):
            rows.append(row("t%03d|g%d" % (t, k), q, 5))
    return _case(rows, first=["q|x%d" % k for k in range(6)] + ["q|pad%d" % k for k in range(3)])


def tie_block(tag, L, scores, default="1"):
    """a run of L rows of query a|<tag> over L genes of taxon b, `scores`: {row: text}; then every marked subject answers -- the pairs
    and the flags of the core table show which row won"""
    q = "a|%s" % tag
    rows = [row(q, "b|%s_%03d" % (tag, i), scores.get(i, default)) for i in range(L)]
    for i in sorted(scores):
        rows.append(row("b|%s_%03d" % (tag, i), q, 3))
    return rows


def edge_ties():
    """ties, where the FIRST row must win: equal maxima in neighbouring lanes, in lanes 0 and 63, at rows 63 and 64 of a long run, 0
    against -0.0 in either order (short and long runs), a later larger score after an equal pair, and '7' '7.0' '7e0'"""
    rows = []
    rows += tie_block("near", 10, {4: "9", 5: "9"})
    rows += tie_block("ends", 64, {0: "9", 63: "9"})
    rows += tie_block("seam", 130, {63: "9", 64: "9"})
    rows += tie_block("zero", 3, {1: "0", 2: "-0.0"}, default="-5")
    rows += tie_block("nzero", 3, {1: "-0.0", 2: "0"}, default="-5")
    rows += tie_block("lzero", 70, {10: "-0.0", 69: "0"}, default="-3")
    rows += tie_block("later", 8, {1: "9", 2: "9", 6: "10"})
    rows += tie_block("seven", 6, {2: "7", 3: "7.0", 4: "7e0"})
    rows += tie_block("lseven", 100, {20: "7e0", 70: "7", 99: "7.0"})
    return _case(rows)


def edge_pairs():
    """a key proposed 3 times (prints once) and 4 times (prints twice) by a query with two / three runs, a pair proposed once, two
    queries whose best hits point at different partners, a run of only self-taxon rows, self hits, and a last row that is a run of its own"""
    rows = [
        row("a|m1", "b|m1", 50), row("b|m1", "a|m1", 50), row("c|z", "a|m9", 7), row("a|m1", "b|m1", 50),
        row("a|m2", "b|m2", 40), row("b|m2", "a|m2", 40), row("a|m2", "b|m2", 41), row("b|m2", "a|m2", 42), row("a|m2", "c|z", 1),
        row("a|m3", "b|m3", 30),
        row("a|m4", "b|m4", 20), row("b|m4", "a|m5", 20), row("a|m5", "b|m6", 20),
        row("a|m6", "a|m7", 99), row("a|m6", "a|m6", 120),
        row("b|m8", "b|m8", 200), row("b|m8", "a|m8", 60), row("a|m8", "a|m8", 200), row("a|m8", "b|m8", 60),
        row("c|last", "a|m8", 9),
    ]
    return _case(rows, refs=("", "b", "c"))


def edge_core():
    """the core table.  Taxa A (4 genes), B and C (3 each: B comes first in the FASTA, so it has slot 1).  A|1's second run overwrites
    its forward hit in B and not in C; A|2's flag in B is set only by B|3's LATER run; A|3's forward hit in B is not reciprocal;
    -r: the largest taxon (default), a smaller one, and one absent from the hits"""
    rows = [
        row("A|1", "B|1", 50), row("A|1", "C|1", 40), row("A|1", "A|2", 90),
        row("B|1", "A|1", 50),
        row("A|2", "B|3", 33), row("A|2", "C|2", 32),
        row("B|3", "A|3", 70), row("B|3", "C|3", 5),
        row("A|1", "B|2", 30),
        row("B|2", "A|1", 30), row("C|1", "A|1", 40),
        row("B|3", "A|2", 33),
        row("C|2", "A|2", 32), row("C|2", "B|3", 1),
        row("A|3", "B|1", 20), row("A|3", "C|3", 21),
        row("C|3", "A|3", 21),
    ]
    return _case(rows, refs=("", "B", "C", "D"), first=["A|1", "A|2", "A|3", "A|4", "B|1", "C|1", "C|2", "C|3", "B|2", "B|3"])


def edge_lonely():
    """a FASTA header and a hit id without the separator: the whole header LINE is the taxon (so it carries no description here), the
    whole id the taxon of the hit; the last header has no line end and loses its last character, as in the script"""
    rows = [row("a|1", "lonely", 12), row("a|1", "a|2", 50), row("lonely", "a|1", 12), row("a|2", "lonely", 3)]
    return Case("".join(rows).encode(), b">a|1 d\nACDEF\n>lonely\nACDEF\n>a|2 d\nACDEF\n>a|3x", [""])


def edge_absent_taxon():
    """a hit taxon that is not in the FASTA: rbh2phy.py raises KeyError, core_table() refuses; get_rbh.py needs no FASTA"""
    rows = [row("a|1", "x|9", 12), row("a|1", "b|1", 11), row("x|9", "a|1", 12), row("b|1", "a|1", 11)]
    text = "".join(rows)
    return Case(text.encode(), fasta_of("", extra=["a|1", "a|2", "b|1"]), [""])


def edge_empty():
    return Case(b"", fasta_of("", extra=["a|1", "b|1"]), [""])


def edge_one():
    return _case([row("a|1", "b|1", 4)])


def edge_nan():
    """NaN scores: outside the numpy definition and the kernels (Python's `<` and sort disagree on them) -- served by the literal loops"""
    rows = [row("a|1", "b|1", "nan"), row("a|1", "b|2", 5), row("a|1", "b|3", "nan"), row("a|1", "b|4", 7), row("a|1", "c|1", 2), row("a|1", "c|2", "nan"),
            row("a|2", "b|2", 6), row("a|2", "b|1", "nan"), row("a|2", "b|4", 7)]
    for s in ("b|1", "b|2", "b|3", "b|4", "c|1", "c|2"):
        rows.append(row(s, "a|1", 5))
        rows.append(row(s, "a|2", "nan" if s == "b|4" else 4))
    return _case(rows, refs=("", "b"))


BUILDERS = {"edge_runs": edge_runs, "edge_taxa": edge_taxa, "edge_ties": edge_ties, "edge_pairs": edge_pairs, "edge_core": edge_core,
            "edge_lonely": edge_lonely, "edge_absent_taxon": edge_absent_taxon, "edge_empty": edge_empty, "edge_one": edge_one, "edge_nan": edge_nan}


def designed():
    return {k: f() for k, f in BUILDERS.items()}


def taxa_headers(counts, sep="|"):
    """the header lines of a multi-taxon generator file with counts[t] genes in taxon t, genes numbered through"""
    out, k = [], 0
    for t, c in enumerate(counts):
        for _ in range(c):
            out.append("tx%02d%sg%05d some description" % (t, sep, k))
            k += 1
    return out


def dummy_fasta(headers):
    """a FASTA with the given header lines (without '>') and stand-in residues: the stage reads only the headers"""
    return "".join(">%s\nACDEFGHIKL\n" % h for h in headers).encode()


# ---- the goldens (tests/golden/rbh_<name>.json: what the REAL scripts gave on these bytes) ------------------------------------------
def golden_names():
    import os
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    return sorted(f[4:-5] for f in os.listdir(gold) if f.startswith("rbh_") and f.endswith(".json"))


_loaded = {}


def golden(name):
    """-> (sc bytes, fasta bytes, meta): meta['pairs'] the text of get_rbh.py, meta['groups'][-r value] the groups of rbh2phy.py,
    meta['raises'] the -r values at which it raises"""
    import json
    import os
    if name not in _loaded:
        gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        meta = json.load(open(os.path.join(gold, "rbh_%s.json" % name)))
        if "designed" in meta:
            case = BUILDERS[meta["designed"]]()
            sc, fasta = case.sc, case.fasta
            assert sorted(case.refs) == sorted(list(meta["groups"]) + meta["raises"]), "the golden is older than the input: run make_rbh_goldens.py"
        else:
            sc = open(os.path.join(gold, meta["input"]), "rb").read() if "input" in meta else "".join(row(*r) for r in meta["rows"]).encode()
            fasta = dummy_fasta(taxa_headers(meta["counts"], meta["sep"]))
        _loaded[name] = (sc, fasta, meta)
    return _loaded[name]


def golden_ref_cases():
    """(name, -r value) of every golden group list and refusal"""
    return [(n, r) for n in golden_names() for r in sorted(list(golden(n)[2]["groups"]) + golden(n)[2]["raises"])]


def random_columns(seed, n_runs=400, n_taxa=6, genes=7, long_every=37):
    """a seeded random table as (sc bytes, fasta bytes): mostly short runs, every `long_every`-th one longer than a wave holds"""
    rng = np.random.default_rng(seed)
    lens = [int(rng.integers(65, 200)) if k % long_every == long_every - 1 else int(rng.integers(1, 20)) for k in range(n_runs)]
    text = "".join(random_runs(seed + 1000, lens, n_taxa=n_taxa, genes=genes))
    return text.encode(), fasta_of(text)


# ---- run shapes at the edges of the run kernels and of the scan under them (csrc/k_util.hip: 256 rows a workgroup, SCAN_TILE = 8192 values
# a tile, up to SCAN_SMALL_TILES = 4 tiles in one launch) ---------------------------------------------------------------------------------
RUN_SIZES = (1, 256, 257, 8192, 8193, 32768, 32769)
RUN_SHAPES = ("each", "one", "cut")
RUN_CUTS = (255, 256, 257, 8191, 8192, 8193, 32767, 32768)   # rows a head stands on in shape "cut", where n reaches them
_FILL = 97                                                  # filler genes per taxon


def run_shape_starts(n, shape):
    """first row of every run: "each" -- every row its own query; "one" -- all rows one query; "cut" -- heads on row 0 and on RUN_CUTS"""
    if shape == "each":
        return np.arange(n, dtype=np.int64)
    if shape == "one":
        return np.zeros(1, dtype=np.int64)
    return np.array([0] + [c for c in RUN_CUTS if c < n], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def run_shape_case(n, shape):
    """(columns, fasta, run starts, numpy pairs, {-r value: numpy table}) of n rows in runs of the given shape: computed once, shared,
    left unchanged.  Run r asks as ta|q<r> (r even) or tb|q<r> (r odd); runs 2k and 2k + 1 are partners: each holds the other's query
    in its middle row with the largest score of the run, so they are a reciprocal best hit and ta|q<2k> a core gene.  Every other row
    holds a filler gene of ta, tb or tc with a score of 1 .. 50 that repeats inside a long run (ties: the first row wins).  A run without
    a partner (the last of an odd number, and the only run of shape "one") still has a winner per foreign taxon -- a core gene when it
    asks as ta -- but no pair: one run proposes every key once."""
    from swiftortho_amd import find_orth, rbh
    starts = run_shape_starts(n, shape)
    nruns = len(starts)
    rid = np.searchsorted(starts, np.arange(n), side="right") - 1
    j = np.arange(n) - starts[rid]
    length = np.diff(np.concatenate([starts, [n]]))[rid]
    partner = rid ^ 1
    at_partner = (j == length // 2) & (partner < nruns)
    ids = [("t%s|q%05d" % ("ab"[r & 1], r)).encode() for r in range(nruns)] + [("t%s|f%03d" % (t, g)).encode() for t in "abc" for g in range(_FILL)]
    names, code = np.unique(np.array(ids), return_inverse=True)
    filler = nruns + (rid * 7 + j * 3) % (3 * _FILL)
    s = code[np.where(at_partner, partner, filler)].astype(np.int64)
    score = np.where(at_partner, 1000., 1. + (rid * 13 + j * 31) % 50).astype(np.float64)
    one, hundred = np.ones(n), np.full(n, 100.)
    cols = find_orth.HitColumns(names, code[rid].astype(np.int64), s, hundred, hundred, one, hundred, score, hundred)
    fasta = dummy_fasta([i.decode() for i in ids])
    return cols, fasta, starts, rbh.reciprocal_best_hits(cols), {r: rbh.core_table(cols, fasta, r) for r in ("ta", "tb")}
