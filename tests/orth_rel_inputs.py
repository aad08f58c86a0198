"""Inputs for the relations stage of find_orth (tests/test_orth_relations.py, tests/test_gpu_orth_relations.py): what lies behind the candidate
tables -- in-paralog normalisers, co-ortholog products, the repeat rule, the per-(block, taxon) normalisation.  The inputs of
tests/orth_inputs.py do not reach that stage's corners (no repeat survives, no pair occurs more than twice, no taxon has more than 64 forward
in-paralog pairs, taxon codes ascend with the names), so this module builds a CLIQUE family that does, small hand-made edge inputs, and a
plain-Python restatement of the stage (dictionaries and loops, nothing shared with the numpy code or the kernels)."""
import numpy as np

import orth_inputs as oi
from swiftortho_amd import find_orth as fo

# The stage has no size tiers: one wave per group walks it ORTH_WAVE_ROWS (csrc/tune.h; mirrored in orth_inputs, which
# test_orth_candidates.py checks against the header) rows at a time, whatever its length.  That chunk is the only bound it has: a (block, taxon)
# group of the OT section of clique(k) holds k rows, so k = bound - 1, bound, bound + 1 ends the chunk loop on 63 rows, a full chunk, one row.
CLIQUE_KS = (2, 3, 12, 15, 16, 17, 31, 32, 33)   # k(k-1)/2 forward pairs per taxon: 66 at 12 (a chunk and two rows), 120 / 136 at 16 / 17; k*k products per pair
BOUND_KS = (oi.ORTH_WAVE_ROWS - 1, oi.ORTH_WAVE_ROWS, oi.ORTH_WAVE_ROWS + 1)
CLIQUE_TAXA = (b"ab", b"ab-c", b"ac")             # in byte order the NAMES go ab-c|.., ab|.., ac|..: taxon codes 1, 0, 2
FLAGS = {"no": (.5, 0., "no"), "bal": (.5, 0., "bal")}


def clique(k, norm="no"):
    """-> HitColumns.  Three taxa of k genes.  Inside a taxon every gene hits every other (both ways) above every cross score: k - 1 in-paralogs
    each.  Gene i of one taxon and gene i of another hit each other with the best score either has in that taxon: 3k ortholog pairs.  Every
    other cross pair hits lower: co-ortholog candidates, which every ortholog pair of the same two taxa reaches through its k x k products --
    so each occurs k times in a block.  Taxon y: three genes, in-paralogs only (normaliser = mean over all).  Taxon z (not under bsr, where
    0 / 0 would be a NaN): two genes whose only hits are each other, score 0 -- normaliser 0, no IP row.  Scores are no small integers and
    alignment lengths vary: the order of a sum shows in its last bits."""
    names, rows = [], []
    gene = lambda t, i: CLIQUE_TAXA[t] + b"|g%03d" % i
    aln = lambda q, s: 80. + (hash_mix(q, s) % 37)
    row = lambda q, s, bit: (q, s, 90., aln(q, s), 1., 100., bit, 100.)
    for t in range(3):
        names += [gene(t, i) for i in range(k)]
    for t in range(3):
        for i in range(k):
            q = gene(t, i)
            for j in range(k):
                if j != i:
                    rows.append(row(q, gene(t, j), 500.3 + .7 * ((min(i, j) * 7 + max(i, j) * 3 + t) % 11) + (.01 if i < j else 0.)))
            for u in range(3):
                if u == t:
                    continue
                for j in range(k):
                    if j == i:
                        rows.append(row(q, gene(u, j), 300.1 + 1.3 * ((i * 5 + t + u) % 7)))
                    else:
                        lo, hi = (i, j) if t < u else (j, i)
                        rows.append(row(q, gene(u, j), 100.7 + .9 * ((lo * 11 + hi * 5 + t * u) % 13) + (.3 if t < u else 0.)))
    ys = [b"y|1", b"y|2", b"y|3"]
    names += ys
    for a in range(3):
        for b in range(3):
            if a != b:
                rows.append(row(ys[a], ys[b], 210.9 + 3.1 * (a + b)))
    if norm != "bsr":
        names += [b"z|1", b"z|2"]
        rows += [row(b"z|1", b"z|2", 0.), row(b"z|2", b"z|1", 0.)]
    return oi.columns(names, rows)


def hash_mix(q, s):
    h = 0
    for c in q + b"/" + s:
        h = (h * 131 + c) % 1000003
    return h


def edge_inputs():
    """name -> HitColumns: ortholog pairs whose first gene alone has in-paralogs, whose second alone has, and none of which has (while the
    in-paralog, co-candidate and ortholog tables are all non-empty, so the co-ortholog stage runs and finds no product)"""
    names = [b"a|1", b"a|2", b"b|1", b"b|2", b"c|1", b"c|2"]
    both = lambda q, s, bit: [(q, s, 90., 100., 1., 100., bit, 100.), (s, q, 90., 100., 1., 100., bit, 100.)]
    cols = lambda rows: oi.columns(names, sorted(rows, key=lambda r: r[0]))   # (one run per query)
    out = {}
    #   a|1 - b|1 and a|2 - b|2 are orthologs, a|1 - a|2 in-paralogs, a|2 - b|1 a co-ortholog candidate: nq = 1, ns = 0
    out["nq_only"] = cols(both(b"a|1", b"b|1", 100.5) + both(b"a|1", b"a|2", 120.25) + both(b"a|2", b"b|2", 90.5) + both(b"a|2", b"b|1", 80.1))
    out["ns_only"] = cols(both(b"a|1", b"b|1", 100.5) + both(b"b|1", b"b|2", 120.25) + both(b"a|2", b"b|2", 90.5) + both(b"a|1", b"b|2", 80.1))
    out["both_zero"] = cols(both(b"a|1", b"b|1", 100.5) + both(b"c|1", b"c|2", 120.25) + both(b"a|1", b"b|2", 80.1))
    return out


# ---------------------------------------------------------------------------------------------------------
# the stage in plain Python
# ---------------------------------------------------------------------------------------------------------
def reference(names, tax, cand, reverse=False):
    """Candidates -> dict ip / ot / co: lists of (a, b, value), plus what the tests assert about the input: avg (taxon -> in-paralog normaliser),
    means ((section, block, taxon) -> mean), products (per ortholog pair that expands), kept / dropped (repeats that survived / went) and
    max_occ (most occurrences of one pair in a block).  reverse: every float sum adds its rows in the opposite order"""
    out = dict(ip=[], ot=[], co=[], avg={}, means={}, products=[], kept=0, dropped=0, max_occ=0, blocks={})
    if cand.n_rows == 0:
        return out
    M = max(len(names), 1)
    tax = [int(t) for t in tax]
    ot = list(zip(cand.ot_a.tolist(), cand.ot_b.tolist(), cand.ot_s.tolist()))
    ip = list(zip(cand.ip_a.tolist(), cand.ip_b.tolist(), cand.ip_s.tolist()))
    co = dict(zip(cand.co_key.tolist(), cand.co_best.tolist()))
    chain = lambda xs: _chain(xs[::-1] if reverse else xs)
    has_ot = set(a for a, _, _ in ot) | set(b for _, b, _ in ot)
    per = {}
    for a, b, s in ip:
        if a < b:
            e = per.setdefault(tax[a], ([], []))
            e[0].append(s)
            if a in has_ot or b in has_ot:
                e[1].append(s)
    for t, (al, nr) in per.items():
        out["avg"][t] = chain(nr) / len(nr) if nr else chain(al) / max(len(al), 1)
    out["ip"] = [(a, b, s / out["avg"][tax[a]]) for a, b, s in ip if a < b and out["avg"][tax[a]] != 0]
    partners = {}
    for a, b, _ in ip:
        partners.setdefault(a, []).append(b)
    co_rows = []
    if ip and co and ot:
        for a, b, _ in ot:
            pa, pb = partners.get(a, []), partners.get(b, [])
            if not pa and not pb:
                continue
            out["products"].append((len(pa) + 1) * (len(pb) + 1))
            for x in pa + [a]:
                for y in pb + [b]:
                    if x * M + y in co:
                        co_rows.append((x, y, co[x * M + y]))
    for kind, rows in (("ot", ot), ("co", co_rows)):
        i, blk = 0, 0
        while i < len(rows):
            j = i
            while j < len(rows) and tax[rows[j][0]] == tax[rows[i][0]]:
                j += 1
            seen, kept = {}, []
            first = rows[i][:2]
            for a, b, s in rows[i:j]:
                c = seen.get((a, b), 0)
                seen[(a, b)] = c + 1
                if c == 0 or (c == 1 and (a, b) == first):
                    kept.append((a, b, s))
                    out["kept"] += c == 1
                else:
                    out["dropped"] += 1
            out["max_occ"] = max([out["max_occ"]] + list(seen.values()))
            groups = {}
            for a, b, s in kept:
                groups.setdefault(tax[b], []).append(s)
            for t, g in groups.items():
                out["means"][(kind, blk, t)] = chain(g) / float(len(g))
            out[kind] += [(a, b, s / out["means"][(kind, blk, tax[b])]) for a, b, s in kept]
            i, blk = j, blk + 1
        out["blocks"][kind] = blk
    return out


def _chain(xs):
    acc = 0.
    for x in xs:
        acc = acc + x
    return acc


def as_lists(tables):
    """RelationTables -> the comparable form reference() uses"""
    z = lambda k: list(zip(getattr(tables, k + "_a").tolist(), getattr(tables, k + "_b").tolist(), getattr(tables, k + "_v").tolist()))
    return dict(ip=z("ip"), ot=z("ot"), co=z("co"))


def same_tables(x, y):
    """two RelationTables: every array equal, float64 arrays bit for bit, and the counters"""
    for k in fo.RelationTables.FIELDS:
        a, b = getattr(x, k), getattr(y, k)
        if a.dtype != b.dtype or a.shape != b.shape:
            return "%s: dtype / shape %s %s vs %s %s" % (k, a.dtype, a.shape, b.dtype, b.shape)
        if not np.array_equal(a.view(np.int64), b.view(np.int64)):
            return "%s differs" % k
    for k in ("n_rows", "n_runs", "n_groups"):
        if getattr(x, k) != getattr(y, k):
            return "%s: %d vs %d" % (k, getattr(x, k), getattr(y, k))
    return ""


def numpy_tables(cols, coverage=.5, identity=0., norm="no", sep="|"):
    cand = fo.candidates(cols, coverage, identity, norm, sep)
    return fo.relation_tables(cols.names, cand.tax, cand.taxa, cand)
