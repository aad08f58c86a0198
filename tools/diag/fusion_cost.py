"""The gene-fusion stage in one warm process: so_fusion_cols (the whole device call, and its stages split by events: the row stages, the
sort of all rows' keys, the count pass, that pass once more -- only a timed call runs it: what coming first costs --, the emit pass, the
sort of the links) against the numpy definition swiftortho_amd/fusion.py
fusion_links(), on a table shaped like the records of an all-vs-all search of `proteins` proteins: every protein is one run; it has one
domain family or (15 %) two, family sizes are skewed (a few families of thousands), and a run holds about as many rows as its families
have members, 1000 at most (the wrapper's -v), drawn from them with repeats; a row covers the subject's domain, so a two-domain subject
is covered by half and a one-domain subject as a whole.
    python tools/diag/fusion_cost.py [proteins] [rows] [rounds] [sample_runs]
Defaults: 100000 proteins, about 1600000 rows, 9 rounds after a warm call; the definition is timed on the table of the first `sample_runs`
(20000) runs alone and scaled by the pairs of representatives -- its expansion is linear in them --, not run on all of them."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from swiftortho_amd import fusion

args = [int(x) for x in sys.argv[1:] if x.isdigit()]
NP = args[0] if args else 100000
ROWS = args[1] if len(args) > 1 else 1600000
rounds = args[2] if len(args) > 2 else 9
sample = min(args[3] if len(args) > 3 else 20000, NP)
TAXA, DOMAIN = 100, 150


def line(name, tt, note=""):
    tt = sorted(tt)
    print("%-52s min %9.3f ms  median %9.3f ms  (%d runs)  %s" % (name, tt[0], tt[len(tt) // 2], len(tt), note))
    sys.stdout.flush()


def table_of(n_proteins, n_rows, seed=5):
    rng = np.random.default_rng(seed)
    F = max(n_proteins // 20, 1)
    two = rng.random(n_proteins) < .15
    fam = np.stack([(F * rng.random(n_proteins) ** 6).astype(np.int64), (F * rng.random(n_proteins) ** 6).astype(np.int64)], axis=1)
    ndom = 1 + two.astype(np.int64)
    # the members of every family: (protein, which of its domains)
    prot = np.concatenate([np.arange(n_proteins), np.flatnonzero(two)])
    dom = np.concatenate([np.zeros(n_proteins, dtype=np.int64), np.ones(int(two.sum()), dtype=np.int64)])
    mfam = fam[prot, dom]
    order = np.argsort(mfam, kind="stable")
    prot, dom, mfam = prot[order], dom[order], mfam[order]
    fstart = np.searchsorted(mfam, np.arange(F + 1))
    fsize = np.diff(fstart)
    members = fsize[fam[:, 0]] + np.where(two, fsize[fam[:, 1]], 0)
    # run lengths with a heavy tail (Pareto, 1000 at most), the longest runs to the proteins of the largest families, none longer than
    # its families have members; the scale is bisected to n_rows
    raw, rank = np.sort(rng.pareto(1.1, n_proteins) + 1.), np.argsort(members, kind="stable")
    lengths = lambda scale: np.minimum(np.clip(np.rint(raw * scale), 1, 1000).astype(np.int64), np.maximum(members[rank], 1))
    lo, hi = 0., 1000.
    for _ in range(50):
        lo, hi = ((lo + hi) / 2, hi) if lengths((lo + hi) / 2).sum() < n_rows else (lo, (lo + hi) / 2)
    length = np.empty(n_proteins, dtype=np.int64)
    length[rank] = lengths(hi)
    q = np.repeat(np.arange(n_proteins), length)
    n = len(q)
    d = np.where(two[q], rng.integers(0, 2, n), 0)                    # the domain of the query this row aligns
    f = fam[q, d]
    pick = fstart[f] + (rng.random(n) * fsize[f]).astype(np.int64)
    s, e = prot[pick], dom[pick]
    jit = rng.integers(0, 8, (4, n))
    qst, qed = DOMAIN * d + 1 + jit[0], DOMAIN * (d + 1) - jit[1]
    sst, sed = DOMAIN * e + 1 + jit[2], DOMAIN * (e + 1) - jit[3]
    names = np.asarray([b"t%03d|p%07d" % (k % TAXA, k) for k in range(n_proteins)])
    order = np.argsort(names)                                         # name codes ascend with the ids
    code = np.empty(n_proteins, dtype=np.int64)
    code[order] = np.arange(n_proteins)
    tax = (np.arange(n_proteins) % TAXA)[order]
    return fusion.Table(names[order], code[q], code[s], qst, qed, sst, sed, DOMAIN * ndom[s], DOMAIN * ndom[q]), tax, length


def prefix(table, n):
    return fusion.Table(table.names, *(getattr(table, k)[:n] for k in ("q", "s", "qst", "qed", "sst", "sed", "slen", "qlen")))


table, tax, length = table_of(NP, ROWS)
print("%d proteins of %d taxa, %d rows in %d runs (longest %d, %d of 500 rows and more); coverage 7/10, max_overlap 0, same_taxon" %
      (NP, TAXA, len(table), NP, length.max(), int((length >= 500).sum())))

fusion.device_fusion_links(prefix(table, 8), tax)                     # warm-up: the library, the device, the code objects
fusion.device_fusion_links(table, tax)                                # a warm call on the input itself
wall, ev = [], []
for _ in range(rounds):
    st = {}
    t0 = time.time()
    links = fusion.device_fusion_links(table, tax, stats=st, timed=True)
    wall.append((time.time() - t0) * 1e3), ev.append(st)
line("so_fusion_cols (upload, stages, copy back)", wall, "%d links, %d waits; %s" % (len(links), st["waits"], links.counters()))
for k in ("prep_ms", "keys_ms", "count_ms", "count_again_ms", "emit_ms", "sort_ms"):
    line("  ... %s (events)" % k[:-3], [e[k] for e in ev])
best = min(e["count_ms"] for e in ev)
print("  the count pass: %.3e pairs, %.3e of them looked up twice, in %.3f ms = %.3e pairs / s" % (links.n_pairs, links.n_disjoint, best, links.n_pairs / (best * 1e-3)))

n_sub = int(length[:sample].sum())
sub = prefix(table, n_sub)
dev = fusion.device_fusion_links(sub, tax)
tt = []
for _ in range(3):
    t0 = time.time()
    want = fusion.fusion_links(sub, tax)
    tt.append((time.time() - t0) * 1e3)
scale = links.n_pairs / float(max(want.n_pairs, 1))
line("numpy: fusion_links on the first %d runs (%d rows)" % (sample, n_sub), tt,
     "%d pairs; x %.1f = %.1f s for all %d pairs (scaled by the pairs, not run)" % (want.n_pairs, scale, min(tt) * scale / 1e3, links.n_pairs))
same = np.array_equal(dev.row_a, want.row_a) and np.array_equal(dev.row_b, want.row_b) and dev.counters() == want.counters()
print("the device's links on those rows are the definition's: %s (%d links)" % (same, len(want)))
