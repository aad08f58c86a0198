"""Inputs of the operon tests (tests/test_operon.py, tests/test_gpu_operon.py) and of tools/refharness/make_operon_goldens.py.

GOLDEN_CASES: what the REAL scripts/operon_cluster.py was run on -- name -> input; an input is either the literal text of the two files
or the arguments of a generator, from which it is regenerated (only the arguments are stored in the fixture).
tests/golden/operon_<name>.json holds the script's standard output.
designed(): operon tables at the edges only the device kernels see (family lists around a wave and a workgroup, batches cut at, one
below and one above a budget, an operon larger than a budget, operons without an indexed family first, last and between two batches,
the filter's boundaries, rank ties), each with the budgets under which it must run in more than one batch.
"""
import functools
import json
import os
import random

import numpy as np

from conftest import GOLD


# ---------------------------------------------------------------------------------------------------------
# golden inputs
# ---------------------------------------------------------------------------------------------------------
def _gene(n):
    return 'g' + np.base_repr(n, 36).lower()


def synth(n_taxa, n_per, n_fam, n_common, seed, final_newline=True):
    """-> (groups text, operon text): every taxon holds n_per operons, each a copy of one of n_per templates over the n_common common
    families (family 0 among them) with genes lost, replaced from the tail of rare families, or unknown to the groups file"""
    rng = random.Random(seed)
    templates = [[rng.randrange(n_common) for _ in range(rng.randint(3, 6))] for _ in range(n_per)]
    members = [[] for _ in range(n_fam)]
    lines, n = [], 0
    for t in range(n_taxa):
        for k in range(n_per):
            fams = []
            for f in templates[k]:
                u = rng.random()
                if u < .15:
                    continue
                fams.append(rng.randrange(n_common, n_fam) if u < .3 else f)
            if not fams:
                fams = [rng.randrange(n_fam)]
            toks = []
            for f in fams:
                g, n = _gene(n), n + 1
                if rng.random() >= .1:
                    members[f].append(g)
                toks.append(g)
            lines.append(('-->' if rng.random() < .5 else '<--').join(toks) + '\t%d\t+' % t)
    groups = '\n'.join('\t'.join(m) for m in members) + ('\n' if final_newline else '')
    return groups, '\n'.join(lines) + ('\n' if final_newline else '')


def wrap(n_ops, n_clusters, stride):
    """-> (groups text, operon text): n_ops operons, every stride-th line of the file, hold a gene of family 1, so each has all of them
    as candidates: a set that resizes several times and whose members, spread over n_ops * stride numbers, wrap around its table.  Such an
    operon shares two more families with the ones n_clusters further alone, and only those pairs print; the lines between are single
    genes of no family"""
    members = [[] for _ in range(2 + 2 * n_clusters)]
    lines = []
    for k in range(n_ops):
        lines.extend('x%d' % (k * stride + m) for m in range(1, stride))
        c = k % n_clusters
        toks = ['a%d' % k, 'b%d' % k, 'c%d' % k]
        members[1].append(toks[0]), members[2 + 2 * c].append(toks[1]), members[3 + 2 * c].append(toks[2])
        lines.append('-->'.join(toks))
    members[0].append('nobody')
    return '\n'.join('\t'.join(m) for m in members) + '\n', '\n'.join(lines) + '\n'


BASE_GROUPS = 'z1\tz2\tz3\tz4\na1\ta2\ta3\ta4\nb1\tb2\tb3\tb4\nc1\tc2\tc3\tc4\nd1\td2\td3\td4\n'

GOLDEN_CASES = {
    'toy': {'groups': 't1|a\tt2|a\tt3|a\nt1|b\tt2|b\tt3|b\nt1|c\tt2|c\tt3|c\nt1|d\tt2|d\tt3|d\nt1|e\tt2|e\n',
            'operons': 't1|a-->t1|b-->t1|c-->t1|d\t+\nt2|d<--t2|c<--t2|b<--t2|a\t-\nt3|b-->t3|c-->t3|d\t+\nt1|e-->t1|x\t+\nt2|e\t-\nt3|a\n'},
    'taxa30': {'gen': dict(n_taxa=30, n_per=6, n_fam=40, n_common=8, seed=11)},
    'wrap600': {'wrap': dict(n_ops=600, n_clusters=200, stride=5)},
    # both separators: a string with '-->' is split there alone, its '<--' stays inside a token (an unknown gene)
    'mixed': {'groups': BASE_GROUPS, 'operons': 'a1-->b1-->c1\na2<--b2<--c2\na3-->b3<--c3-->d3\nd4<--c4-->b4-->a4\nb3<--c3\na1<--b1<--c1<--d1\n'},
    'header_mid': {'groups': BASE_GROUPS, 'operons': 'a1-->b1-->c1\tx\ngene_id\tstrand\na2-->b2-->c2\tx\ngene_id_a3-->b3-->c3\na4-->b4-->c4-->gene_id\n'},
    'no_newline': {'groups': BASE_GROUPS[:-1], 'operons': 'a1-->b1-->c1-->d4\na2-->b2-->c2-->d4\na3-->b3-->c3-->d\nd4-->d-->c4-->b4-->a4'},
    # b1 and c2 stand on two lines each: the later line owns them
    'two_fams': {'groups': BASE_GROUPS + 'b1\tc2\te1\te2\n', 'operons': 'a1-->b1-->c1-->e1\na2-->b2-->c2-->e2\na3-->b3-->c3\nb1-->c2-->e1-->a4\n'},
    # the empty groups line defines the gene '': empty tokens, and the empty operon string, belong to family 5
    'empty_tokens': {'groups': BASE_GROUPS + '\nf1\tf2\n', 'operons': 'a1-->-->b1-->c1\na2-->b2-->-->-->c2\n-->a3-->b3\n\n<--\na4<--b4<--\n-->\n'},
    'dups': {'groups': BASE_GROUPS, 'operons': 'a1-->b1-->c1\na1-->b1-->c1\na2-->b2-->c2-->d2\na1-->b1-->c1\na2-->b2-->c2-->d2\nd3\nd3\n'},
    # family 0 is never indexed but counts: pairs that reach N == 3 only through it, operons of family-0 genes alone, N == 2 without it
    'fam0': {'groups': BASE_GROUPS, 'operons': 'z1-->a1-->b1\nz2-->a2-->b2\nq-->a3-->b3\nz3-->z4\nz3\nz4-->a4-->b4-->c4-->d4-->x-->y\nz1-->a1-->b1-->c1-->d1-->x\n'
                                               'a2-->b2-->u-->v-->w\nz2-->z3-->a3\n'},
}


def case_texts(name):
    """-> (groups text, operon text)"""
    spec = GOLDEN_CASES[name]
    if 'gen' in spec:
        return synth(**spec['gen'])
    if 'wrap' in spec:
        return wrap(**spec['wrap'])
    return spec['groups'], spec['operons']


def golden_names():
    return sorted(GOLDEN_CASES)


@functools.lru_cache(maxsize=None)
def golden(name):
    """the fixture the REAL script left: dict with `input` (what it was made from) and `stdout`"""
    meta = json.load(open(os.path.join(GOLD, 'operon_%s.json' % name)))
    assert meta['input'] == GOLDEN_CASES[name], 'tests/golden/operon_%s.json was made from other arguments: rerun make_operon_goldens.py' % name
    return meta


# ---------------------------------------------------------------------------------------------------------
# designed operon tables
# ---------------------------------------------------------------------------------------------------------
BUDGETS = (None, 1, 7, 64, 1000)     # SOHIT_OPERON_EXPAND: unset and the values every table is run under


class Table:
    """the arrays of an OperonTable (no names)"""

    def __init__(self, ops, n_fam=None):
        """ops: [(families of the slice, length, has0)]"""
        self.start = np.concatenate(([0], np.cumsum([len(f) for f, _, _ in ops]))).astype(np.int64)
        self.fam = np.asarray([k for f, _, _ in ops for k in f], dtype=np.int32)
        self.length = np.asarray([l for _, l, _ in ops], dtype=np.int32)
        self.has0 = np.asarray([h for _, _, h in ops], dtype=np.uint8)
        self.n_fam = n_fam if n_fam is not None else int(self.fam.max()) + 1 if len(self.fam) else 1
        self.names = None

    @property
    def n_ops(self):
        return len(self.length)


def expansion_totals(t):
    """per operon the sum of its families' list lengths"""
    size = np.bincount(t.fam, minlength=t.n_fam)
    return [int(size[t.fam[a:b]].sum()) for a, b in zip(t.start[:-1], t.start[1:])]


def batch_totals(t, budget):
    """the batches rule restated: consecutive operons while the total stays within the budget (None: 2^28); an operon above it stays
    alone -> the expansions of every batch ([]: nothing is launched)"""
    if len(t.fam) == 0:
        return []
    budget = (1 << 28) if budget is None else budget
    out = [0]
    for k, x in enumerate(expansion_totals(t)):
        if k and out[-1] + x > budget:
            out.append(0)
        out[-1] += x
    return out


def expected_batches(t, budget):
    return len(batch_totals(t, budget))


def _private(m, nxt):
    """m families nobody else holds"""
    return list(range(nxt[0], nxt[0] + m)), nxt.__setitem__(0, nxt[0] + m)


def _lists():
    """families 1 .. 7 hold the first 1, 63, 64, 65, 255, 256, 257 operons; rotating families vary the shared count, the lengths put
    pairs on both sides of 2 * N == min(len); operon 0 alone expands beyond every test budget"""
    sizes = (1, 63, 64, 65, 255, 256, 257)
    ops = []
    for k in range(257):
        fams = [f + 1 for f, s in enumerate(sizes) if k < s] + [8 + k % 5, 13 + k % 3]
        if k % 2:
            fams.reverse()
        ops.append((fams, len(fams) + k % 4 + (k % 7 == 0) * 5, k % 3 == 0))
    return Table(ops)


def _exact():
    """only private families: an operon's total is its slice length.  3 + 4 hit the budget 7, 4 + 4 pass it by one; the operons up to the
    first 32 hit 64, 32 + 33 pass it by one; bare operons (no indexed family) first, last, where a batch ends full (it joins) and behind
    an operon larger than the budget (which stays alone)"""
    nxt = [1]
    ops = []
    for m in (0, 3, 4, 0, 4, 4, 0, 0, 17, 32, 0, 32, 33, 1, 0):
        ops.append((_private(m, nxt)[0], max(m, 1) + (m == 4), m % 2 == 0))
    return Table(ops)


def _edges():
    """N of 2 and 3 with and without family 0; 2 * N == min(len) and 2 * N == min(len) + 1"""
    ops = [([1, 2], 2, 0), ([2, 1], 2, 0),            # N = 2: never
           ([1, 2], 3, 1), ([1, 2], 3, 1),            # N = 3 through family 0, len 3: passes
           ([1, 2, 3], 6, 0), ([3, 2, 1], 6, 0),      # N = 3, 2 N == min(len): fails
           ([1, 2, 3], 5, 0), ([1, 2, 3], 9, 0),      # 2 N == min(len) + 1 against the pair above and each other
           ([4, 5], 4, 1), ([5, 4], 5, 1), ([4, 5], 5, 0),
           ([], 3, 1), ([6], 1, 0)]
    return Table(ops)


def _rank_ties():
    """operon 0 lists family 6 before family 5; 3 and 9 stand in both lists, 1 in the later one alone: first occurrence is 0 3 9 1 ..."""
    ops = [([6, 5], 2, 0), ([5], 1, 0), ([7], 1, 0), ([5, 6], 2, 0), ([7, 8], 2, 0), ([8, 7, 5], 3, 1), ([], 1, 0), ([9], 2, 0), ([9, 7], 2, 0), ([6, 5, 8], 3, 1)]
    return Table(ops)


def _random(n_ops, n_fam, seed):
    rng = np.random.RandomState(seed)
    w = 1. / np.arange(1, n_fam) ** 1.2
    ops = []
    for k in range(n_ops):
        m = rng.randint(0, 7)
        fams = rng.choice(np.arange(1, n_fam), size=min(m, n_fam - 1), replace=False, p=w / w.sum()).tolist()
        ops.append((fams, max(len(fams) + rng.randint(0, 3), 1), int(rng.rand() < .4)))
    return Table(ops, n_fam)


@functools.lru_cache(maxsize=None)
def designed():
    """-> {name: (Table, budgets under which more than one batch is called for)}"""
    return {
        'lists': (_lists(), (1, 7, 64, 1000)),
        'exact': (_exact(), (1, 7, 64)),
        'edges': (_edges(), (1, 7)),
        'rank_ties': (_rank_ties(), (1, 7)),
        'identical': (Table([([1, 2, 3, 4], 4, 0)] * 70), (1, 7, 64, 1000)),
        'none': (Table([]), ()),
        'one': (Table([([1, 2, 3], 3, 0)]), ()),
        'one_bare': (Table([([], 2, 1)]), ()),
        'bare': (Table([([], 1, 1), ([], 4, 0)], n_fam=3), ()),
        'random': (_random(150, 30, 3), (1, 7, 64, 1000)),
    }
