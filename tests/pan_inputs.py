"""Inputs of the pan-genome tests (tests/test_pan.py, tests/test_gpu_pan.py) and of tools/refharness/make_pan_goldens.py.

GOLDEN_CASES: what the REAL scripts/pan_genome.py was run on -- name -> (input, flags); an input is either literal text or the
arguments of synth(), from which it is regenerated (only the arguments are stored in the fixture).  tests/golden/pan_<name>.json holds
what the script printed and wrote: the taxon order of its `#family` line, the `# Number` line, the table text, the _xy.txt text.
designed(): member tables at the edges of the device kernels (rows around a 64-row tile, taxa around a word group, all-zero rows, a row
holding every taxon, counts above 1, with and without rows behind the file rows) under every threshold regime.
"""
import functools
import json
import os
import random

import numpy as np

from conftest import GOLD


def synth(n_taxa, n_groups, seed, n_single=5, desc=False, final_newline=True, paralogs=0.1):
    """-> (fasta text, groups text): taxa tx000 .., every group takes each taxon with a probability of its own (so that core, shared
    and specific families all occur), a second copy with probability `paralogs`; n_single genes stand in no group"""
    rng = random.Random(seed)
    genes, groups = [], []
    for g in range(n_groups):
        p = (0.03, 0.1, 0.3, 0.6, 0.9, 0.99)[int(rng.random() * 6)]
        grp = []
        for t in range(n_taxa):
            if rng.random() < p:
                for c in range(2 if rng.random() < paralogs else 1):
                    grp.append('tx%03d|g%04d_%d' % (t, g, c))
        if not grp:
            grp.append('tx%03d|g%04d_0' % (int(rng.random() * n_taxa), g))
        genes += grp
        groups.append(grp)
    genes += ['tx%03d|s%04d' % (int(rng.random() * n_taxa), k) for k in range(n_single)]
    order = sorted(range(len(genes)), key=lambda k: (rng.random(), k))
    fasta = ''.join('>%s%s\nMKV\n' % (genes[k], ' some description %d' % k if desc else '') for k in order)
    text = '\n'.join('\t'.join(g) for g in groups) + ('\n' if final_newline else '')
    return fasta, text


QUIRKS_FASTA = ('>a|1 first gene\nMK\n>a|2\nMK\n>b|1\nMK\n>b|2 x y\nMK\n>c|1\nMKL\nVV\n>c|2\nMK\n>a|3\nMK\n>c|3\nM\n>b|3\nM\n')
# a|1 twice in one group, b|1 in two groups, an empty-handed taxon per row, a|3 / c|3 / b|3 in no group
QUIRKS_GROUPS = 'a|1\ta|1\tb|1\tc|1\nb|1\tc|2\na|2\tb|2\n'

GOLDEN_CASES = {
    'default': ({'gen': dict(n_taxa=7, n_groups=40, seed=1)}, []),
    'frac': ({'gen': dict(n_taxa=9, n_groups=60, seed=2)}, ['-l', '.2', '-u', '.8']),
    'abs': ({'gen': dict(n_taxa=9, n_groups=60, seed=2)}, ['-l', '2', '-u', '5']),
    'l0': ({'gen': dict(n_taxa=7, n_groups=40, seed=3)}, ['-l', '0']),
    'u1': ({'gen': dict(n_taxa=7, n_groups=40, seed=3)}, ['-u', '1']),
    'rfile': ({'gen': dict(n_taxa=8, n_groups=50, seed=4), 'allow': 'tx001\n tx003 \ntx004\ntx006\nnobody\n'}, []),
    'quirks': ({'fasta': QUIRKS_FASTA, 'groups': QUIRKS_GROUPS}, []),
    'no_newline': ({'gen': dict(n_taxa=5, n_groups=12, seed=5, final_newline=False)}, []),
    'desc': ({'gen': dict(n_taxa=6, n_groups=30, seed=6, desc=True)}, ['-l.3', '-u.7']),
    'taxa2': ({'gen': dict(n_taxa=2, n_groups=25, seed=7)}, []),
    'taxa3': ({'gen': dict(n_taxa=3, n_groups=25, seed=8)}, []),
    # 0.07 * 100 > 7 and 0.29 * 100 < 29 in floats: core asks for 8 genomes and new for ys <= 27 at j = 100, where exact fractions give 7 and 28
    'float100': ({'gen': dict(n_taxa=100, n_groups=260, seed=9, n_single=20)}, ['-l.29', '-u.07']),
    'wide65': ({'gen': dict(n_taxa=65, n_groups=129, seed=10, n_single=0)}, []),
    # -u 0: Tc = 0 at every step, so every row is core, before any genome that holds it has come -- 75 rows, 11 of them in the last 64-row tile, whose other
    # 53 lanes must not count.  -l 1e12: S is the 32-bit clamp at every step, so every row a genome brings is new
    'u0': ({'gen': dict(n_taxa=7, n_groups=70, seed=11, n_single=5)}, ['-u', '0']),
    'l_huge': ({'gen': dict(n_taxa=7, n_groups=70, seed=11, n_single=5)}, ['-l', '1e12']),
}


def case_texts(name):
    """-> (fasta text, groups text, allow text or None, flags)"""
    spec, flags = GOLDEN_CASES[name]
    fasta, groups = synth(**spec['gen']) if 'gen' in spec else (spec['fasta'], spec['groups'])
    return fasta, groups, spec.get('allow'), list(flags)


def golden_names():
    return sorted(GOLDEN_CASES)


@functools.lru_cache(maxsize=None)
def golden(name):
    """the fixture the REAL script left: dict with taxa, number, table, xy (and the arguments it was made from)"""
    meta = json.load(open(os.path.join(GOLD, 'pan_%s.json' % name)))
    spec, flags = GOLDEN_CASES[name]
    assert meta['input'] == spec and meta['flags'] == list(flags), 'tests/golden/pan_%s.json was made from other arguments: rerun make_pan_goldens.py' % name
    return meta


def flag_values(flags):
    """-> (ts, tc) the flags ask for (defaults .05 / .95)"""
    ts, tc = .05, .95
    k = 0
    while k < len(flags):
        f = flags[k]
        if f in ('-l', '-u'):
            v = float(flags[k + 1])
            k += 1
        else:
            v = float(f[2:])
        ts, tc = (v, tc) if f[:2] == '-l' else (ts, v)
        k += 1
    return ts, tc


# ---------------------------------------------------------------------------------------------------------
# designed member tables
# ---------------------------------------------------------------------------------------------------------
REGIMES = {'default': (.05, .95), 'frac': (.3, .7), 'abs': (2., 5.), 'l0': (0., .95), 'u1': (.05, 1.), 'float': (.29, .07)}
# (file rows, rows behind them, taxa): a tile is 64 rows; taxa around one 64-word group and at 100 (where the float thresholds part)
SHAPES = [(1, 0, 2), (63, 0, 3), (64, 0, 63), (65, 0, 64), (129, 0, 65), (120, 9, 100), (1, 0, 1), (60, 5, 3), (0, 3, 4), (300, 40, 17)]


class Case:
    def __init__(self, row, taxon, n_rows, n_file_rows, n_taxa):
        self.row, self.taxon, self.n_rows, self.n_file_rows, self.n_taxa = row, taxon, n_rows, n_file_rows, n_taxa


@functools.lru_cache(maxsize=None)
def designed_table(n_file, n_behind, n_taxa, seed=0):
    """a member table: row 0 holds every taxon (when there is a file row), every 7th file row is all zero, counts reach 3, the rows
    behind the file rows hold one member each"""
    rng = np.random.RandomState(1000 * seed + n_file * 7 + n_taxa)
    row, tax = [], []
    for r in range(n_file):
        if r == 0:
            present = np.arange(n_taxa)
        elif r % 7 == 3:
            present = np.zeros(0, dtype=np.int64)
        else:
            p = (0.05, 0.3, 0.6, 0.95)[rng.randint(4)]
            present = np.flatnonzero(rng.rand(n_taxa) < p)
        for t in present.tolist():
            for _ in range(1 + (rng.rand() < 0.15) + (rng.rand() < 0.05)):
                row.append(r), tax.append(t)
    for k in range(n_behind):
        row.append(n_file + k), tax.append(int(rng.randint(n_taxa)))
    order = rng.permutation(len(row))     # (the pairs come in any order)
    return Case(np.asarray(row, dtype=np.int32)[order], np.asarray(tax, dtype=np.int32)[order], n_file + n_behind, n_file, n_taxa)


def designed():
    """-> [(id, Case, (ts, tc))]: every shape under the default regime, every regime on the shapes where it matters"""
    out = []
    for shape in SHAPES:
        for regime, (ts, tc) in sorted(REGIMES.items()):
            if regime == 'default' or shape in ((129, 0, 65), (120, 9, 100), (300, 40, 17)):
                out.append(('%dx%d+%d_%s' % (shape[0], shape[2], shape[1], regime), designed_table(*shape), (ts, tc)))
    return out
