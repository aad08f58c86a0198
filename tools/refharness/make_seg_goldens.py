"""SEG query masks of the REAL reference at every edge of the mask kernels (container only).

    python tools/refharness/make_seg_goldens.py

Writes tests/golden/seg_edges.json: input strings and the first value of the reference's seg() for them, nothing else.  The
run is deterministic (own generators, seeded per case) and reproduces the committed file byte for byte.  make_goldens.py and
kat.json are left alone: their random stream must not move.

Inputs are MOSAICS: segments of 3-39 residues, each of a kind drawn at random -- iid over the 20 amino acids, iid over a random
2-7 letter sub-alphabet (which straddles the 2.2-bit threshold of the 12-residue window), a homopolymer, a tandem repeat of
period 2-6 -- concatenated and cut to the wanted length.  The "odd" variant of a length puts two bytes of ODD into about a fifth
of its segments.  ASCII only: the loader runs the reference under Python 3, whose upper() differs from the translated binary's
at 0x80 and above.

The lengths sit at the edges of csrc/k_prep.hip's k_seg: the first window (n < 12) and the tail rule mask[n-12:], one / two / three
tiles of the sliding steps 1 .. n-12 for the instances with 128- and 512-step tiles, and the lengths at which a query moves to the
next instance (1024, 4096, 32768).  alphabet64 / alphabet65: five queries that hold exactly 64 / 65 distinct upper-cased bytes
between them, the boundary between the device kernel and the host's seg_mask.

An output byte is the upper-cased input byte or 'x', so outputs above VERBATIM_MAX residues are stored as run lengths (unmasked,
masked, unmasked, ...; the first may be 0) with the SHA-1 of the whole string; shorter ones verbatim.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import refload  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
AA = "ACDEFGHIKLMNPQRSTVWY"
ODD = "-*.UJOBZxXak"
VERBATIM_MAX = 300

LENGTHS = {
    "first_window_and_tail": [1, 2, 11, 12, 13, 14, 23, 24, 25, 75, 76, 77],
    "small_tiles": [139, 140, 141, 268, 269],
    "small_mid_boundary": [1023, 1024, 1025],
    "mid_tiles": [1035, 1036, 1037, 1547, 1548, 1549],
    "mid_giant_boundary_and_giant_tiles": [4095, 4096, 4097, 4107, 4108, 4109, 4620, 4621],
}
LENGTHS_PLAIN_ONLY = {"giant_unstaged_boundary_and_unstaged_tile": [32767, 32768, 32769, 33293]}
MIN_MASKED_SHARE = 0.25
INNER_EDGE_FROM = 75


def segment(rng, odd):
    n = int(rng.integers(3, 40))
    kind = int(rng.integers(0, 4))
    if kind == 0:
        s = [AA[i] for i in rng.integers(0, 20, n)]
    elif kind == 1:
        sub = rng.choice(20, int(rng.integers(2, 8)), replace=False)
        s = [AA[sub[i]] for i in rng.integers(0, len(sub), n)]
    elif kind == 2:
        s = [AA[int(rng.integers(0, 20))]] * n
    else:
        unit = [AA[i] for i in rng.integers(0, 20, int(rng.integers(2, 7)))]
        s = (unit * (n // len(unit) + 1))[:n]
    if odd and rng.random() < 0.2:
        for p in rng.integers(0, n, 2):
            s[int(p)] = ODD[int(rng.integers(0, len(ODD)))]
    return "".join(s)


def mosaic(n, odd, seed):
    rng = np.random.default_rng(seed)
    out, have = [], 0
    while have < n:
        out.append(segment(rng, odd))
        have += len(out[-1])
    return "".join(out)[:n]


def runs_of(out):
    """alternating run lengths of unmasked / masked ('x') bytes, starting with the unmasked run (0 if the string opens masked)"""
    runs, cur, k = [], False, 0
    for ch in out:
        if (ch == "x") != cur:
            runs.append(k)
            cur, k = not cur, 0
        k += 1
    runs.append(k)
    return runs


def inner_edges(out):
    return sum((out[i] == "x") != (out[i - 1] == "x") for i in range(1, len(out)))


def encode(name, group, s, out, **extra):
    assert len(out) == len(s) and all(o == "x" or o == c.upper() for c, o in zip(s, out)), name
    d = dict(name=name, group=group, n=len(s), **extra)
    d["in"] = s
    if len(s) <= VERBATIM_MAX:
        d["out"] = out
    else:
        d["runs"] = runs_of(out)
        d["sha1"] = hashlib.sha1(out.encode("ascii")).hexdigest()
    return d


def draw_mosaic(m, n, odd):
    """the first seed whose sequence keeps the promise: from INNER_EDGE_FROM residues on, a mask edge strictly inside"""
    seed = 1000003 * n + (500009 if odd else 0)
    while True:
        s = mosaic(n, odd, seed)
        out = m.seg(s)[0]
        if n < INNER_EDGE_FROM or inner_edges(out) > 0:
            return s, out, seed
        seed += 1


def alphabet_group(m, nsym, seed0):
    """five queries of 60-300 residues with low-complexity islands, exactly `nsym` distinct upper-cased bytes between them:
    printable ASCII without '>' and blanks"""
    pool = [chr(b) for b in range(33, 127) if chr(b) != ">" and not ("a" <= chr(b) <= "z")]   # 67 distinct upper-cased values
    assert len(pool) >= nsym
    seed = seed0
    while True:
        rng = np.random.default_rng(seed)
        syms = [pool[i] for i in rng.permutation(len(pool))[:nsym]]
        seqs = []
        for k, n in enumerate(int(x) for x in rng.integers(60, 301, 5)):
            mine = syms[k::5]
            s = []
            while len(s) < n:
                kind = int(rng.integers(0, 3))
                ln = int(rng.integers(8, 36))
                if kind == 0:     # every symbol of this query's share, shuffled, some in lower case
                    seg_ = [mine[i] for i in rng.permutation(len(mine))]
                    seg_ = [c.lower() if rng.random() < 0.3 else c for c in seg_]
                elif kind == 1:
                    seg_ = [mine[int(rng.integers(0, len(mine)))]] * ln
                else:
                    unit = [mine[i] for i in rng.integers(0, len(mine), int(rng.integers(2, 4)))]
                    seg_ = (unit * ln)[:ln]
                s += seg_
            seqs.append("".join(s[:n]))
        outs = [m.seg(s)[0] for s in seqs]
        distinct = len(set("".join(seqs).upper()))
        if distinct == nsym and all(inner_edges(o) > 0 for s, o in zip(seqs, outs) if len(s) >= INNER_EDGE_FROM):
            return seqs, outs, seed
        seed += 1


def main():
    m = refload.load()
    cases = []
    for group, lens in list(LENGTHS.items()) + list(LENGTHS_PLAIN_ONLY.items()):
        for n in lens:
            for odd in ((False,) if group in LENGTHS_PLAIN_ONLY else (False, True)):
                s, out, seed = draw_mosaic(m, n, odd)
                cases.append(encode("%s_%d" % ("odd" if odd else "plain", n), group, s, out, odd=odd, seed=seed))
    for nsym, seed0 in ((64, 64000), (65, 65000)):
        seqs, outs, seed = alphabet_group(m, nsym, seed0)
        assert len(set("".join(seqs).upper())) == nsym
        for k, (s, out) in enumerate(zip(seqs, outs)):
            cases.append(encode("alphabet%d_%d" % (nsym, k), "alphabet%d" % nsym, s, out, odd=True, seed=seed))
    outs = {c["name"]: m.seg(c["in"])[0] for c in cases}
    total = sum(c["n"] for c in cases)
    masked = sum(o.count("x") for o in outs.values())
    edges = sum(inner_edges(o) for o in outs.values())
    assert masked >= MIN_MASKED_SHARE * total, (masked, total)
    assert all(inner_edges(outs[c["name"]]) > 0 for c in cases if c["n"] >= INNER_EDGE_FROM)
    assert all(ord(ch) < 128 for c in cases for ch in c["in"])
    doc = {"about": "inputs and first return value of the reference's seg() (lib/fsearch.py), tools/refharness/make_seg_goldens.py",
           "lengths": LENGTHS, "lengths_plain_only": LENGTHS_PLAIN_ONLY, "verbatim_max": VERBATIM_MAX,
           "min_masked_share": MIN_MASKED_SHARE, "inner_edge_from": INNER_EDGE_FROM,
           "residues": total, "masked": masked, "inner_edges": edges, "cases": cases}
    path = os.path.join(GOLD, "seg_edges.json")
    with open(path, "w", newline="\n") as f:
        f.write(json.dumps(doc, separators=(",", ":"), sort_keys=False).replace('},{"name"', '},\n{"name"') + "\n")
    print("seg_edges.json: %d cases, %d residues, %d masked (%.1f %%), %d inner edges, %d bytes"
          % (len(cases), total, masked, 100.0 * masked / total, edges, os.path.getsize(path)))


if __name__ == "__main__":
    main()
