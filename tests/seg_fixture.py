"""tests/golden/seg_edges.json (tools/refharness/make_seg_goldens.py): inputs and masks of the REAL reference's seg() at the edges
of the mask kernels.  Outputs above `verbatim_max` residues are stored as run lengths (unmasked, masked, ...) and a SHA-1: they are
rebuilt here from the upper-cased input, and the digest is checked before anything is compared with them."""
import hashlib
import json
import os

from conftest import GOLD

_CASES = None


def rebuild(c):
    """the expected bytes of one case"""
    if "out" in c:
        return c["out"].encode("ascii")
    up, out, p, masked = c["in"].encode("ascii").upper(), bytearray(), 0, False
    for k in c["runs"]:
        out += b"x" * k if masked else up[p:p + k]
        p, masked = p + k, not masked
    assert p == c["n"] and hashlib.sha1(bytes(out)).hexdigest() == c["sha1"], c["name"]
    return bytes(out)


def document():
    return json.load(open(os.path.join(GOLD, "seg_edges.json")))


def cases():
    """[(name, group, input bytes, expected bytes)] in file order, read once"""
    global _CASES
    if _CASES is None:
        _CASES = [(c["name"], c["group"], c["in"].encode("ascii"), rebuild(c)) for c in document()["cases"]]
    return _CASES


def inner_edges(out):
    return sum((out[i:i + 1] == b"x") != (out[i - 1:i] == b"x") for i in range(1, len(out)))


def fasta(seqs):
    return b"".join(b">q%d\n%s\n" % (i, s) for i, s in enumerate(seqs))


def first_difference(got, want):
    """None, or 'first differing position / length' text for an assertion message"""
    if got == want:
        return None
    if got is None:
        return "no masked query kept (wanted %d bytes)" % len(want)
    k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    return "first difference at %d of %d (got length %d): gpu %r  wanted %r" % (k, len(want), len(got), got[max(0, k - 12):k + 13], want[max(0, k - 12):k + 13])
