"""The shared device primitives, called directly (so_prim_*, swiftortho_amd/prim.py -> csrc/prim.hip -> the wrappers of csrc/kernels.h the
stages call) on the inputs of tests/prim_inputs.py against their numpy definitions: exact integer equality throughout, device memory
poisoned, every call twice in one process.  The scans at every tile and path edge, misaligned ranges with the words around them
watched, wrapping sums; effscan's packed pair; run heads of 64-bit and negative keys; the numbering across the scan's path switch; the
library sorts across their algorithms, bit ranges, dispatch thresholds and segment classes, with the path / tier / variant each case
reports equal to what its name claims (tests/test_prim_inputs.py).

Run on the GPU box:  python -m pytest tests/test_gpu_prim.py -m gpu -q
"""
import numpy as np
import pytest

import prim_inputs as pi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prim():
    from swiftortho_amd import prim
    return prim


@pytest.fixture(autouse=True)
def poisoned(monkeypatch):
    monkeypatch.setenv("SOHIT_POISON", "165")


def same(a, b):
    return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def twice(call):
    """the result of call(), which a second call() repeats word for word"""
    first, second = call(), call()
    assert same(first, second), "the second call differs from the first"
    return first


def untouched(prim, *guards):
    return all((g == prim.SENTINEL).all() for g in guards)


# ---- scan ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", pi.SCAN_SIZES)
def test_scan(prim, n):
    for kind in pi.SCAN_KINDS:
        v = pi.scan_values(n, kind)
        for inclusive in (False, True):
            want, total = pi.scan_ref(v, inclusive)
            for in_place in (False, True):
                r = twice(lambda: prim.scan(v, inclusive, in_place))
                what = (n, kind, inclusive, in_place)
                assert (r.path, r.tiles) == pi.scan_path(n), what
                assert np.array_equal(r.out, want), what
                assert r.total == total, what
                assert untouched(prim, r.before, r.after), what


@pytest.mark.parametrize("n", pi.SKEW_SIZES)
def test_scan_at_every_skew(prim, n):
    v = pi.scan_values(n, "full")
    for inclusive in (False, True):
        want, total = pi.scan_ref(v, inclusive)
        for si in range(4):
            for so in range(4):
                for in_place in ((False, True) if si == so else (False,)):
                    r = twice(lambda: prim.scan(v, inclusive, in_place, si, so))
                    what = (n, inclusive, si, so, in_place)
                    assert np.array_equal(r.out, want) and r.total == total, what
                    assert untouched(prim, r.before, r.after), what
                    assert (r.path, r.tiles) == pi.scan_path(n)


# ---- effscan --------------------------------------------------------------------------------------------------------------------------
def check_effscan(prim, mark, scnt, mark_skew=0, scnt_skew=0):
    hoff, cidx, hits, seeds = pi.effscan_ref(mark, scnt)
    r = twice(lambda: prim.effscan(mark, scnt, mark_skew, scnt_skew))
    what = (len(mark), mark_skew, scnt_skew)
    assert np.array_equal(r.hoff, hoff), what
    assert np.array_equal(r.cidx, cidx), what
    assert (r.hits, r.seeds) == (hits, seeds), what
    assert untouched(prim, r.guards), what
    assert r.tiles == pi.scan_path(len(mark))[1]


@pytest.mark.parametrize("n", pi.EFF_SIZES)
def test_effscan(prim, n):
    check_effscan(prim, *pi.eff_case(n))


@pytest.mark.parametrize("n", pi.EFF_SKEW_SIZES)
def test_effscan_at_every_skew(prim, n):
    mark, scnt = pi.eff_case(n)
    for mark_skew in range(4):
        for scnt_skew in range(4):
            check_effscan(prim, mark, scnt, mark_skew, scnt_skew)


def test_effscan_near_overflow(prim):
    """hits two words short of 2^32 ... must not carry into the count of non-empty seeds that shares their 64-bit value"""
    for mark_skew in (0, 3):
        check_effscan(prim, *pi.eff_near_overflow(), mark_skew=mark_skew)


# ---- runs -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pi.run_cases()))
def test_runs(prim, name):
    keys = pi.run_cases()[name]
    head, rid, start = pi.runs_ref(keys)
    r = twice(lambda: prim.runs(keys))
    assert np.array_equal(r.head, head) and np.array_equal(r.rid, rid)
    assert r.n_runs == len(start) - 1
    assert np.array_equal(r.start[:len(start)], start)                       # ... the closing word included
    assert (r.start[len(start):] == prim.SENTINEL).all()                     # and nothing behind it


# ---- numbering ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pi.number_cases()))
def test_number_by_first_appearance(prim, name):
    cx, cy, n_codes = pi.number_cases()[name]
    X, Y, gene_code, first, flag = pi.number_ref(cx, cy, n_codes)
    r = twice(lambda: prim.number(cx, cy, n_codes))
    assert r.n_genes == len(gene_code)
    assert np.array_equal(r.X, X) and np.array_equal(r.Y, Y)
    assert np.array_equal(r.gene_code[:r.n_genes], gene_code) and (r.gene_code[r.n_genes:] == -1).all()
    assert np.array_equal(r.first, first) and np.array_equal(r.flag, flag)


# ---- device-wide sorts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", pi.WIDE_BITS)
@pytest.mark.parametrize("n", pi.WIDE_SIZES)
def test_device_wide_sorts(prim, n, bits):
    """the low `bits` sorted, the random bits above riding along, values = original positions: the stable order and nothing else"""
    keys, order = pi.wide_keys(n, 0, bits), pi.wide_order(n, 0, bits)
    want = keys[order]
    for kind, vt in ((prim.SORT_KEYS, None), (prim.SORT_PAIRS32, np.uint32), (prim.SORT_PAIRS64, np.uint64)):
        values = None if vt is None else np.arange(n, dtype=vt)
        r = twice(lambda: prim.sort(kind, keys, 0, bits, values))
        what = (kind, n, bits)
        assert r.tier == pi.sort_tier(n) and r.variant == -1, what
        assert r.temp_bytes > 0 and r.temp_overrun == 0, what
        assert np.array_equal(r.keys, want), what
        if vt is not None:
            assert np.array_equal(r.values, order.astype(vt)), what


@pytest.mark.parametrize("b0,b1", pi.WIDE_RANGES)
@pytest.mark.parametrize("n", pi.WIDE_RANGE_SIZES)
def test_sort_keys_from_a_begin_bit(prim, n, b0, b1):
    keys, order = pi.wide_keys(n, b0, b1), pi.wide_order(n, b0, b1)
    r = twice(lambda: prim.sort(prim.SORT_KEYS, keys, b0, b1))
    assert r.tier == pi.sort_tier(n, b0, b1) and r.temp_overrun == 0
    assert np.array_equal(r.keys, keys[order])


# ---- segmented sorts ------------------------------------------------------------------------------------------------------------------
SEG_RANGES = tuple((pi.SEG_B0, pi.SEG_B0 + w) for w in pi.SEG_WIDTHS) + (pi.SEG_B1_63,)


def check_seg_sort(prim, kind, lengths, b0, b1, descending=False):
    words = pi.seg_words(lengths, b0, b1)
    n, nseg = len(words), len(lengths)
    if kind == prim.SORT_SEG2:
        begins, ends = pi.gapped(lengths)
        r = twice(lambda: prim.sort(kind, words, b0, b1, seg_begin=begins, seg_end=ends))
    else:
        b = pi.bounds(lengths)
        begins, ends = b[:-1], b[1:]
        r = twice(lambda: prim.sort(kind, words, b0, b1, seg_begin=b))
    want = pi.seg_sort_ref(words, begins, ends, b0, b1, prim.SORT_FILL, descending)
    what = (kind, n, nseg, b0, b1)
    variant = pi.cand_cfg(n, nseg) if kind == prim.SORT_CAND else 0 if kind == prim.SORT_SEG_DESC else pi.seg_variant(n, nseg, b1 - b0)
    assert r.variant == variant and r.tier == -1, what
    assert r.temp_overrun == 0, what
    bad = np.flatnonzero(r.keys != want)
    assert len(bad) == 0, (what, "first of %d differing words at %d: %#x, want %#x" % (len(bad), bad[0], int(r.keys[bad[0]]), int(want[bad[0]])) if len(bad) else "")
    return r


@pytest.mark.parametrize("mix", sorted(pi.SEG_MIXES))
@pytest.mark.parametrize("kind", ("seg", "seg2"))
def test_segmented_sort(prim, kind, mix):
    """the field sorted inside every segment, ties in input order (the positions below the field), the segment numbers above it carried;
    seg2: the words between a segment's end and the next one's begin keep what the output held"""
    for b0, b1 in SEG_RANGES:
        check_seg_sort(prim, prim.SORT_SEG if kind == "seg" else prim.SORT_SEG2, pi.SEG_MIXES[mix], b0, b1)


@pytest.mark.parametrize("mix", sorted(pi.CAND_MIXES))
def test_candidate_sort(prim, mix):
    for b0, b1 in SEG_RANGES:
        check_seg_sort(prim, prim.SORT_CAND, pi.CAND_MIXES[mix], b0, b1)


@pytest.mark.parametrize("mix", sorted(pi.DESC_MIXES))
def test_descending_sort(prim, mix):
    """from bit 0, as order_chunk sorts: the keys; from a begin bit with the position below it: ties keep input order"""
    for b1 in pi.DESC_END_BITS:
        check_seg_sort(prim, prim.SORT_SEG_DESC, pi.DESC_MIXES[mix], 0, b1, descending=True)
    for b0, b1 in pi.DESC_TAGGED:
        check_seg_sort(prim, prim.SORT_SEG_DESC, pi.DESC_MIXES[mix], b0, b1, descending=True)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
SEG_KINDS = ("SORT_SEG", "SORT_SEG2", "SORT_CAND", "SORT_SEG_DESC")
ALL_KINDS = ("SORT_KEYS", "SORT_PAIRS32", "SORT_PAIRS64") + SEG_KINDS


def served(prim):
    """a valid call right after a refusal"""
    v = pi.scan_values(17, "small")
    assert np.array_equal(prim.scan(v).out, pi.scan_ref(v, False)[0])
    lengths = pi.SEG_MIXES["segs_63"]
    check_seg_sort(prim, prim.SORT_SEG, lengths, pi.SEG_B0, pi.SEG_B0 + 8)


@pytest.mark.parametrize("kind", SEG_KINDS)
def test_end_bit_64_is_refused(prim, kind):
    k = getattr(prim, kind)
    lengths = (3, 40, 0, 200)
    words = pi.seg_words(lengths, 40, 63)
    b = pi.bounds(lengths)
    seg = dict(seg_begin=b[:-1], seg_end=b[1:]) if k == prim.SORT_SEG2 else dict(seg_begin=b)
    with pytest.raises(RuntimeError, match="end_bit must be below 64"):
        prim.sort(k, words, 40, 64, **seg)
    served(prim)
    assert np.array_equal(prim.sort(k, words, 40, 63, **seg).keys,
                          pi.seg_sort_ref(words, b[:-1], b[1:], 40, 63, prim.SORT_FILL, k == prim.SORT_SEG_DESC))


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_two_to_the_31_keys_are_refused(prim, kind):
    """by the sort's *_temp_bytes, which the entry asks before it reads an array (none is given), and by the sort itself"""
    k = getattr(prim, kind)
    seg = {} if kind not in SEG_KINDS else dict(seg_begin=np.zeros(2, np.uint32), seg_end=np.zeros(2, np.uint32))
    for n in (1 << 31, (1 << 32) + 5):
        with pytest.raises(RuntimeError, match=r"_temp_bytes: 2\^31 keys and more are not served"):
            prim.sort(k, None, 0, 8, n=n, **seg)
        with pytest.raises(RuntimeError, match=r"sort_[a-z0-9_]+: 2\^31 keys and more are not served") as e:
            prim.sort(k | prim.WRAPPER_ONLY, None, 0, 8, n=n, **seg)
        assert "_temp_bytes" not in str(e.value)
    served(prim)


def test_bad_device_is_refused(prim):
    v = pi.scan_values(17, "small")
    mark, scnt = pi.eff_case(17)
    cx, cy, n_codes = pi.number_cases()["self_row_first"]
    for device in (-1, 99):
        for call in (lambda: prim.scan(v, device=device), lambda: prim.effscan(mark, scnt, device=device),
                     lambda: prim.runs(pi.run_cases()["n1_int"], device=device), lambda: prim.number(cx, cy, n_codes, device=device),
                     lambda: prim.sort(prim.SORT_KEYS, pi.wide_keys(2, 0, 8), 0, 8, device=device)):
            with pytest.raises(RuntimeError, match="device index out of range"):
                call()
            served(prim)
