"""CPU-only: every named input of tests/prim_inputs.py has the property it is named for -- the scan's tile count and launch path, n / nseg
against the segmented sorts' dispatch thresholds, segment lengths and counts on both sides of the warp-sort classes, ties in every sorted
field, the near-overflow total, keys that differ only above bit 31 -- and the Python mirrors of the library's rules agree with what the
library itself reports (the so_prim_* calls that need no device)."""
import numpy as np
import pytest

import prim_inputs as pi


@pytest.fixture(scope="module")
def prim():
    from swiftortho_amd import build
    build.build(verbose=False)
    from swiftortho_amd import prim
    return prim


# ---- mirrors against the library ------------------------------------------------------------------------------------------------------
def test_scan_path_mirror(prim):
    edges = sorted(set(pi.SCAN_SIZES + pi.EFF_SIZES + pi.SKEW_SIZES + tuple(2 * nr for nr in pi.NUM_ROWS) + (pi.SCAN_TILE * pi.SCAN_SMALL_TILES + 1,)))
    for n in edges:
        assert prim.scan_path(n) == pi.scan_path(n), n


def test_sort_tier_mirror(prim):
    for kind in (prim.SORT_KEYS, prim.SORT_PAIRS32, prim.SORT_PAIRS64):
        for n in pi.WIDE_SIZES + (0, 3 * pi.MERGE_LIMIT):
            tier, single, limit = prim.sort_tier(kind, n)
            assert (tier, single, limit) == (pi.sort_tier(n), pi.SINGLE_BLOCK, pi.MERGE_LIMIT), (kind, n)


def test_variant_mirrors(prim):
    widths = pi.SEG_WIDTHS + (pi.SEG_B1_63[1] - pi.SEG_B1_63[0], 24, 26)
    for lengths in list(pi.SEG_MIXES.values()) + list(pi.CAND_MIXES.values()):
        n, nseg = sum(lengths), len(lengths)
        for w in widths:
            for kind in (prim.SORT_SEG, prim.SORT_SEG2):
                assert prim.seg_variant(kind, n, nseg, w) == pi.seg_variant(n, nseg, w)
            assert prim.seg_variant(prim.SORT_CAND, n, nseg, w) == pi.cand_cfg(n, nseg)
    assert prim.seg_variant(prim.SORT_SEG, 0, 0, 8) == 0 == prim.seg_variant(prim.SORT_CAND, 0, 0, 8)


# ---- scan ---------------------------------------------------------------------------------------------------------------------------
def test_scan_sizes_sit_on_the_edges():
    T, S = pi.SCAN_TILE, pi.SCAN_SMALL_TILES
    assert {0, 1, T - 1, T, T + 1, S * T - 1, S * T, S * T + 1, 5 * T + 1, 256 * T, 256 * T + 1, 257 * T + 3} <= set(pi.SCAN_SIZES)
    assert {2 * T - 1, 2 * T, 2 * T + 1} <= set(pi.SCAN_SIZES)                   # one step of the single launch: 16 K values
    path = {n: pi.scan_path(n) for n in pi.SCAN_SIZES}
    assert path[0] == ("none", 0) and path[S * T] == ("single", S) and path[S * T + 1] == ("three", S + 1) and path[5 * T + 1] == ("three", 6)
    # the block-sum kernel walks 256 tiles per pass: one pass, and a second one of one and of two tiles
    assert path[256 * T] == ("three", 256) and path[256 * T + 1] == ("three", 257) and path[257 * T + 3] == ("three", 258)
    assert {pi.scan_path(n)[0] for n in pi.SKEW_SIZES} == {"single", "three"} and all(n % 4 for n in pi.SKEW_SIZES)
    assert {n % 4 for n in pi.SCAN_SIZES} == {0, 1, 2, 3}


@pytest.mark.parametrize("n", (5, 40961))
def test_scan_values_and_definition(n):
    v = {k: pi.scan_values(n, k) for k in pi.SCAN_KINDS}
    assert v["small"].max() <= 7 and len(set(v["small"].tolist())) > 2
    assert (v["ones"] == 1).all() and (v["wrap"] == pi.M32).all()
    assert not v["last"][:-1].any() and v["last"][-1]
    assert v["full"].max() > 1 << 31
    ex, tot = pi.scan_ref(v["wrap"], False)
    inc, tot2 = pi.scan_ref(v["wrap"], True)
    assert tot == tot2 == (n * pi.M32) % (1 << 32) and int(v["wrap"].astype(np.uint64).sum()) > pi.M32      # it wraps
    assert ex[0] == 0 and ex.tolist()[:3] == [0, pi.M32, pi.M32 - 1] and inc.tolist()[:2] == [pi.M32, pi.M32 - 1]
    assert ((inc.astype(np.uint64) - ex) % (1 << 32) == v["wrap"]).all()
    assert pi.scan_ref(np.zeros(0, np.uint32), True)[1] == 0


# ---- effscan --------------------------------------------------------------------------------------------------------------------------
def test_effscan_inputs():
    T = pi.SCAN_TILE
    assert {1, 2, 3} <= {n % 4 for n in pi.EFF_SIZES if n < 8} and {1, 2, 3} <= {n % 4 for n in pi.EFF_SIZES if n > T}    # tails of 1, 2, 3 slots
    assert {T - 1, T, T + 1, 4 * T, 4 * T + 1, 5 * T + 1, 256 * T + 1} <= set(pi.EFF_SIZES)
    mark, scnt = pi.eff_case(40961)
    assert set(mark.tolist()) == set(pi.MARK_BYTES)
    words = mark[:40960].reshape(-1, 4)
    for b in range(4):      # every byte of a word holds 2 and 0x80 (on without bit 0) and sits alone among zeros
        assert {2, 0x80} <= set(words[:, b].tolist())
    assert ((mark != 0) & (scnt == 0)).any() and ((mark == 0) & (scnt != 0)).any()
    hoff, cidx, hits, seeds = pi.effscan_ref(mark, scnt)
    assert seeds == int(((mark != 0) & (scnt != 0)).sum()) < int((mark != 0).sum()) and hits == int(scnt[mark != 0].sum())
    assert all(n % 4 for n in pi.EFF_SKEW_SIZES) and {pi.scan_path(n)[1] > 1 for n in pi.EFF_SKEW_SIZES} == {False, True}


def test_effscan_near_overflow():
    mark, scnt = pi.eff_near_overflow()
    c = np.where(mark != 0, scnt, 0).astype(np.uint64)
    assert (1 << 32) - 64 <= int(c.sum()) < (1 << 32)
    assert int(scnt.astype(np.uint64).sum()) > (1 << 34)          # the counts under clear marks would wrap it many times
    per_tile = np.add.reduceat(c, np.arange(0, len(c), pi.SCAN_TILE))
    assert (per_tile > (1 << 24)).sum() >= 4                      # large partial sums in several tiles
    hoff, cidx, hits, seeds = pi.effscan_ref(mark, scnt)
    assert hits == (1 << 32) - 17 and seeds == int((c != 0).sum()) and int(hoff[-1]) + int(c[-1]) == hits


# ---- runs -----------------------------------------------------------------------------------------------------------------------------
def test_run_cases():
    c = pi.run_cases()
    for name, keys in c.items():
        assert keys.dtype == (np.int32 if "int" in name else np.uint64), name
    heads = lambda k: np.flatnonzero(pi.runs_ref(k)[0]).tolist()
    assert len(c["n1_int"]) == len(c["n1_u64"]) == 1
    for t in ("int", "u64"):
        assert heads(c["all_equal_" + t]) == [0] and heads(c["all_distinct_" + t]) == list(range(len(c["all_distinct_" + t])))
        assert heads(c["heads_" + t]) == [0] + list(pi.RUN_HEADS)
        assert pi.scan_path(len(c["all_equal_" + t]))[0] == "three"
    for name in ("u64_high_only", "u64_bit63_only", "int_negative"):
        assert set(pi.RUN_HEADS) < set(heads(c[name])), name
    k = c["u64_high_only"]
    assert len(set((k & np.uint64(pi.M32)).tolist())) == 1 and len(heads(k)) == len(pi.RUN_HEADS) + 4       # 32-bit compares see one run
    k = c["u64_bit63_only"]
    assert set((k[1:] ^ k[:-1]).tolist()) == {0, 1 << 63}
    assert c["int_negative"].max() < 0
    k = c["int_cross_zero"]
    assert k.min() == -(1 << 31) and k.max() == (1 << 31) - 1 and {-1, 0, 1} <= set(k.tolist())
    assert (k[1:] < k[:-1]).any()            # runs, not sorted keys: a key may come back
    head, rid, start = pi.runs_ref(k)
    assert rid[-1] == head.sum() == len(start) - 1 and start[-1] == len(k) and start[0] == 0


# ---- numbering ------------------------------------------------------------------------------------------------------------------------
def test_number_cases():
    c = pi.number_cases()
    assert [pi.scan_path(2 * nr) for nr in pi.NUM_ROWS] == [("single", 4), ("three", 5)] and 2 * pi.NUM_ROWS[0] == 32768 and 2 * pi.NUM_ROWS[1] == 32770
    for nr in pi.NUM_ROWS:
        cx, cy, n_codes = c["rows_%d" % nr]
        assert len(cx) == nr and cx[5] == cy[5] and cy[-1] not in set(cx.tolist()) | set(cy[:-1].tolist())
        X, Y, gene_code, first, flag = pi.number_ref(cx, cy, n_codes)
        assert X[5] == Y[5] and flag[10] == 1 and flag[11] == 0 and flag[-1] == 1 and Y[-1] == len(gene_code) - 1
        assert (first == pi.M32).any() and len(gene_code) == flag.sum() < min(n_codes, 2 * nr)
        assert gene_code[X].tolist() == cx.tolist() and gene_code[Y].tolist() == cy.tolist()
    cx, cy, n_codes = c["self_row_first"]
    assert [a.tolist() for a in pi.number_ref(cx, cy, n_codes)[:3]] == [[0, 0, 2], [0, 1, 0], [4, 1, 2]]
    cx, cy, n_codes = c["first_seen_as_cy"]
    X, Y, gene_code, first, flag = pi.number_ref(cx, cy, n_codes)
    assert gene_code.tolist() == [3, 8, 0, 9, 7] and first[8] == 1 and first[7] == 7 and first[0] == 2 and flag.tolist() == [1, 1, 1, 0, 1, 0, 0, 1]
    cx, cy, n_codes = c["far_codes"]
    assert n_codes > 100000 * len(set(cx.tolist()) | set(cy.tolist())) and max(cx.max(), cy.max()) == n_codes - 1 and min(cx.min(), cy.min()) == 0


# ---- device-wide sorts ----------------------------------------------------------------------------------------------------------------
def test_wide_sizes_cross_the_tiers():
    assert [pi.sort_tier(n) for n in pi.WIDE_SIZES] == [0, 0, 0, 1, 1, 2]
    assert {pi.sort_tier(n) for n in pi.WIDE_RANGE_SIZES} == {0, 1, 2} and {pi.SINGLE_BLOCK, pi.SINGLE_BLOCK + 1, pi.MERGE_LIMIT + 1} <= set(pi.WIDE_RANGE_SIZES)
    assert [pi.sort_tier(n, 20, 64) for n in pi.WIDE_RANGE_SIZES] == [0, 2, 2, 2] and [pi.sort_tier(n, 20, 63) for n in pi.WIDE_RANGE_SIZES] == [0, 1, 1, 2]
    assert {1, 8, 9, 32, 33, 63, 64} <= set(pi.WIDE_BITS) and all(b0 > 0 for b0, _ in pi.WIDE_RANGES) and any(b1 == 64 for _, b1 in pi.WIDE_RANGES)


@pytest.mark.parametrize("n", (2, 1025))
def test_wide_keys(n):
    for b0, b1 in [(0, b) for b in pi.WIDE_BITS] + list(pi.WIDE_RANGES):
        keys, order = pi.wide_keys(n, b0, b1), pi.wide_order(n, b0, b1)
        f = pi.field_of(keys, b0, b1)
        assert len(np.unique(f)) < n, (b0, b1)                                   # ties
        sf = f[order]
        assert (sf[1:] >= sf[:-1]).all() and (order[1:] > order[:-1])[sf[1:] == sf[:-1]].all()      # stable
        if n > 1000:
            outside = keys & ~(np.uint64((1 << (b1 - b0)) - 1) << np.uint64(b0))
            if b1 - b0 < 64:
                assert len(np.unique(outside)) > min(n // 2, (1 << (64 - b1 + b0)) - 1)     # random bits outside the field
            if b1 < 64:
                assert (keys >> np.uint64(b1)).any()
            sk = keys[order]
            if b1 - b0 < 60:
                assert (sk[1:] < sk[:-1]).any()                                  # ... so the whole words are not in order


# ---- segmented sorts ------------------------------------------------------------------------------------------------------------------
def test_segment_mixes():
    for name, lengths in list(pi.SEG_MIXES.items()) + list(pi.CAND_MIXES.items()) + list(pi.DESC_MIXES.items()):
        assert sum(lengths) < min(300_000, 1 << pi.SEG_B0), name
    for mixes, avgs in ((pi.SEG_MIXES, (pi.SEG_TUNED_AVG,)), (pi.CAND_MIXES, pi.CAND_AVGS)):
        for a in avgs:
            lo, hi = mixes["below_%d" % a], mixes["at_%d" % a]
            assert sum(lo) // len(lo) == a - 1 and (sum(lo) + 1) // len(lo) == a and sum(hi) // len(hi) == a and (sum(hi) - 1) // len(hi) == a - 1
            for m in (lo, hi):
                assert set(pi.EDGE_LENGTHS) < set(m) and m[0] == 0 and m[-1] == 0 and len(m) == len(pi.EDGE_LENGTHS) + 2
        for c in (1, 63, 64):
            assert len(mixes["segs_%d" % c]) == c
    e = set(pi.EDGE_LENGTHS)
    S, M = pi.WARP_SMALL, pi.WARP_MEDIUM
    assert {0, 1, 2, S, S + 1, M, M + 1, 255, 256, 257, 4095, 4096, 4097} == e
    for c in (63, 64):
        assert {S - 1, S, S + 1, M - 1, M, M + 1, 0, 1} <= set(pi.SEG_MIXES["segs_%d" % c])
    assert pi.WARP_PARTITION == 64
    # the variants the names claim
    w = 8
    sv = lambda m: pi.seg_variant(sum(pi.SEG_MIXES[m]), len(pi.SEG_MIXES[m]), w)
    cv = lambda m: pi.cand_cfg(sum(pi.CAND_MIXES[m]), len(pi.CAND_MIXES[m]))
    assert [sv("below_4096"), sv("at_4096"), sv("segs_1"), sv("segs_63"), sv("segs_64")] == [0, 2, 2, 0, 0]
    assert [pi.seg_variant(sum(pi.SEG_MIXES["at_4096"]), 15, x) for x in pi.SEG_WIDTHS] == [2, 2, 2, 2, 6, 6, 2]
    assert [cv("below_1024"), cv("at_1024"), cv("below_3072"), cv("at_3072"), cv("segs_1"), cv("segs_63")] == [0, 1, 1, 2, 2, 0]


def test_segment_words_and_definition():
    ranges = [(pi.SEG_B0, pi.SEG_B0 + w) for w in pi.SEG_WIDTHS] + [pi.SEG_B1_63]
    assert ranges[-1][1] == 63 and set(pi.SEG_WIDTHS) == {1, 8, 9, 24, 25, 27, 28}
    for lengths in (pi.SEG_MIXES["below_4096"], pi.SEG_MIXES["segs_64"]):
        b = pi.bounds(lengths)
        for b0, b1 in ranges:
            words = pi.seg_words(lengths, b0, b1)
            f = pi.field_of(words, b0, b1)
            assert ((words & np.uint64((1 << b0) - 1)) == np.arange(len(words))).all()           # the position below the field
            assert len(np.unique(words >> np.uint64(b1))) == min(len([x for x in lengths if x]), 1 << (64 - b1))
            for s, e in zip(b[:-1].tolist(), b[1:].tolist()):
                if e - s >= pi.WARP_SMALL:
                    assert len(np.unique(f[s:e])) < e - s                                       # ties in every such segment
            if b1 - b0 > 1:
                assert len(np.unique(f)) > 8
            ref = pi.seg_sort_ref(words, b[:-1], b[1:], b0, b1, 0)
            assert sorted(ref.tolist()) == sorted(words.tolist()) and (ref != words).any()
            s, e = int(b[7]), int(b[8])
            pos = (ref[s:e] & np.uint64((1 << b0) - 1)).astype(np.int64)
            rf = pi.field_of(ref[s:e], b0, b1)
            assert (rf[1:] >= rf[:-1]).all() and (pos[1:] > pos[:-1])[rf[1:] == rf[:-1]].all()
            d = pi.seg_sort_ref(words, b[:-1], b[1:], b0, b1, 0, descending=True)
            pos, df = (d[s:e] & np.uint64((1 << b0) - 1)).astype(np.int64), pi.field_of(d[s:e], b0, b1)
            assert (df[1:] <= df[:-1]).all() and (pos[1:] > pos[:-1])[df[1:] == df[:-1]].all()   # ties keep input order


def test_gapped_segments():
    for lengths in pi.SEG_MIXES.values():
        begins, ends = pi.gapped(lengths)
        b = pi.bounds(lengths)
        assert (begins == b[:-1]).all() and (ends <= b[1:]).all() and (ends >= begins).all()
        if len(lengths) > 2:
            assert (ends < b[1:]).any()
        ref = pi.seg_sort_ref(pi.seg_words(lengths, pi.SEG_B0, pi.SEG_B0 + 8), begins, ends, pi.SEG_B0, pi.SEG_B0 + 8, 7)
        assert int((ref == 7).sum()) == int((b[1:] - ends).sum())


def test_descending_inputs():
    assert all(b1 < 64 for b1 in pi.DESC_END_BITS) and 63 in pi.DESC_END_BITS and all(b0 > 0 for b0, _ in pi.DESC_TAGGED)
    for lengths in pi.DESC_MIXES.values():
        words = pi.seg_words(lengths, 0, 24)
        assert len(np.unique(words)) < len(words)
