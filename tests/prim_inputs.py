"""TEST INFRASTRUCTURE -- inputs aimed at the edges of the shared device primitives (csrc/k_util.hip, k_sort.hip, k_sortseg.hip, reached
through so_prim_*, swiftortho_amd/prim.py) and their plain numpy definitions: prefix sums as np.cumsum in uint64 reduced mod 2^32, the
sorts as a stable argsort of the sorted field per segment, the numbering as a Python loop.  Fixed seeds throughout; every generator is
cached, its arrays are shared among the tests and must be left unchanged.  tests/test_prim_inputs.py asserts from this file alone that
every named case has the property it is named for; tests/test_gpu_prim.py runs them on the device."""
import functools

import numpy as np

M32 = (1 << 32) - 1

# ---- mirrors of the library's rules (the tests compare them with what the library reports) -----------------------------------------
SCAN_TILE = 8192            # values per tile of scan_u32 / effscan
SCAN_SMALL_TILES = 4        # tiles up to which scan_u32 is one launch
SINGLE_BLOCK = 1024         # keys the device-wide sorts sort in one block
MERGE_LIMIT = 1 << 20       # keys up to which they merge-sort
SEG_TUNED_AVG = 4096        # n / nseg from which sort_keys_u64_seg(2) runs a tuned instance
CAND_AVGS = (1024, 3072)    # ... and sort_cand_keys_seg its two
WARP_SMALL, WARP_MEDIUM, WARP_PARTITION = 32, 128, 64   # keys per segment of the two warp-sort classes, segments from which they are used


def scan_path(n):
    tiles = (n + SCAN_TILE - 1) // SCAN_TILE
    return ("none" if tiles == 0 else "single" if tiles <= SCAN_SMALL_TILES else "three"), tiles


def sort_tier(n, b0=0, b1=0):
    """sort_keys_u64 on a field [b0, 64), b0 > 0, leaves the merge sort out (the library's comparator there: csrc/k_sort.hip)"""
    return 0 if n <= SINGLE_BLOCK else 1 if n <= MERGE_LIMIT and not (b0 > 0 and b1 == 64) else 2


def seg_variant(n, nseg, width):
    if not (nseg and n // nseg >= SEG_TUNED_AVG):
        return 0
    return 6 if 24 < width <= 27 else 2


def cand_cfg(n, nseg):
    avg = n // nseg if nseg else 0
    return 2 if avg >= CAND_AVGS[1] else 1 if avg >= CAND_AVGS[0] else 0


# ---- scan -----------------------------------------------------------------------------------------------------------------------
SCAN_SIZES = (0, 1, 3, 4, 5, 6, 15, 16, 17, 8191, 8192, 8193, 16383, 16384, 16385, 32767, 32768, 32769, 40961, 40966, 256 * 8192,
              256 * 8192 + 1, 257 * 8192 + 3)
SCAN_KINDS = ("small", "ones", "wrap", "last", "full")
SKEW_SIZES = (19, 32771)    # one per launch path, both with a tail that is no multiple of four


@functools.lru_cache(maxsize=None)
def scan_values(n, kind):
    rng = np.random.default_rng(1000 + n % 9973 + 31 * SCAN_KINDS.index(kind))
    if kind == "small":
        v = rng.integers(0, 8, n, dtype=np.uint32)
    elif kind == "ones":
        v = np.ones(n, np.uint32)
    elif kind == "wrap":
        v = np.full(n, M32, np.uint32)
    elif kind == "last":
        v = np.zeros(n, np.uint32)
        v[-1:] = 0x9E3779B9
    else:
        v = rng.integers(0, 1 << 32, n, dtype=np.uint32)
    v.setflags(write=False)
    return v


def scan_ref(values, inclusive):
    """-> (prefix sums mod 2^32, the sum mod 2^32)"""
    c = np.cumsum(values.astype(np.uint64), dtype=np.uint64)
    total = int(c[-1]) & M32 if len(c) else 0
    if not inclusive:
        c = np.concatenate([np.zeros(1, np.uint64), c[:-1]]) if len(c) else c
    return (c & np.uint64(M32)).astype(np.uint32), total


# ---- effscan ----------------------------------------------------------------------------------------------------------------------
EFF_SIZES = (1, 2, 3, 4, 5, 6, 7, 15, 16, 17, 8191, 8192, 8193, 8194, 16383, 16384, 16385, 32767, 32768, 32769, 40961, 256 * 8192 + 1)
MARK_BYTES = (0, 1, 2, 0x80, 0xFF)
EFF_SKEW_SIZES = (19, 32771)
EFF_NEAR_N = 40961


@functools.lru_cache(maxsize=None)
def eff_case(n):
    """(mark, scnt): marks from MARK_BYTES, counts 0 .. 9 with about a fifth of them zero (a set mark over a zero count counts nothing)"""
    rng = np.random.default_rng(2000 + n % 9973)
    mark = rng.choice(np.array(MARK_BYTES, np.uint8), n)
    scnt = rng.integers(1, 10, n, dtype=np.uint32)
    scnt[rng.random(n) < 0.2] = 0
    if n >= 8:   # each of the four bytes of a word the only one set, once with a zero count under it
        mark[0:4] = (0x80, 0, 0, 0)
        mark[4:8] = (0, 0, 0xFF, 0)
        scnt[0], scnt[6] = 7, 0
    mark.setflags(write=False), scnt.setflags(write=False)
    return mark, scnt


@functools.lru_cache(maxsize=None)
def eff_near_overflow():
    """EFF_NEAR_N slots whose hits sum to 2^32 - 17: large counts under set marks in every tile, larger ones under clear marks"""
    mark, scnt = (a.copy() for a in eff_case(EFF_NEAR_N))
    rng = np.random.default_rng(77)
    big = rng.choice(EFF_NEAR_N - 1, 64, replace=False)
    mark[big] = rng.choice(np.array(MARK_BYTES[1:], np.uint8), 64)
    scnt[big] = 0x03F00000
    off = rng.choice(np.setdiff1d(np.arange(EFF_NEAR_N - 1), big), 64, replace=False)
    mark[off], scnt[off] = 0, 0xFFFFFFFF
    mark[-1] = 1
    scnt[-1] = 0
    rest = int(np.where(mark != 0, scnt, 0).astype(np.uint64).sum())
    want = (1 << 32) - 17
    assert 0 < want - rest < (1 << 32)
    scnt[-1] = want - rest
    mark.setflags(write=False), scnt.setflags(write=False)
    return mark, scnt


def effscan_ref(mark, scnt):
    """-> (hoff, cidx, hits mod 2^32, non-empty seeds)"""
    c = np.where(mark != 0, scnt, 0).astype(np.uint32)
    hoff, hits = scan_ref(c, False)
    cidx, seeds = scan_ref((c != 0).astype(np.uint32), False)
    return hoff, cidx, hits, seeds


# ---- runs -------------------------------------------------------------------------------------------------------------------------
RUN_HEADS = (255, 256, 257, 8191, 8192, 8193, 32767, 32768, 32769)
RUN_N = 40000


def _keys_with_heads(n, heads, dtype, value_of_run):
    head = np.zeros(n, np.int64)
    head[list(heads)] = 1
    return np.array([value_of_run(r) for r in range(len(heads) + 1)], dtype=dtype)[np.cumsum(head)]


@functools.lru_cache(maxsize=None)
def run_cases():
    """name -> keys (int32 or uint64)"""
    h63 = 1 << 63
    lo = 0xDEADBEEF
    c = {
        "n1_int": np.array([-7], np.int32),
        "n1_u64": np.array([h63 | 5], np.uint64),
        "all_equal_int": np.full(RUN_N, -3, np.int32),
        "all_equal_u64": np.full(33000, h63 | lo, np.uint64),
        "all_distinct_int": (np.arange(33000, dtype=np.int64) - 16500).astype(np.int32),
        "all_distinct_u64": np.arange(RUN_N, dtype=np.uint64) << np.uint64(32),
        # a run starts at every position of RUN_HEADS and nowhere else
        "heads_int": _keys_with_heads(RUN_N, RUN_HEADS, np.int32, lambda r: 3 * r - 11),
        "heads_u64": _keys_with_heads(RUN_N, RUN_HEADS, np.uint64, lambda r: (r + 1) * 0x100000001),
        # neighbours differ in bits 32 .. 63 only: the low words are all the same
        "u64_high_only": _keys_with_heads(RUN_N, RUN_HEADS + (5, 6, 39999), np.uint64, lambda r: ((r * 0x9E3779B1) & M32) << 32 | lo),
        # ... in bit 63 only
        "u64_bit63_only": _keys_with_heads(RUN_N, RUN_HEADS + (1, 2, 39998), np.uint64, lambda r: (r & 1) << 63 | 0x7123456789ABCDEF),
        "int_negative": _keys_with_heads(RUN_N, RUN_HEADS + (1, 100), np.int32, lambda r: -(1 << 31) + 7 * r),
        "int_cross_zero": np.repeat(np.array([-(1 << 31), -2, -1, 0, 1, (1 << 31) - 1, -1, 0, 0x7FFFFFFF, -(1 << 31)], np.int64), [3, 1, 2, 2, 1, 3, 1, 1, 2, 1]).astype(np.int32),
    }
    for a in c.values():
        a.setflags(write=False)
    return c


def runs_ref(keys):
    """-> (head, rid, starts with the closing word)"""
    head = np.ones(len(keys), np.uint32)
    head[1:] = keys[1:] != keys[:-1]
    rid = np.cumsum(head, dtype=np.uint64).astype(np.uint32)
    start = np.concatenate([np.flatnonzero(head), [len(keys)]]).astype(np.uint32)
    return head, rid, start


# ---- numbering by first appearance ----------------------------------------------------------------------------------------------------
NUM_ROWS = (16384, 16385)    # 2 nr = 32768 (the scan's one launch) and 32770 (its three kernels)
NUM_FAR_CODES = 1_000_003


@functools.lru_cache(maxsize=None)
def number_cases():
    """name -> (cx, cy, n_codes)"""
    c = {}
    for nr in NUM_ROWS:
        rng = np.random.default_rng(3000 + nr)
        ncodes = nr // 3
        cx, cy = rng.integers(0, ncodes, nr), rng.integers(0, ncodes, nr)
        cx[5] = cy[5] = ncodes                          # a row with cx == cy, its code not seen before
        cy[nr - 1] = ncodes + 1                         # a code first (and only) seen as cy, in the last row
        c["rows_%d" % nr] = (cx.astype(np.int32), cy.astype(np.int32), ncodes + 3)
    c["self_row_first"] = (np.array([4, 4, 2], np.int32), np.array([4, 1, 4], np.int32), 6)
    c["first_seen_as_cy"] = (np.array([3, 0, 9, 3], np.int32), np.array([8, 8, 0, 7], np.int32), 10)
    c["far_codes"] = (np.array([NUM_FAR_CODES - 1, 17, 500_000, 17], np.int32), np.array([0, NUM_FAR_CODES - 1, 17, 999], np.int32), NUM_FAR_CODES)
    for t in c.values():
        t[0].setflags(write=False), t[1].setflags(write=False)
    return c


def number_ref(cx, cy, n_codes):
    """-> (X, Y, gene_code, first, flag): genes numbered in the order cx[0], cy[0], cx[1], ... first names them"""
    num, gene_code = {}, []
    first = np.full(n_codes, M32, np.uint32)
    flag = np.zeros(2 * len(cx), np.uint32)
    for i in range(len(cx)):
        for side, code in enumerate((int(cx[i]), int(cy[i]))):
            if code not in num:
                num[code] = len(gene_code)
                gene_code.append(code)
                first[code] = 2 * i + side
                flag[2 * i + side] = 1
    X = np.array([num[int(a)] for a in cx], np.int32)
    Y = np.array([num[int(a)] for a in cy], np.int32)
    return X, Y, np.array(gene_code, np.int32), first, flag


# ---- device-wide sorts ----------------------------------------------------------------------------------------------------------------
WIDE_SIZES = (1, 2, SINGLE_BLOCK, SINGLE_BLOCK + 1, MERGE_LIMIT, MERGE_LIMIT + 1)
WIDE_BITS = (1, 7, 8, 9, 32, 33, 63, 64)
WIDE_RANGES = ((3, 11), (31, 33), (20, 64), (1, 64), (20, 63))     # sort_keys_u64 with begin_bit > 0
WIDE_RANGE_SIZES = (SINGLE_BLOCK, SINGLE_BLOCK + 1, 40000, MERGE_LIMIT + 1)


def _mask(bits):
    return np.uint64((1 << bits) - 1)


def field_of(keys, b0, b1):
    return (keys >> np.uint64(b0)) & _mask(b1 - b0)


@functools.lru_cache(maxsize=None)
def wide_keys(n, b0, b1):
    """n keys: bits [b0, b1) from a pool of at most n / 4 values (ties), every other bit random"""
    rng = np.random.default_rng(4000 + n % 9973 + 67 * b0 + b1)
    w = b1 - b0
    pool = rng.integers(0, 1 << w, max(1, min(1 << min(w, 40), n // 4)), dtype=np.uint64)
    keys = rng.integers(0, 1 << 64, n, dtype=np.uint64) & ~(_mask(w) << np.uint64(b0))
    keys |= rng.choice(pool, n) << np.uint64(b0)
    keys.setflags(write=False)
    return keys


@functools.lru_cache(maxsize=None)
def wide_order(n, b0, b1):
    """the stable order of wide_keys(n, b0, b1) by its field"""
    o = np.argsort(field_of(wide_keys(n, b0, b1), b0, b1), kind="stable")
    o.setflags(write=False)
    return o


# ---- segmented sorts ------------------------------------------------------------------------------------------------------------------
SEG_WIDTHS = (1, 8, 9, 24, 25, 27, 28)
SEG_B0 = 19                       # the word's original position sits below (n stays under 2^19)
SEG_B1_63 = (35, 63)              # the one field that ends at bit 63
EDGE_LENGTHS = (0, 1, 2, 32, 33, 128, 129, 255, 256, 257, 4095, 4096, 4097)
POOL = 29                         # field values per case: a segment of WARP_SMALL keys and more holds a tie


def edge_mix(avg, at):
    """EDGE_LENGTHS, a long segment, an empty last one: n / nseg is avg, exactly (at) or with the largest remainder (not at: the next
    key would not yet change it)"""
    nseg = len(EDGE_LENGTHS) + 2
    n = avg * nseg + (0 if at else nseg - 1)
    long_ = n - sum(EDGE_LENGTHS)
    assert long_ > 0
    return EDGE_LENGTHS[:7] + (long_,) + EDGE_LENGTHS[7:] + (0,)


def count_mix(nseg):
    """nseg segments on both sides of the warp-sort classes (one segment: 5000 keys)"""
    if nseg == 1:
        return (5000,)
    cyc = (31, 32, 33, 127, 128, 129, 0, 1, 2, 200, 130, 34)
    return tuple(cyc[k % len(cyc)] for k in range(nseg))


# name -> segment lengths.  below_* / at_*: n / nseg one below / on a dispatch threshold
SEG_MIXES = {
    "below_4096": edge_mix(4095, False), "at_4096": edge_mix(4096, True),
    "segs_1": count_mix(1), "segs_63": count_mix(63), "segs_64": count_mix(64),
}
CAND_MIXES = {
    "below_1024": edge_mix(1023, False), "at_1024": edge_mix(1024, True), "below_3072": edge_mix(3071, False), "at_3072": edge_mix(3072, True),
    "segs_1": count_mix(1), "segs_63": count_mix(63), "segs_64": count_mix(64),
}
DESC_MIXES = {"segs_63": count_mix(63), "segs_64": count_mix(64), "edges": edge_mix(1023, False)}
DESC_END_BITS = (24, 40, 63)      # begin_bit = 0, as order_chunk sorts a chunk's buckets
DESC_TAGGED = ((SEG_B0, SEG_B0 + 9), (SEG_B0, SEG_B0 + 25))


def bounds(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)


def gapped(lengths):
    """-> (begins, ends): segment k gives up its last k % 3 words (as far as it has them) to the gap in front of segment k + 1"""
    b = bounds(lengths)
    gap = np.minimum(np.arange(len(lengths)) % 3, np.asarray(lengths))
    return b[:-1].copy(), (b[1:] - gap).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def seg_words(lengths, b0, b1):
    """one word per key: its segment's number above b1 (as far as there is room), a field of POOL values in [b0, b1), its position below b0"""
    n, w = int(sum(lengths)), b1 - b0
    assert n < (1 << b0) or b0 == 0
    rng = np.random.default_rng(5000 + len(lengths) + 131 * w + b1 + n % 997)
    pool = rng.integers(0, 1 << w, min(POOL, 1 << w), dtype=np.uint64) if w > 1 else np.array([0, 1], np.uint64)
    seg = np.repeat(np.arange(len(lengths), dtype=np.uint64), lengths) & _mask(64 - b1)
    words = (seg << np.uint64(b1)) | (rng.choice(pool, n) << np.uint64(b0))
    if b0:
        words |= np.arange(n, dtype=np.uint64)
    words.setflags(write=False)
    return words


def seg_sort_ref(words, begins, ends, b0, b1, fill, descending=False):
    """every segment [begins[k], ends[k]) stably sorted by bits [b0, b1) (descending: larger fields first, ties in input order); every other
    word = fill"""
    out = np.full(len(words), fill, np.uint64)
    f = field_of(words, b0, b1)
    if descending:
        f = _mask(b1 - b0) - f
    for s, e in zip(begins.tolist(), ends.tolist()):
        out[s:e] = words[s:e][np.argsort(f[s:e], kind="stable")]
    return out
