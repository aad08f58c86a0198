"""The shared device primitives, one at a time (include/sohit.h so_prim_*, csrc/prim.hip): the scans, run helpers and library sorts every
device stage stands on, run through the wrappers the stages call.  For the tests (tests/test_gpu_prim.py); a refusal raises RuntimeError
with the library's message."""
import collections
import ctypes as C

import numpy as np

from . import _lib

SENTINEL = 0xA5C3F00D      # what the guard words and the unwritten words of `start` hold
SORT_FILL = 0xD6D6D6D6D6D6D6D6   # a key slot of a sort's output that the sort did not write
GUARD = 4                  # guard words on either side of an output range

# so_prim_sort's kinds
SORT_KEYS, SORT_PAIRS32, SORT_PAIRS64, SORT_SEG, SORT_SEG2, SORT_CAND, SORT_SEG_DESC = range(7)
WRAPPER_ONLY = 0x100       # kind | WRAPPER_ONLY, n >= 2^31: the sort itself (not its *_temp_bytes) is asked and must refuse
PATHS = ("none", "single", "three")

Scan = collections.namedtuple("Scan", "out total before after path tiles")
EffScan = collections.namedtuple("EffScan", "hoff cidx hits seeds guards tiles")
Runs = collections.namedtuple("Runs", "head rid n_runs start")
Numbering = collections.namedtuple("Numbering", "X Y gene_code n_genes first flag")
Sorted = collections.namedtuple("Sorted", "keys values variant tier temp_bytes temp_overrun")


def _ptr(a):
    return C.c_void_p(None if a is None else a.ctypes.data)


def _check(rc):
    if rc != 0:
        raise RuntimeError(_lib.load().so_prim_last_error().decode())


def scan_path(n):
    """-> (path name, tiles) of scan_u32 over n values; no device"""
    t = C.c_int64(0)
    return PATHS[_lib.load().so_prim_scan_path(int(n), C.byref(t))], t.value


def sort_tier(kind, n):
    """-> (tier, largest one-block n, largest merge-sort n) of a device-wide sort; no device"""
    s, m = C.c_int64(0), C.c_int64(0)
    return _lib.load().so_prim_sort_tier(int(kind), int(n), C.byref(s), C.byref(m)), s.value, m.value


def seg_variant(kind, n, nseg, width):
    return _lib.load().so_prim_seg_variant(int(kind), int(n), int(nseg), int(width))


def scan(values, inclusive=False, in_place=False, in_skew=0, out_skew=0, device=0):
    v = np.ascontiguousarray(values, dtype=np.uint32)
    n = len(v)
    out, guards, total = np.empty(max(n, 1), np.uint32), np.zeros(2 * GUARD, np.uint32), np.zeros(1, np.uint32)
    path, tiles = C.c_int32(-1), C.c_int64(-1)
    _check(_lib.load().so_prim_scan(int(device), n, _ptr(v), int(in_skew), int(out_skew), int(bool(inclusive)), int(bool(in_place)), _ptr(out), _ptr(guards),
                                    _ptr(total), C.byref(path), C.byref(tiles)))
    return Scan(out[:n], int(total[0]), guards[:GUARD], guards[GUARD:], PATHS[path.value], tiles.value)


def effscan(mark, scnt, mark_skew=0, scnt_skew=0, device=0):
    m, s = np.ascontiguousarray(mark, dtype=np.uint8), np.ascontiguousarray(scnt, dtype=np.uint32)
    n = len(m)
    if len(s) != n:
        raise ValueError("effscan: one mark and one count per slot")
    hoff, cidx = np.empty(max(n, 1), np.uint32), np.empty(max(n, 1), np.uint32)
    guards, totals, tiles = np.zeros(4 * GUARD, np.uint32), np.zeros(2, np.uint32), C.c_int64(-1)
    _check(_lib.load().so_prim_effscan(int(device), n, _ptr(m), int(mark_skew), _ptr(s), int(scnt_skew), _ptr(hoff), _ptr(cidx), _ptr(guards), _ptr(totals),
                                       C.byref(tiles)))
    return EffScan(hoff[:n], cidx[:n], int(totals[0]), int(totals[1]), guards, tiles.value)


def runs(keys, device=0):
    """keys: an int32 or uint64 array"""
    k = np.ascontiguousarray(keys)
    if k.dtype not in (np.dtype(np.int32), np.dtype(np.uint64)):
        raise ValueError("runs: int32 or uint64 keys")
    n = len(k)
    head, rid, start, nr = np.empty(max(n, 1), np.uint32), np.empty(max(n, 1), np.uint32), np.empty(n + 2, np.uint32), C.c_int64(-1)
    _check(_lib.load().so_prim_runs(int(device), n, k.dtype.itemsize, _ptr(k), _ptr(head), _ptr(rid), _ptr(start), C.byref(nr)))
    return Runs(head[:n], rid[:n], nr.value, start)


def number(cx, cy, n_codes, device=0):
    x, y = np.ascontiguousarray(cx, dtype=np.int32), np.ascontiguousarray(cy, dtype=np.int32)
    nr = len(x)
    if len(y) != nr:
        raise ValueError("number: one cx and one cy per row")
    g = max(min(int(n_codes), 2 * nr), 1)
    X, Y, gc = np.empty(max(nr, 1), np.int32), np.empty(max(nr, 1), np.int32), np.empty(g, np.int32)
    first, flag, ng = np.empty(max(int(n_codes), 1), np.uint32), np.empty(max(2 * nr, 1), np.uint32), C.c_int64(-1)
    _check(_lib.load().so_prim_number(int(device), nr, int(n_codes), _ptr(x), _ptr(y), _ptr(X), _ptr(Y), _ptr(gc), _ptr(first), _ptr(flag), C.byref(ng)))
    return Numbering(X[:nr], Y[:nr], gc, ng.value, first, flag[:2 * nr])


def sort(kind, keys, begin_bit, end_bit, values=None, seg_begin=None, seg_end=None, device=0, n=None):
    """values: uint32 (SORT_PAIRS32) or uint64 (SORT_PAIRS64); seg_begin: nseg + 1 bounds, or with seg_end (SORT_SEG2) nseg begins and
    nseg ends.  n: the count handed over when it is not len(keys) (the refusals: keys may then be None)"""
    base = kind & ~WRAPPER_ONLY
    k = None if keys is None else np.ascontiguousarray(keys, dtype=np.uint64)
    cnt = len(k) if n is None else int(n)
    v = None
    if base in (SORT_PAIRS32, SORT_PAIRS64) and values is not None:
        v = np.ascontiguousarray(values, dtype=np.uint32 if base == SORT_PAIRS32 else np.uint64)
    sb = None if seg_begin is None else np.ascontiguousarray(seg_begin, dtype=np.uint32)
    se = None if seg_end is None else np.ascontiguousarray(seg_end, dtype=np.uint32)
    nseg = 0 if sb is None else (len(sb) if base == SORT_SEG2 else len(sb) - 1)
    kout = None if k is None else np.empty(max(len(k), 1), np.uint64)
    vout = None if v is None else np.empty(max(len(v), 1), v.dtype)
    info = np.full(4, -1, np.int64)
    _check(_lib.load().so_prim_sort(int(device), int(kind), cnt, _ptr(k), _ptr(v), nseg, _ptr(sb), _ptr(se), int(begin_bit), int(end_bit), _ptr(kout), _ptr(vout),
                                    _ptr(info)))
    return Sorted(kout[:cnt], None if vout is None else vout[:cnt], int(info[0]), int(info[1]), int(info[2]), int(info[3]))
