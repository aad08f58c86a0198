"""Host-side mirror of the reference's native search core interface (lib/fsearch.py), backed
by libsohit.so on an MI355X.

Same names, argument meaning and error behaviour as the reference for this path:

* ``blastp(qry, ref, expect, v, max_miss, st, ed, rst, red, thr, flt, ..., ssd, nr, step, ht, chk)``
  -- fsearch.py:2968 -- generator of hit tuples in the reference's order;
* ``entry_point(argv)`` -- fsearch.py:3152-3264 -- the ``fsearch-c`` flag grammar (``-k v`` or
  ``-kv``, unknown tokens skipped, always returns 0, manual text on bad input) and the
  16-column output row.

The compute is entirely in the HIP library; this module never falls back to a CPU path.
"""
import ctypes as C
import os
import sys

from . import _lib


class _LazyNumpy:
    """numpy is imported by the first function that uses it: the one-GPU command line (find_hit.py -> Searcher -> Hits.write) never does,
    and its import is ~0.1 s of a 0.7 s command."""

    def __getattr__(self, name):
        import numpy
        globals()["np"] = numpy
        return getattr(numpy, name)


np = _LazyNumpy()

AA9 = "AST,CFILMVY,DN,EQ,G,H,KR,P,W"
AA20 = "A,S,T,C,F,I,L,M,V,Y,D,N,E,Q,G,H,K,R,P,W"


class SohitError(RuntimeError):
    pass


class Searcher:
    """One libsohit context == one GPU (include/sohit.h).  Not thread-safe."""

    def __init__(self, ssd="111111", nr=AA9, ht=120000000, chk=50000, step=1, v=500, thr=-1, expect=1e-3, max_miss=1e-3,
                 flt="T", device=0, profile=False):
        self.L = _lib.load()
        self._keep = (ssd.encode(), nr.encode())
        p = _lib.SoParams(self._keep[0], self._keep[1], int(ht), int(chk), int(step), int(v), int(thr), float(expect),
                          float(max_miss), 1 if flt == "T" else 0, 1 if profile else 0)
        self.device = int(device)
        self.h = self.L.so_create(int(device), C.byref(p))
        if not self.h:
            raise SohitError(self.L.so_last_error(None).decode())
        self.nc = int(self.L.so_bucket_count(self.h))  # -M, or the reference's `bins` default when -M < 1

    def close(self):
        if getattr(self, "h", None):
            self.L.so_destroy(self.h)
            self.h = None

    __del__ = close

    def _chk(self, rc):
        if rc:
            raise SohitError(self.L.so_last_error(self.h).decode())

    # reference side ---------------------------------------------------------------------------
    def load_ref(self, path, rst=-1, red=-1):
        self._chk(self.L.so_load_ref(self.h, os.fsencode(path), rst, red))

    def load_ref_bytes(self, data, rst=-1, red=-1):
        self._chk(self.L.so_load_ref_mem(self.h, data, len(data), rst, red))

    def build_index(self):
        self._chk(self.L.so_build_index(self.h))

    def drop_index(self):
        self._chk(self.L.so_drop_index(self.h))

    def load_index(self, prefix):
        """Fasta.load (fsearch.py:2355-2444): make the chunk indexes `<prefix>.<k>.idx/.soas/.bin` resident instead of building them
        (the reference FASTA must be loaded: the files hold no sequences)."""
        self._chk(self.L.so_load_index(self.h, os.fsencode(prefix)))

    # query side -------------------------------------------------------------------------------
    def load_queries(self, path):
        self._chk(self.L.so_load_queries(self.h, os.fsencode(path)))

    def load_queries_bytes(self, data):
        self._chk(self.L.so_load_queries_mem(self.h, data, len(data)))

    @property
    def num_queries(self):
        return int(self.L.so_num_queries(self.h))

    @property
    def num_refs(self):
        return int(self.L.so_num_refs(self.h))

    def query_lengths(self):
        n = self.num_queries
        return np.array([self.L.so_query_len(self.h, i) for i in range(n)], dtype=np.int64)

    def ref_lengths(self):
        n = self.num_refs
        return np.array([self.L.so_ref_len(self.h, i) for i in range(n)], dtype=np.int64)

    # search -----------------------------------------------------------------------------------
    def search(self, st=-1, ed=-1, alignments=False, cigar=False):
        """Queries [st, ed) of the loaded query file -> Hits (owning wrapper).  alignments=True: every row also carries its
        aligned query and subject strings (Hits.alignment / Hits.alignment_buffer).  cigar=True: every row carries its alignment
        path as a CIGAR instead (Hits.cigar / Hits.cigar_ops; Hits.write then writes it as a 17th column) -- a few bytes per row,
        coded on the GPU; cigar_to_strings() leads from it to the strings.  One search gives one of the two."""
        if alignments and cigar:
            raise ValueError("alignments=True and cigar=True in one search: ask for one of them")
        hits = C.POINTER(_lib.SoHit)()
        n = C.c_int64(0)
        if cigar:
            ops, off = C.c_void_p(), C.c_void_p()
            self._chk(self.L.so_search_loaded_cigar(self.h, st, ed, C.byref(hits), C.byref(n), C.byref(ops), C.byref(off)))
            return Hits(self, hits, n.value, cigar_ptrs=(ops.value, off.value))
        if not alignments:
            self._chk(self.L.so_search_loaded(self.h, st, ed, C.byref(hits), C.byref(n)))
            return Hits(self, hits, n.value)
        aln = C.c_void_p()
        nb = C.c_int64(0)
        self._chk(self.L.so_search_loaded_aln(self.h, st, ed, C.byref(hits), C.byref(n), C.byref(aln), C.byref(nb)))
        return Hits(self, hits, n.value, aln.value, nb.value)

    def search_device(self, st=-1, ed=-1):
        """Like search(), but the so_hit records stay in HBM (multi-GPU path: exchanged over RCCL before any host copy)."""
        n = C.c_int64(0)
        ptr = C.c_void_p()
        self._chk(self.L.so_search_device(self.h, st, ed, C.byref(ptr), C.byref(n)))
        return DeviceHits(self, n.value, ptr.value)

    def query_work(self, st=-1, ed=-1):
        """Index entries each query of [st, ed) visits over all chunks (pre-pass, no search): the shard-balancing weight."""
        N = self.num_queries
        lo = min(max(0, st), N)
        hi = min(N if ed < 0 else ed, N)
        out = np.zeros(max(hi - lo, 1), dtype=np.uint64)
        self._chk(self.L.so_query_work(self.h, lo, hi, out.ctypes.data))
        return out[:max(hi - lo, 0)].astype(np.int64)

    def counters(self):
        c = _lib.SoCounters()
        self.L.so_get_counters(self.h, C.byref(c))
        return c.as_dict()

    def set_profile(self, on):
        self.L.so_set_profile(self.h, 1 if on else 0)

    def set_option(self, name, value):
        """one switch of csrc/tune.h by its SOHIT_* name, for this searcher from now on (so_create read the environment once)"""
        if self.L.so_set_option(self.h, str(name).encode(), str(value).encode()) != 0:
            raise ValueError(self.L.so_last_error(self.h).decode())

    def reset_counters(self):
        self.L.so_reset_counters(self.h)

    def timing(self):
        n = self.L.so_timing_report(self.h, None, 0)
        buf = C.create_string_buffer(n + 2)
        self.L.so_timing_report(self.h, buf, n + 1)
        return {kv.split("=")[0]: float(kv.split("=")[1]) for kv in buf.value.decode().split(";") if kv}

    # introspection (tests) ----------------------------------------------------------------------
    def chunk_threshold(self, k):
        return int(self.L.so_chunk_threshold(self.h, k))

    def chunk_index(self, k):
        n = int(self.L.so_chunk_entries(self.h, k))
        start = np.zeros(self.nc + 1, dtype=np.uint32)
        ent = np.zeros(max(n, 1), dtype=np.uint64)
        self._chk(self.L.so_chunk_download(self.h, k, start.ctypes.data, ent.ctypes.data))
        return start, ent[:n]

    def masked_query(self, q):
        n = self.L.so_masked_query(self.h, q, None, 0)
        if n < 0:
            return None
        buf = C.create_string_buffer(max(1, n))
        self.L.so_masked_query(self.h, q, buf, n)
        return buf.raw[:n]

    def query_candidates(self, q):
        n = self.L.so_query_candidates(self.h, q, None, 0)
        if n < 0:
            return None
        out = np.zeros((max(n, 1), 4), dtype=np.uint32)
        self.L.so_query_candidates(self.h, q, out.ctypes.data, n)
        return out[:n]

    P2_FIELDS = ("next", "unmch", "bv", "nsel", "done", "ntask", "ntile", "qcells")

    def query_phase2(self, q):
        """tests (SOHIT_KEEP_CANDS=1): query q's phase-2 state behind the alignment rounds of the last search, a dict of P2_FIELDS --
        the stop rule's next rank, consecutive misses, passing tiles, selected tiles and stopped flag, the ranks considered, their
        alignment tasks and the band cells of the tasks aligned (None without a kept state)"""
        out = np.zeros(8, dtype=np.int64)
        if self.L.so_query_phase2(self.h, q, out.ctypes.data) != 0:
            return None
        return dict(zip(self.P2_FIELDS, (int(x) for x in out)))

    ALIGN_DTYPE = [(f, "<i4") for f in ("maxscore", "aln", "matches", "gap", "qst", "qed", "sst", "sed", "cells", "wide")]

    def align_pairs(self, tasks, kernel, order=None, alignments=False, cigar=False):
        """tests: the windows tasks[k] = (qidx, sidx, qi, qj, qe, se) aligned by ONE phase-2 aligner (so_align_pairs; qe / se = -1: the
        sequence's end) -> one record per task, fields ALIGN_DTYPE.  order: the launch list (None: 0 .. n-1).  alignments=True (traced
        kernels 3 and 4, so_align_pairs_aln): (records, [(query string, subject string) per task]), built by the search's emission chain.
        cigar=True (kernels 3 and 4, so_align_pairs_cigar): (records, [uint32 runs per task]) -- format_cigar() gives their text."""
        if alignments and cigar:
            raise ValueError("alignments=True and cigar=True in one call: ask for one of them")
        t = np.ascontiguousarray(np.asarray(tasks, dtype=np.int64).reshape(-1, 6))
        n = len(t)
        out = np.zeros(max(n, 1), dtype=self.ALIGN_DTYPE)
        o = None
        if order is not None:
            o = np.ascontiguousarray(np.asarray(order, dtype=np.uint32))
            if len(o) != n:
                raise ValueError("order must hold n positions")
        if cigar:
            ops, off = C.c_void_p(), C.c_void_p()
            self._chk(self.L.so_align_pairs_cigar(self.h, int(kernel), n, t.ctypes.data, None if o is None else o.ctypes.data, out.ctypes.data,
                                                  C.byref(ops), C.byref(off)))
            try:
                offs = np.frombuffer((C.c_int64 * (n + 1)).from_address(off.value), dtype=np.int64).copy()
                runs = np.frombuffer((C.c_uint32 * max(int(offs[n]), 1)).from_address(ops.value), dtype=np.uint32)[:int(offs[n])].copy()
            finally:
                self.L.so_free_cigar(ops, off)
            return out[:n], [runs[int(offs[k]):int(offs[k + 1])] for k in range(n)]
        if not alignments:
            self._chk(self.L.so_align_pairs(self.h, int(kernel), n, t.ctypes.data, None if o is None else o.ctypes.data, out.ctypes.data))
            return out[:n]
        ptr, nb = C.c_void_p(), C.c_int64()
        self._chk(self.L.so_align_pairs_aln(self.h, int(kernel), n, t.ctypes.data, None if o is None else o.ctypes.data, out.ctypes.data,
                                            C.byref(ptr), C.byref(nb)))
        try:
            raw = C.string_at(ptr.value, nb.value) if nb.value else b""
        finally:
            self.L.so_free_aln(ptr)
        alns, pos = [], 0
        for a in out[:n]["aln"].tolist():
            a = max(0, a)
            alns.append((raw[pos:pos + a], raw[pos + a:pos + 2 * a]))
            pos += 2 * a
        if pos != len(raw):
            raise SohitError("so_align_pairs_aln: the strings do not match the records")
        return out[:n], alns


class DeviceHits:
    """so_hit records of one so_search_device() call, resident in the ctx's device memory until its next search."""
    record_bytes = C.sizeof(_lib.SoHit)

    def __init__(self, s, n, ptr=None):
        self.s, self.n, self.ptr = s, n, ptr

    def device_pointer(self):
        """address of the records in the ctx's device memory (so_search_device's d_hits; 0 when there are none): for device-side consumers
        such as find_orth.relations_from_device, until the searcher's next search"""
        return int(self.ptr or 0)

    def __len__(self):
        return self.n

    def tensor(self, device=None):
        """uint8 torch tensor (n * 80 bytes) on the ctx's GPU holding a copy of the records (device-to-device)."""
        import torch
        t = torch.empty(self.n * self.record_bytes, dtype=torch.uint8, device=device or torch.device("cuda", torch.cuda.current_device()))
        # the block comes from torch's caching allocator on torch's stream and is filled from the library's own stream: nothing torch
        # queued earlier on that block may still be running when the copy starts
        torch.cuda.current_stream(t.device).synchronize()
        self.s._chk(self.s.L.so_device_hits_copy(self.s.h, C.c_void_p(t.data_ptr()), self.n))
        return t

    def close(self):
        pass


def hits_from_bytes(s, data):
    """so_hit records gathered from other ranks (bytes / uint8 array) -> ctypes array usable with so_write_sc / so_format_hit.
    A writable contiguous uint8 array (the pinned staging buffer of the gather) is wrapped in place: a 1 M-protein result is 24 GB
    and must not be copied again on rank 0."""
    rec = C.sizeof(_lib.SoHit)
    if isinstance(data, np.ndarray) and data.dtype == np.uint8 and data.flags.c_contiguous and data.flags.writeable and data.size >= rec:
        n = data.size // rec
        arr = (_lib.SoHit * n).from_buffer(data)
        return arr, n
    buf = np.ascontiguousarray(data, dtype=np.uint8).tobytes()
    n = len(buf) // rec
    arr = (_lib.SoHit * max(n, 1)).from_buffer_copy(buf + b"\0" * (rec if n == 0 else 0))
    return arr, n


class Hits:
    """Result rows of one search; frees the library buffer on close."""

    def __init__(self, s, ptr, n, aln_ptr=None, aln_bytes=0, cigar_ptrs=None):
        self.s, self.ptr, self.n = s, ptr, n
        self.aln_ptr, self.aln_bytes = aln_ptr, aln_bytes
        self._aln_off = None
        self.cig_ptrs = cigar_ptrs   # (ops, op_off) of so_search_loaded_cigar
        self._cig = None

    def __len__(self):
        return self.n

    def _aln_offsets(self):
        if self.aln_ptr is None:
            raise SohitError("this search was run without alignments: Searcher.search(..., alignments=True)")
        if self._aln_off is None:
            a = self.array()["aln"].astype(np.int64) if self.n else np.zeros(0, dtype=np.int64)
            off = np.zeros(self.n + 1, dtype=np.int64)
            np.cumsum(2 * a, out=off[1:])
            self._aln_off = off
        return self._aln_off

    def alignment_buffer(self):
        """(uint8 view of the strings -- no copy, valid until close() --, int64 offsets [n + 1]): row k's query string is
        buf[off[k] : off[k] + aln_k], its subject string buf[off[k] + aln_k : off[k + 1]]."""
        off = self._aln_offsets()
        if not self.aln_bytes:
            return np.zeros(0, dtype=np.uint8), off
        return np.frombuffer((C.c_char * self.aln_bytes).from_address(self.aln_ptr), dtype=np.uint8), off

    def alignment(self, k):
        """(query string, subject string) of row k as bytes: kswat_st's al0 / al1 (fsearch.py:1417-1444)."""
        off = self._aln_offsets()
        if not 0 <= k < self.n:
            raise IndexError(k)
        a0, a1 = int(off[k]), int(off[k + 1])
        mid = (a0 + a1) // 2
        return C.string_at(self.aln_ptr + a0, mid - a0), C.string_at(self.aln_ptr + mid, a1 - mid)

    def cigar_buffer(self):
        """(uint32 view of every row's runs -- no copy, valid until close() --, int64 offsets [n + 1]): row k's runs are
        ops[off[k]:off[k + 1]], each length << 4 | op with op 0 = M, 1 = I, 2 = D, first column first."""
        if self.cig_ptrs is None:
            raise SohitError("this search was run without CIGARs: Searcher.search(..., cigar=True)")
        if self._cig is None:
            off = np.frombuffer((C.c_int64 * (self.n + 1)).from_address(self.cig_ptrs[1]), dtype=np.int64)
            nops = int(off[self.n])
            ops = np.frombuffer((C.c_uint32 * nops).from_address(self.cig_ptrs[0]), dtype=np.uint32) if nops else np.zeros(0, dtype=np.uint32)
            self._cig = (ops, off)
        return self._cig

    def cigar_ops(self, k):
        """row k's runs: a uint32 view, length << 4 | op (0 M, 1 I, 2 D)"""
        ops, off = self.cigar_buffer()
        if not 0 <= k < self.n:
            raise IndexError(k)
        return ops[int(off[k]):int(off[k + 1])]

    def cigar(self, k):
        """row k's CIGAR as text: M both sides advance, I the query alone, D the subject alone (35M2D10M)"""
        return format_cigar(self.cigar_ops(k))

    def array(self):
        """numpy structured view (copy) of the so_hit records."""
        dt = np.dtype([(n, t) for n, t in (("qidx", "<i8"), ("sidx", "<i8"), ("identity", "<f8"), ("evalue", "<f8"), ("aln", "<i4"),
                                          ("mis", "<i4"), ("gap", "<i4"), ("qst", "<i4"), ("qed", "<i4"), ("sst", "<i4"),
                                          ("sed", "<i4"), ("bit", "<i4"), ("qlen", "<i4"), ("slen", "<i4"), ("matches", "<i4"),
                                          ("ungapped", "<i4"))])
        if self.n == 0:
            return np.zeros(0, dtype=dt)
        nbytes = self.n * C.sizeof(_lib.SoHit)  # can exceed 2 GiB (1M x 1M: 24 GB): no string_at
        view = (C.c_char * nbytes).from_address(C.addressof(self.ptr.contents))
        return np.frombuffer(view, dtype=dt).copy()

    def write(self, path, mode="w"):
        """the rows as text: 16 columns, or 17 -- the CIGAR last -- when the hits carry CIGARs"""
        if self.cig_ptrs is not None:
            self.s._chk(self.s.L.so_write_sc_cigar(self.s.h, self.ptr, self.n, self.cig_ptrs[0], self.cig_ptrs[1], os.fsencode(path), mode.encode()))
            return
        self.s._chk(self.s.L.so_write_sc(self.s.h, self.ptr, self.n, os.fsencode(path), mode.encode()))

    def rows(self):
        buf = C.create_string_buffer(1 << 16)
        out = []
        for i in range(self.n):
            k = self.s.L.so_format_hit(self.s.h, C.byref(self.ptr[i]), buf, len(buf))
            if k < 0:
                raise SohitError(self.s.L.so_last_error(self.s.h).decode())
            if k >= len(buf):  # so_format_hit returns the size it needs: very long headers
                buf = C.create_string_buffer(int(k) + 1)
                k = self.s.L.so_format_hit(self.s.h, C.byref(self.ptr[i]), buf, len(buf))
            out.append(buf.raw[:k])
        return out

    def view_u8(self):
        """uint8 numpy view of the record buffer (no copy; valid until close())."""
        if not self.n:
            return np.zeros(0, dtype=np.uint8)
        nbytes = self.n * C.sizeof(_lib.SoHit)
        return np.frombuffer((C.c_char * nbytes).from_address(C.addressof(self.ptr.contents)), dtype=np.uint8)

    def raw_bytes(self):
        if not self.n:
            return b""
        nbytes = self.n * C.sizeof(_lib.SoHit)
        return bytes((C.c_char * nbytes).from_address(C.addressof(self.ptr.contents)))

    def close(self):
        if self.ptr:
            self.s.L.so_free_hits(self.ptr)
            self.ptr = None
        if self.aln_ptr:
            self.s.L.so_free_aln(self.aln_ptr)
            self.aln_ptr = None
        if self.cig_ptrs:
            self._cig = None
            self.s.L.so_free_cigar(self.cig_ptrs[0], self.cig_ptrs[1])
            self.cig_ptrs = None

    __del__ = close


def blastp(qry, ref, expect=1e-5, v=500, max_miss=1e-3, st=-1, ed=-1, rst=-1, red=-1, thr=-1, flt="T", ref_idx="", memory=True,
           ssd="", nr="", step=4, ht=-1, chk=100000, tmpdir="./tmpdir", device=0, alignments=False, cigar=False):
    """fsearch.py:2968 -- yields (i, j, li, lj, idy, aln, mis, gap, qst, qed, sst, sed, e, bit, seed) per reported row
    (query ordinal, subject ordinal, lengths, identity, ..., 1-based starts as printed, e-value, bit, ungapped score);
    alignments=True: + (query string, subject string) as bytes; cigar=True: + the CIGAR text (one of the two per call)."""
    s = Searcher(ssd=ssd, nr=nr, ht=ht, chk=chk, step=step, v=v, thr=thr, expect=expect, max_miss=max_miss, flt=flt, device=device)
    try:
        s.load_ref(ref, rst, red)
        s.load_queries(qry)
        hits = s.search(st, ed, alignments=alignments, cigar=cigar)
        for k, r in enumerate(hits.array()):
            row = (int(r["qidx"]), int(r["sidx"]), int(r["qlen"]), int(r["slen"]), float(r["identity"]), int(r["aln"]), int(r["mis"]),
                   int(r["gap"]), int(r["qst"]), int(r["qed"]), int(r["sst"]), int(r["sed"]), float(r["evalue"]), int(r["bit"]),
                   int(r["ungapped"]))
            yield row + hits.alignment(k) if alignments else row + (hits.cigar(k),) if cigar else row
        hits.close()
    finally:
        s.close()


def aln_stats(al0, al1):
    """(matches, mis, gap, identity) of two aligned strings by the reference's rules (fsearch.py:1454-1471): a column counts
    as a match when its two characters are equal, a mismatch otherwise; gap openings by the three-state machine over '-'
    characters (a literal '-' residue counts like a gap); identity = matches * (100. / len).  The reference runs the machine over
    its own order of the two strings, subject first when it put the subject on its columns; the orders can differ only where a
    column holds '-' on both sides (a literal '-' residue opposite a gap), and aln_stats(al1, al0) gives the other one."""
    if len(al0) != len(al1):
        raise ValueError("aligned strings differ in length")
    if isinstance(al0, str):
        al0 = al0.encode("latin-1")
    if isinstance(al1, str):
        al1 = al1.encode("latin-1")
    AL = len(al0)
    idy = 0.
    mis = gap = 0
    op = -1
    dash = 45   # '-'
    for a, b in zip(al0, al1):
        if a == b:
            idy += 1.
        else:
            mis += 1
        if a == dash and op != 0:
            gap += 1
            op = 0
        elif b == dash and op != 1:
            gap += 1
            op = 1
        else:
            op = -1
    matches = AL - mis
    identity = idy * (100. / AL) if AL else float("nan")
    return matches, mis, gap, identity


def format_cigar(ops):
    """runs (uint32, length << 4 | op with op 0 = M, 1 = I, 2 = D) -> CIGAR text by the library's formatter (so_format_cigar; no device)"""
    a = np.ascontiguousarray(np.asarray(ops, dtype=np.uint32))
    L = _lib.load()
    n = int(L.so_format_cigar(a.ctypes.data if len(a) else None, len(a), None, 0))
    if n < 0:
        raise ValueError("not a CIGAR: a run of length 0 or an unknown operation")
    buf = C.create_string_buffer(n + 1)
    L.so_format_cigar(a.ctypes.data if len(a) else None, len(a), buf, n + 1)
    return buf.raw[:n].decode("ascii")


def parse_cigar(cigar):
    """CIGAR text -> [(length, op)] with op in 'MID'; runs of length 0 and repeated operations are accepted as written"""
    if isinstance(cigar, bytes):
        cigar = cigar.decode("ascii")
    runs, n, digits = [], 0, False
    for ch in cigar:
        if ch.isdigit():
            n, digits = 10 * n + int(ch), True
            continue
        if ch not in "MID" or not digits:
            raise ValueError("not a CIGAR of M, I and D runs: %r" % cigar[:60])
        runs.append((n, ch))
        n, digits = 0, False
    if digits:
        raise ValueError("CIGAR ends inside a run: %r" % cigar[-60:])
    return runs


def cigar_to_strings(cigar, q, s, qst, sst):
    """(query string, subject string) as bytes -- so_search_loaded_aln's strings -- from a row's CIGAR (text, or uint32 runs), the query
    as the aligner saw it (Searcher.masked_query: SEG-masked under -F T), the subject, and the row's 1-based starts as printed: M
    takes a residue of either, I one of the query opposite '-', D one of the subject opposite '-'.  Non-canonical CIGARs are accepted."""
    if not isinstance(cigar, (str, bytes)):
        cigar = [(int(v) >> 4, "MID"[int(v) & 15]) for v in cigar]
    else:
        cigar = parse_cigar(cigar)
    q = q.encode("latin-1") if isinstance(q, str) else bytes(q)
    s = s.encode("latin-1") if isinstance(s, str) else bytes(s)
    a0, a1, qp, sp = [], [], qst - 1, sst - 1
    if qst < 1 or sst < 1 or qp + sum(n for n, op in cigar if op != "D") > len(q) or sp + sum(n for n, op in cigar if op != "I") > len(s):
        raise ValueError("the CIGAR runs past its sequences")
    for n, op in cigar:
        if op == "M":
            a0.append(q[qp:qp + n]), a1.append(s[sp:sp + n])
            qp, sp = qp + n, sp + n
        elif op == "I":
            a0.append(q[qp:qp + n]), a1.append(b"-" * n)
            qp += n
        else:
            a0.append(b"-" * n), a1.append(s[sp:sp + n])
            sp += n
    return b"".join(a0), b"".join(a1)


def makedb(ref, space='11111111', nr=AA9, step=1, ht=-1, chk=500000, device=0):
    """fsearch.py:2809-2814 + Fasta.makedb / Fasta.write (2283-2352): build the chunk indexes of `ref` (on the GPU) and write them
    in the reference's on-disk format, `<ref>.<k>.idx` (locus: int32 per index entry, a bucket's entries in the reference's
    slot order = descending insertion order), `<ref>.<k>.soas` (prefix lengths of the chunk's sequences) and `<ref>.<k>.bin`
    (start[NC] + the trailer `offset;offend;max weight;threshold;NC;seeds;alphabet` + one length byte).  Nothing in the
    reference's own entry point reads these files back (`entry_point` accepts `-p blastp` only and `blastp` always indexes in
    memory); they are written for tools that consume the format.  Returns the list of (start, end) chunk ranges."""
    s = Searcher(ssd=space, nr=nr, ht=ht, chk=chk, step=step, device=device)
    out = []
    try:
        s.load_ref(ref)
        s.build_index()
        lens = s.ref_lengths()
        N = len(lens)
        mw = max(sp.count('1') for sp in space.split(','))
        NC = s.nc
        for k, i in enumerate(range(0, N, chk)):
            st, ed = i, min(i + chk, N)
            start, ent = s.chunk_index(k)
            soas = np.concatenate([[0], np.cumsum(lens[st:ed])]).astype(np.int64)
            # (so_chunk_download hands the entries over in the reference's slot order: bucket ascending, entry descending inside a bucket --
            # the device puts them in that order, order_chunk in host_index.hip; until round 6 a host lexsort of the chunk did)
            assert int(start[NC]) == len(ent)
            locus = soas[(ent >> np.uint64(32)).astype(np.int64)] + (ent & np.uint64(0xFFFFFF)).astype(np.int64)
            name = '%s.%d' % (ref, i // chk)
            locus.astype('<i4').tofile(name + '.idx')
            soas.astype('<i4').tofile(name + '.soas')
            trailer = '%d;%d;%d;%d;%d;%s;%s' % (st, ed + 1, mw, s.chunk_threshold(k), NC, space, nr)
            with open(name + '.bin', 'wb') as f:
                start[:NC].astype('<i4').tofile(f)
                f.write(trailer.encode('latin-1') + bytes([len(trailer) & 0xFF]))
            out.append((st, ed))
    finally:
        s.close()
    return out


def index_params(name):
    """The parameter trailer of one chunk's `.bin` file as Fasta.load reads it (fsearch.py:2380-2387): the last byte is the length
    of `offset;offend;max weight;threshold;NC;seeds;alphabet`."""
    with open(name + '.bin', 'rb') as f:
        f.seek(0, os.SEEK_END)
        n = f.tell()
        f.seek(n - 1)
        m = f.read(1)[0]
        start = max(n - m - 1, 0)
        f.seek(start)
        para = f.read(m).decode('latin-1')
    offset, offend, mw, thr, nc, space, nr = para.split(';')
    return dict(offset=int(offset), offend=int(offend), mw=int(mw), threshold=int(thr), NC=int(nc), space=space, nr=nr)


def load(ref, name=None, device=0, **search_kw):
    """Fasta.load (fsearch.py:2355-2444) for every chunk `makedb` wrote: a Searcher over `ref` whose index comes from the files
    `<name>.<k>.idx/.soas/.bin` (name defaults to `ref`, as makedb names them), created with the seeds, alphabet and bucket count
    of the files' own trailer; `search_kw` = the search-side parameters (v, expect, max_miss, thr, flt, step is irrelevant here)."""
    name = name or ref
    p = index_params('%s.0' % name)
    s = Searcher(ssd=p['space'], nr=p['nr'], ht=p['NC'], device=device, **search_kw)
    try:
        s.load_ref(ref)
        s.load_index(name)
    except Exception:
        s.close()
        raise
    return s


def manual_print(out=None):
    w = (out or sys.stdout).write
    w("Usage:\n  fsearch -p blastp -i qry.fsa -d db.fsa\nParameters:\n")
    for line in ("-p: program", "-i: query sequences in fasta format", "-l: start index of query sequences",
                 "-u: end index of query sequences", "-L: start index of reference", "-U: end index of reference",
                 "-d: ref database", "-o: output file", "-O: write mode of output file. w: overwrite, a: append",
                 "-s: spaced seed in format: 1111,1110,1001.. etc",
                 "-r: reduced amino acid alphabet in format: AST,CFILMVY,DN,EQ,G,H,KR,P,W", "-v: number of hits to show",
                 "-e: expect value", "-m: max ratio of pseudo hits that will trigger stop",
                 "-j: distance between start sites of two neighbor seeds, greater will reduce the size of database",
                 "-t: filter high frequency kmers whose counts > t", "-F: Filter query sequence",
                 "-M: bucket size of hash table", "-c: chunck size of reference. default is 50K",
                 "-T: tmpdir (accepted, unused: nothing is spilled to disk)"):
        w("  %s\n" % line)


DEFAULTS = {'-p': '', '-v': '500', '-s': '111111', '-i': '', '-d': '', '-e': '1e-3', '-l': '-1', '-u': '-1', '-m': '1e-3',
            '-t': '-1', '-r': AA9, '-j': '4', '-F': 'T', '-o': '', '-D': '', '-O': 'wb', '-L': '-1', '-U': '-1', '-M': '-1',
            '-c': '50000', '-T': './tmpdir'}


def parse_flags(argv, defaults):
    """fsearch.py:3189-3199: `-k v` or `-kv`; unknown tokens are skipped."""
    args = dict(defaults)
    n = len(argv)
    for i in range(1, n):
        k = argv[i]
        if k in args:
            if i + 1 < n:
                args[k] = argv[i + 1]
        elif k[:2] in args and len(k) > 2:
            args[k[:2]] = k[2:]
    return args


def entry_point(argv, device=0, searcher=None):
    """fsearch.py:3152 -- same flags as lib/fsearch-c; writes the 16-column rows; always returns 0."""
    args = parse_flags(argv, DEFAULTS)
    if args['-p'] != 'blastp' or args['-i'] == '' or args['-d'] == '':
        manual_print()
        return 0
    try:
        exp, bv, start, end = float(args['-e']), int(args['-v']), int(args['-l']), int(args['-u'])
        rstart, rend, miss, thr = int(args['-L']), int(args['-U']), float(args['-m']), int(args['-t'])
        step, ht, chk = int(args['-j']), int(args['-M']), int(args['-c'])
    except ValueError:
        print('blastp')
        manual_print()
        return 0
    wrt = args['-O']
    wrt = wrt if (wrt and wrt in 'wa') else 'w'
    try:
        s = searcher or Searcher(ssd=args['-s'], nr=args['-r'], ht=ht, chk=chk, step=step, v=bv, thr=thr, expect=exp, max_miss=miss,
                                 flt=args['-F'], device=device)
    except SohitError as e:  # e.g. -M < 1 with an odd seed weight (the reference crashes there); the native always returns 0
        sys.stderr.write('fsearch: %s\n' % e)
        return 0
    try:
        s.load_ref(args['-d'], rstart, rend)
        s.load_queries(args['-i'])
        hits = s.search(start, end)
        if args['-o']:
            hits.write(args['-o'], wrt)
        else:
            for r in hits.rows():
                sys.stdout.write(r.decode('latin-1'))
        hits.close()
    finally:
        if searcher is None:
            s.close()
    return 0


if __name__ == "__main__":
    sys.exit(entry_point(sys.argv))
