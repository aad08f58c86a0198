"""ctypes binding of libsohit.so (include/sohit.h).  No fallback: if the HIP library is
missing or no GPU is usable, importing/creating a context raises."""
import contextlib
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIBPATH = os.path.join(HERE, "libsohit.so")


class SoParams(C.Structure):
    _fields_ = [("seeds", C.c_char_p), ("alphabet", C.c_char_p), ("nc", C.c_int64), ("chunk", C.c_int64), ("step", C.c_int64),
                ("max_hits", C.c_int64), ("thr", C.c_int64), ("expect", C.c_double), ("max_miss", C.c_double),
                ("filter", C.c_int32), ("profile", C.c_int32)]


class SoOrthRel(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_ip", "n_ot", "n_co", "n_rows", "n_runs", "n_groups")] + \
               [("ip_a", C.POINTER(C.c_int64)), ("ip_b", C.POINTER(C.c_int64)), ("ip_v", C.POINTER(C.c_double)),
                ("ot_a", C.POINTER(C.c_int64)), ("ot_b", C.POINTER(C.c_int64)), ("ot_v", C.POINTER(C.c_double)),
                ("co_a", C.POINTER(C.c_int64)), ("co_b", C.POINTER(C.c_int64)), ("co_v", C.POINTER(C.c_double))]


class SoHit(C.Structure):
    _fields_ = [("qidx", C.c_int64), ("sidx", C.c_int64), ("identity", C.c_double), ("evalue", C.c_double), ("aln", C.c_int32),
                ("mis", C.c_int32), ("gap", C.c_int32), ("qst", C.c_int32), ("qed", C.c_int32), ("sst", C.c_int32),
                ("sed", C.c_int32), ("bit", C.c_int32), ("qlen", C.c_int32), ("slen", C.c_int32), ("matches", C.c_int32),
                ("ungapped", C.c_int32)]


class SoCounters(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_queries", "query_aa", "ref_seqs", "ref_aa", "n_chunks", "seed_windows", "seed_hits",
                                         "groups", "candidates", "alignments", "cells", "rows", "index_entries")] + \
               [("lookup_launches", C.c_int64), ("lookup_ms", C.c_double), ("lookup_bytes", C.c_int64),
                ("bounds_launches", C.c_int64), ("bounds_ms", C.c_double), ("bounds_bytes", C.c_int64),
                ("align_launches", C.c_int64), ("align_ms", C.c_double),
                ("index_ms", C.c_double), ("seed_ms", C.c_double), ("group_ms", C.c_double), ("phase2_ms", C.c_double),
                ("total_ms", C.c_double), ("count_launches", C.c_int64), ("count_ms", C.c_double),
                ("hits_bucketed", C.c_int64), ("align_wide", C.c_int64), ("cells_wide", C.c_int64), ("seed_passes", C.c_int64),
                ("ungap_steps", C.c_int64), ("groups_single", C.c_int64), ("groups_chain", C.c_int64),
                ("bgroup_launches", C.c_int64), ("bgroup_ms", C.c_double),
                ("uq_chain_queries", C.c_int64), ("uq_chain_groups", C.c_int64), ("uq_chain_overcap", C.c_int64), ("uq_left_max", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# every symbol include/sohit.h declares
EXPORTS = ["so_abi_version", "so_set_option", "so_create", "so_destroy", "so_last_error", "so_load_ref", "so_load_ref_mem", "so_build_index", "so_drop_index", "so_load_index",
           "so_load_queries", "so_load_queries_mem", "so_num_queries", "so_num_refs", "so_query_len", "so_search_loaded",
           "so_search", "so_free_hits", "so_search_loaded_aln", "so_free_aln", "so_write_sc", "so_format_hit", "so_get_counters", "so_reset_counters", "so_timing_report",
           "so_chunk_threshold", "so_chunk_entries", "so_chunk_download", "so_masked_query", "so_query_candidates", "so_query_phase2", "so_align_pairs", "so_align_pairs_aln", "so_set_profile",
           "so_bucket_count", "so_uq_chain_tier", "so_ref_len", "so_search_device", "so_device_hits_copy", "so_query_work", "so_mcl", "so_mcl_free",
           "so_mcl_last_error", "so_tsv_lines", "so_tsv_scan", "so_tsv_codes", "so_format_pairs", "so_py_repr", "so_fmt_rows",
           "so_search_loaded_cigar", "so_free_cigar", "so_format_cigar", "so_write_sc_cigar", "so_align_pairs_cigar",
           "so_apc", "so_apc_free", "so_apc_last_error", "so_cnc_groups", "so_cnc_free", "so_cnc_last_error",
           "so_orth_candidates_cols", "so_orth_candidates_records", "so_orth_free", "so_orth_last_error",
           "so_orth_relations_cols", "so_orth_relations_records", "so_orth_rel_free", "so_mcl_rows", "so_mcl_readout", "so_mcl_rows_free",
           "so_cnc_plan", "so_cnc_plan_free", "so_apc_rows", "so_apc_rows_free", "so_nr_expand", "so_nr_expand_free", "so_nr_last_error",
           "so_rbh_cols", "so_rbh_records", "so_rbh_free", "so_rbh_last_error", "so_pan_genome", "so_pan_free", "so_pan_last_error", "so_pan_shared", "so_pan_shared_free",
           "so_phyletic_pairs", "so_phyletic_free", "so_phyletic_last_error",
           "so_fusion_cols", "so_fusion_records", "so_fusion_free", "so_fusion_last_error",
           "so_operon_pairs", "so_operon_free", "so_operon_last_error", "so_phy_rows", "so_phy_build", "so_phy_free", "so_phy_last_error",
           "so_phy_boot_counts", "so_phy_nj_splits", "so_phy_boot", "so_phy_boot_free", "so_phy_subst", "so_phy_subst_free",
           "so_phy_gene", "so_phy_gene_counts", "so_phy_nj_subsets", "so_phy_gene_free",
           "so_prim_scan_path", "so_prim_sort_tier", "so_prim_seg_variant", "so_prim_scan", "so_prim_effscan", "so_prim_runs", "so_prim_number", "so_prim_sort",
           "so_prim_last_error"]


class SoMclResult(C.Structure):
    _fields_ = [("n", C.c_int64), ("nnz", C.c_int64), ("rounds", C.c_int32), ("converged", C.c_int32), ("indptr", C.POINTER(C.c_int64)),
                ("indices", C.POINTER(C.c_int32)), ("data", C.POINTER(C.c_float))]


class SoMclRowsResult(C.Structure):
    _fields_ = [("n_genes", C.c_int64), ("n_pairs", C.c_int64), ("nnz", C.c_int64), ("rounds", C.c_int32), ("converged", C.c_int32),
                ("gene", C.POINTER(C.c_int64)), ("pair_r", C.POINTER(C.c_int64)), ("pair_c", C.POINTER(C.c_int64)),
                ("indptr", C.POINTER(C.c_int64)), ("indices", C.POINTER(C.c_int32)), ("data", C.POINTER(C.c_float))]


class SoApcResult(C.Structure):
    _fields_ = [("n_genes", C.c_int64), ("n_entries", C.c_int64), ("rounds", C.c_int32), ("labels", C.POINTER(C.c_int64)),
                ("r", C.POINTER(C.c_float)), ("a", C.POINTER(C.c_float))]


class SoApcRowsResult(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_codes", "n_rows", "n_genes", "n_entries", "n_taxa_used")] + \
               [("rounds", C.c_int32), ("waits", C.c_int32), ("gene_code", C.POINTER(C.c_int32)), ("labels", C.POINTER(C.c_int64)),
                ("row", C.POINTER(C.c_int32)), ("col", C.POINTER(C.c_int32)), ("score", C.POINTER(C.c_float)), ("r", C.POINTER(C.c_float)),
                ("a", C.POINTER(C.c_float))]


class SoCncResult(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_genes", "n_rows", "n_comp1", "n_grp", "n_keep")] + \
               [("sweeps1", C.c_int32), ("sweeps2", C.c_int32), ("comp1", C.POINTER(C.c_int64)), ("grp", C.POINTER(C.c_int64)),
                ("keep", C.POINTER(C.c_uint8))]


class SoCncPlanResult(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_codes", "n_rows", "n_genes", "n_comp1", "n_grp", "n_keep", "n_cut", "n_tied")] + \
               [(n, C.c_int32) for n in ("sweeps1", "sweeps2", "sort_passes", "waits")] + \
               [(n, C.POINTER(C.c_int32)) for n in ("gene_code", "x", "y", "comp1", "grp", "order", "cut", "tied")]


class SoOrthCand(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_ot", "n_ip", "n_co", "n_rows", "n_runs", "n_groups")] + \
               [("ot_a", C.POINTER(C.c_int64)), ("ot_b", C.POINTER(C.c_int64)), ("ot_s", C.POINTER(C.c_double)),
                ("ip_a", C.POINTER(C.c_int64)), ("ip_b", C.POINTER(C.c_int64)), ("ip_s", C.POINTER(C.c_double)),
                ("co_key", C.POINTER(C.c_int64)), ("co_best", C.POINTER(C.c_double))]


class SoNrExpandResult(C.Structure):
    _fields_ = [("n_in", C.c_int64), ("n_out", C.c_int64), ("n_runs", C.c_int64), ("waits", C.c_int32), ("reserved", C.c_int32), ("d_out", C.c_void_p)]


class SoRbhResult(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_rbh", "n_core", "n_taxa", "n_runs", "n_winners", "n_runs_long", "n_rows_long")] + \
               [("waits", C.c_int32), ("reserved", C.c_int32), ("rbh_a", C.POINTER(C.c_int32)), ("rbh_b", C.POINTER(C.c_int32)),
                ("core_gene", C.POINTER(C.c_int32)), ("core_fwd", C.POINTER(C.c_int32)), ("core_rec", C.POINTER(C.c_uint8))]


class SoPanResult(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_rows", "n_taxa", "size", "n_core", "n_share", "n_spec")] + \
               [("waits", C.c_int32), ("tier", C.c_int32), ("counts", C.POINTER(C.c_int32)), ("type", C.POINTER(C.c_uint8)),
                ("core", C.POINTER(C.c_int64)), ("spec", C.POINTER(C.c_int64)), ("panz", C.POINTER(C.c_int64))]


class SoPanSharedResult(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_taxa", "n_reps", "bytes")] + \
               [("waits", C.c_int32), ("batches", C.c_int32), ("ranges", C.c_int32), ("reserved", C.c_int32), ("draw_ms", C.c_double), ("product_ms", C.c_double),
                ("shared", C.POINTER(C.c_int32))]


class SoFusionResult(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_runs", "n_eligible", "n_reps", "n_pairs", "n_disjoint", "n_links")] + \
               [("waits", C.c_int32), ("reserved", C.c_int32)] + [(n, C.c_double) for n in ("prep_ms", "keys_ms", "count_ms", "count_again_ms", "emit_ms", "sort_ms")] + \
               [("row_a", C.POINTER(C.c_int32)), ("row_b", C.POINTER(C.c_int32)), ("link", C.POINTER(C.c_int32))]


class SoPhyleticResult(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_rows", "n_eligible", "n_pairs", "tiles")] + \
               [("waits", C.c_int32), ("reserved", C.c_int32), ("count_ms", C.c_double), ("emit_ms", C.c_double), ("sort_ms", C.c_double),
                ("present", C.POINTER(C.c_int32)), ("a", C.POINTER(C.c_int32)), ("b", C.POINTER(C.c_int32)), ("shared", C.POINTER(C.c_int32))]


class SoOperonResult(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_ops", "n_pairs", "n_candidates", "n_expansions")] + \
               [("batches", C.c_int32), ("waits", C.c_int32), ("i", C.POINTER(C.c_int32)), ("j", C.POINTER(C.c_int32)),
                ("nshr", C.POINTER(C.c_int32)), ("cand_start", C.POINTER(C.c_int64))]


class SoPhyResult(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_pairs", "n_taxa", "n_cols", "n_keep")] + \
               [("waits", C.c_int32), ("reserved", C.c_int32), ("row", C.POINTER(C.c_int64)), ("matrix", C.POINTER(C.c_uint8)),
                ("gaps", C.POINTER(C.c_int32)), ("keep", C.POINTER(C.c_int32)), ("cmp", C.POINTER(C.c_int64)), ("same", C.POINTER(C.c_int64))]


class SoPhyBootResult(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_taxa", "n_reps", "n_splits", "n_words", "valid")] + \
               [("waits", C.c_int32), ("batches", C.c_int32), ("counts_ms", C.c_double), ("trees_ms", C.c_double), ("support_ms", C.c_double),
                ("cmp", C.POINTER(C.c_int64)), ("same", C.POINTER(C.c_int64)),
                ("splits", C.POINTER(C.c_uint64)), ("count", C.POINTER(C.c_int32)), ("ok", C.POINTER(C.c_uint8)),
                ("nj_tier", C.c_int32), ("reserved", C.c_int32)]


class SoPhyGeneResult(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_taxa", "n_fam", "n_splits", "n_words")] + \
               [("waits", C.c_int32), ("batches", C.c_int32), ("counts_ms", C.c_double), ("trees_ms", C.c_double), ("concord_ms", C.c_double),
                ("cmp", C.POINTER(C.c_int64)), ("same", C.POINTER(C.c_int64)), ("splits", C.POINTER(C.c_uint64)), ("present", C.POINTER(C.c_uint64)),
                ("decisive", C.POINTER(C.c_int32)), ("concordant", C.POINTER(C.c_int32)), ("n_present", C.POINTER(C.c_int32)), ("ok", C.POINTER(C.c_uint8)),
                ("nj_tier", C.c_int32), ("reserved", C.c_int32)]


class SoPhySubstResult(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_taxa", "n_pairs", "n_reps", "bytes")] + \
               [("waits", C.c_int32), ("reserved", C.c_int32), ("code_ms", C.c_double), ("product_ms", C.c_double), ("subst", C.POINTER(C.c_int32))]


_lib = None


def _preload_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's).  Two HIP
    runtimes in one process cannot both open the GPU, so whichever of torch / libsohit loads
    second would fail.  Loading torch's copy first (by path, without importing torch) makes the
    dynamic linker bind libsohit's DT_NEEDED libamdhip64.so.7 to it, and a later `import torch`
    reuses the same mapping.  Without torch installed this is a no-op (system ROCm is used)."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("SOHIT_TORCH_PRELOAD") == "0":   # ("0": a process that will never import torch -- the one-GPU CLI)
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if not spec or not spec.submodule_search_locations:
        return
    p = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.isfile(p):
        try:
            C.CDLL(p, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def result_array(p, n, dtype=None):
    """an own numpy copy of the n elements at p, a typed pointer of a result struct (never NULL, n = 0 included); dtype: the type the
    caller wants them in (None: as the library holds them).  numpy is imported here: this module loads without it (the cold find_hit)"""
    import numpy as np
    a = np.ctypeslib.as_array(p, shape=(max(int(n), 1),))[:int(n)]
    return a.astype(a.dtype if dtype is None else dtype, copy=True)


@contextlib.contextmanager
def call(fn, result_type, free, last_error, *args):
    """A device call that fills a result struct, as a `with` block around what reads it: L.<fn>(*args, byref(result)) -- a numpy array
    among args travels as its data pointer --; a non-zero return raises RuntimeError with L.<last_error>()'s message; the result is
    released by L.<free> when the block ends, whichever way."""
    L = load()
    res = result_type()
    if getattr(L, fn)(*[C.c_void_p(a.ctypes.data) if hasattr(a, 'ctypes') else a for a in args], C.byref(res)) != 0:
        raise RuntimeError(getattr(L, last_error)().decode())
    try:
        yield res
    finally:
        getattr(L, free)(C.byref(res))


def matrix2d(who, matrix):
    """-> the matrix as contiguous uint8[T, L], what the calls over a supermatrix take"""
    import numpy as np
    matrix = np.ascontiguousarray(matrix, dtype=np.uint8)
    if matrix.ndim != 2:
        raise ValueError('%s: the matrix has two dimensions' % who)
    return matrix


def load():
    """Load libsohit.so (never builds, never falls back)."""
    global _lib
    if _lib is not None:
        return _lib
    _preload_torch_hip_runtime()
    if not os.path.isfile(LIBPATH):
        raise ImportError("libsohit.so is missing (%s): run `python -m swiftortho_amd.build` -- there is no CPU fallback" % LIBPATH)
    L = C.CDLL(LIBPATH)
    vp, i64, cp = C.c_void_p, C.c_int64, C.c_char_p
    L.so_abi_version.restype = C.c_int
    L.so_create.restype = vp
    L.so_create.argtypes = [C.c_int, C.POINTER(SoParams)]
    L.so_destroy.argtypes = [vp]
    L.so_last_error.restype = cp
    L.so_last_error.argtypes = [vp]
    L.so_load_ref.argtypes = [vp, cp, i64, i64]
    L.so_load_ref_mem.argtypes = [vp, cp, i64, i64, i64]
    L.so_build_index.argtypes = [vp]
    L.so_drop_index.argtypes = [vp]
    L.so_load_index.argtypes = [vp, cp]
    L.so_load_queries.argtypes = [vp, cp]
    L.so_load_queries_mem.argtypes = [vp, cp, i64]
    for f in ("so_num_queries", "so_num_refs"):
        getattr(L, f).restype = i64
        getattr(L, f).argtypes = [vp]
    L.so_query_len.restype = i64
    L.so_query_len.argtypes = [vp, i64]
    L.so_ref_len.restype = i64
    L.so_ref_len.argtypes = [vp, i64]
    L.so_search_loaded.argtypes = [vp, i64, i64, C.POINTER(C.POINTER(SoHit)), C.POINTER(i64)]
    L.so_search.argtypes = [vp, cp, i64, i64, C.POINTER(C.POINTER(SoHit)), C.POINTER(i64)]
    L.so_free_hits.argtypes = [C.POINTER(SoHit)]
    L.so_search_loaded_aln.argtypes = [vp, i64, i64, C.POINTER(C.POINTER(SoHit)), C.POINTER(i64), C.POINTER(C.c_void_p), C.POINTER(i64)]
    L.so_free_aln.argtypes = [vp]
    L.so_search_loaded_cigar.argtypes = [vp, i64, i64, C.POINTER(C.POINTER(SoHit)), C.POINTER(i64), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.so_free_cigar.argtypes = [vp, vp]
    L.so_free_cigar.restype = None
    L.so_format_cigar.restype = i64
    L.so_format_cigar.argtypes = [vp, i64, vp, i64]
    L.so_write_sc_cigar.argtypes = [vp, C.POINTER(SoHit), i64, vp, vp, cp, cp]
    L.so_align_pairs_cigar.argtypes = [vp, C.c_int, i64, vp, vp, vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.so_search_device.argtypes = [vp, i64, i64, C.POINTER(vp), C.POINTER(i64)]
    L.so_device_hits_copy.argtypes = [vp, vp, i64]
    L.so_query_work.argtypes = [vp, i64, i64, vp]
    L.so_write_sc.argtypes = [vp, C.POINTER(SoHit), i64, cp, cp]
    L.so_format_hit.restype = i64
    L.so_format_hit.argtypes = [vp, C.POINTER(SoHit), cp, i64]
    L.so_get_counters.argtypes = [vp, C.POINTER(SoCounters)]
    L.so_set_profile.argtypes = [vp, C.c_int]
    L.so_bucket_count.restype = i64
    L.so_bucket_count.argtypes = [vp]
    L.so_uq_chain_tier.restype = i64
    L.so_uq_chain_tier.argtypes = [C.c_int]
    L.so_reset_counters.argtypes = [vp]
    L.so_timing_report.restype = i64
    L.so_timing_report.argtypes = [vp, cp, i64]
    L.so_tsv_lines.restype = i64
    L.so_tsv_lines.argtypes = [vp, i64, vp, i64]
    L.so_tsv_scan.argtypes = [vp, i64, vp, i64, C.c_int32, vp, vp, vp, vp, vp, vp, vp]
    L.so_tsv_codes.restype = i64
    L.so_tsv_codes.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, i64]
    L.so_format_pairs.restype = i64
    L.so_format_pairs.argtypes = [cp, C.c_int32, vp, vp, vp, vp, vp, i64, vp, i64]
    L.so_py_repr.restype = i64
    L.so_py_repr.argtypes = [vp, i64, vp, i64]
    L.so_fmt_rows.restype = i64
    L.so_fmt_rows.argtypes = [vp, i64, vp, i64]
    for f in ("so_chunk_threshold", "so_chunk_entries"):
        getattr(L, f).restype = i64
        getattr(L, f).argtypes = [vp, i64]
    L.so_chunk_download.argtypes = [vp, i64, vp, vp]
    L.so_masked_query.restype = i64
    L.so_masked_query.argtypes = [vp, i64, cp, i64]
    L.so_query_candidates.restype = i64
    L.so_query_candidates.argtypes = [vp, i64, vp, i64]
    L.so_query_phase2.restype = C.c_int
    L.so_query_phase2.argtypes = [vp, i64, vp]
    L.so_align_pairs.argtypes = [vp, C.c_int, i64, vp, vp, vp]
    L.so_align_pairs_aln.argtypes = [vp, C.c_int, i64, vp, vp, vp, C.POINTER(C.c_void_p), C.POINTER(i64)]
    L.so_mcl.argtypes = [C.c_int, i64, vp, vp, vp, C.c_double, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.POINTER(SoMclResult)]
    L.so_mcl_free.argtypes = [C.POINTER(SoMclResult)]
    L.so_mcl_last_error.restype = cp
    L.so_mcl_rows.argtypes = [C.c_int, i64, i64, vp, vp, vp, C.c_double, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32, C.POINTER(SoMclRowsResult)]
    L.so_mcl_readout.argtypes = [C.c_int, i64, vp, vp, vp, C.c_double, C.POINTER(SoMclRowsResult)]
    L.so_mcl_rows_free.argtypes = [C.POINTER(SoMclRowsResult)]
    L.so_apc.argtypes = [C.c_int, i64, i64, vp, vp, vp, C.c_double, C.c_int32, C.POINTER(SoApcResult)]
    L.so_apc_free.argtypes = [C.POINTER(SoApcResult)]
    L.so_apc_last_error.restype = cp
    L.so_apc_rows.argtypes = [C.c_int, i64, i64, vp, vp, vp, vp, i64, C.c_double, C.c_int32, C.c_int32, C.POINTER(SoApcRowsResult)]
    L.so_apc_rows_free.argtypes = [C.POINTER(SoApcRowsResult)]
    L.so_cnc_groups.argtypes = [C.c_int, i64, i64, vp, vp, vp, C.POINTER(SoCncResult)]
    L.so_cnc_free.argtypes = [C.POINTER(SoCncResult)]
    L.so_cnc_last_error.restype = cp
    L.so_cnc_plan.argtypes = [C.c_int, i64, i64, vp, vp, vp, C.c_int32, C.POINTER(SoCncPlanResult)]
    L.so_cnc_plan_free.argtypes = [C.POINTER(SoCncPlanResult)]
    L.so_orth_candidates_cols.argtypes = [C.c_int, i64, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, C.c_double, C.c_double, C.c_int, C.POINTER(SoOrthCand)]
    L.so_orth_candidates_records.argtypes = [C.c_int, vp, i64, vp, i64, vp, i64, i64, vp, i64, C.c_double, C.c_double, C.c_int, C.POINTER(SoOrthCand)]
    L.so_orth_free.argtypes = [C.POINTER(SoOrthCand)]
    L.so_orth_last_error.restype = cp
    L.so_orth_relations_cols.argtypes = L.so_orth_candidates_cols.argtypes[:-1] + [C.POINTER(SoOrthRel)]
    L.so_orth_relations_records.argtypes = L.so_orth_candidates_records.argtypes[:-1] + [C.POINTER(SoOrthRel)]
    L.so_orth_rel_free.argtypes = [C.POINTER(SoOrthRel)]
    L.so_nr_expand.argtypes = [C.c_int, vp, i64, vp, vp, i64, vp, vp, i64, C.c_int32, C.POINTER(SoNrExpandResult)]
    L.so_nr_expand_free.argtypes = [C.POINTER(SoNrExpandResult)]
    L.so_nr_last_error.restype = cp
    L.so_rbh_cols.argtypes = [C.c_int, i64, vp, vp, vp, i64, vp, i64, C.c_int32, C.c_int32, C.POINTER(SoRbhResult)]
    L.so_rbh_records.argtypes = [C.c_int, vp, i64, vp, i64, vp, i64, i64, vp, i64, C.c_int32, C.c_int32, C.POINTER(SoRbhResult)]
    L.so_rbh_free.argtypes = [C.POINTER(SoRbhResult)]
    L.so_rbh_last_error.restype = cp
    L.so_pan_genome.argtypes = [C.c_int, i64, vp, vp, i64, i64, i64, C.c_int32, C.c_int32, i64, vp, vp, vp, C.c_int32, C.c_int32, C.POINTER(SoPanResult)]
    L.so_pan_free.argtypes = [C.POINTER(SoPanResult)]
    L.so_pan_last_error.restype = cp
    L.so_pan_shared.argtypes = [C.c_int, i64, vp, vp, i64, i64, C.c_uint64, i64, i64, C.c_int32, C.POINTER(SoPanSharedResult)]
    L.so_pan_shared_free.argtypes = [C.POINTER(SoPanSharedResult)]
    L.so_phyletic_pairs.argtypes = [C.c_int, i64, vp, vp, i64, i64, i64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(SoPhyleticResult)]
    L.so_phyletic_free.argtypes = [C.POINTER(SoPhyleticResult)]
    L.so_phyletic_last_error.restype = cp
    L.so_fusion_cols.argtypes = [C.c_int, i64] + [vp] * 8 + [i64, vp, i64, i64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(SoFusionResult)]
    L.so_fusion_records.argtypes = [C.c_int, vp, i64, vp, i64, vp, i64, i64, vp, i64, i64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(SoFusionResult)]
    L.so_fusion_free.argtypes = [C.POINTER(SoFusionResult)]
    L.so_fusion_last_error.restype = cp
    L.so_operon_pairs.argtypes = [C.c_int, i64, vp, vp, vp, vp, i64, C.c_int32, C.POINTER(SoOperonResult)]
    L.so_operon_free.argtypes = [C.POINTER(SoOperonResult)]
    L.so_operon_last_error.restype = cp
    L.so_phy_rows.argtypes = [C.c_int, i64, vp, vp, vp, i64, vp, vp, C.c_int32, C.POINTER(SoPhyResult)]
    L.so_phy_build.argtypes = [C.c_int, i64, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, C.c_double, C.c_int32, C.POINTER(SoPhyResult)]
    L.so_phy_free.argtypes = [C.POINTER(SoPhyResult)]
    L.so_phy_last_error.restype = cp
    L.so_phy_boot_counts.argtypes = [C.c_int, i64, i64, vp, i64, vp, C.c_uint64, i64, i64, C.c_int32, C.POINTER(SoPhyBootResult)]
    L.so_phy_nj_splits.argtypes = [C.c_int, i64, i64, vp, C.c_int32, C.POINTER(SoPhyBootResult)]
    L.so_phy_boot.argtypes = [C.c_int, i64, i64, vp, i64, vp, C.c_uint64, i64, vp, C.c_int32, C.POINTER(SoPhyBootResult)]
    L.so_phy_boot_free.argtypes = [C.POINTER(SoPhyBootResult)]
    L.so_phy_subst.argtypes = [C.c_int, i64, i64, vp, i64, vp, C.c_uint64, i64, i64, C.c_int32, C.POINTER(SoPhySubstResult)]
    L.so_phy_subst_free.argtypes = [C.POINTER(SoPhySubstResult)]
    L.so_phy_gene.argtypes = [C.c_int, i64, i64, vp, i64, vp, i64, vp, vp, C.c_int32, C.POINTER(SoPhyGeneResult)]
    L.so_phy_gene_counts.argtypes = [C.c_int, i64, i64, vp, i64, vp, i64, vp, i64, i64, C.c_int32, C.POINTER(SoPhyGeneResult)]
    L.so_phy_nj_subsets.argtypes = [C.c_int, i64, i64, vp, vp, C.c_int32, C.POINTER(SoPhyGeneResult)]
    L.so_phy_gene_free.argtypes = [C.POINTER(SoPhyGeneResult)]
    i32 = C.c_int32
    L.so_prim_scan_path.restype = i32
    L.so_prim_scan_path.argtypes = [i64, vp]
    L.so_prim_sort_tier.restype = i32
    L.so_prim_sort_tier.argtypes = [i32, i64, vp, vp]
    L.so_prim_seg_variant.restype = i32
    L.so_prim_seg_variant.argtypes = [i32, i64, i64, i32]
    L.so_prim_scan.argtypes = [C.c_int, i64, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L.so_prim_effscan.argtypes = [C.c_int, i64, vp, i32, vp, i32, vp, vp, vp, vp, vp]
    L.so_prim_runs.argtypes = [C.c_int, i64, i32, vp, vp, vp, vp, vp]
    L.so_prim_number.argtypes = [C.c_int, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.so_prim_sort.argtypes = [C.c_int, i32, i64, vp, vp, i64, vp, vp, i32, i32, vp, vp, vp]
    L.so_prim_last_error.restype = cp
    L.so_set_option.argtypes = [vp, cp, cp]
    if L.so_abi_version() != 3:
        raise ImportError("libsohit.so ABI version mismatch")
    _lib = L
    return L
