/* sohit.h -- C ABI of libsohit.so, the MI355X-native replacement for SwiftOrtho's
 * seed-and-extend search core.
 *
 * What it replaces.  The reference has no in-process API for this path: its
 * bin/find_hit.py shells out to the RPython-built native `lib/fsearch-c`, one process
 * per query block (find_hit.py:119-132, 191-192), and the native's whole interface is
 * its flag list (lib/fsearch.py:3187-3188, 3215-3216) plus the 16-column row it prints
 * (fsearch.py:3242-3243).  Each entry point below therefore cites the piece of that
 * process boundary it stands in for.  bin/find_hit.py of THIS repository binds these
 * symbols with ctypes; INTEGRATION.md shows the stub a SwiftOrtho maintainer would add.
 *
 * Conventions: plain C types only; inputs are borrowed, result buffers are allocated
 * by the library and released with so_free_hits(); every function that can fail
 * returns 0 on success / non-zero on error and leaves a message retrievable with
 * so_last_error(); nothing aborts.  One so_ctx per GPU per process; a ctx is not
 * thread-safe.  There is NO CPU fallback: without a usable HIP device so_create()
 * fails.
 */
#ifndef SOHIT_H
#define SOHIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SOHIT_ABI_VERSION 3

typedef struct so_ctx so_ctx;

/* The native's flags (fsearch.py:3187-3188; defaults as driven by find_hit.py:227-228). */
typedef struct so_params {
    const char *seeds;    /* -s  comma-separated spaced-seed patterns, e.g. "111111"          */
    const char *alphabet; /* -r  reduced alphabet groups; '/' separates several alphabets     */
    int64_t nc;           /* -M  number of hash buckets NC; < 1 = the reference's default (2228-2231) */
    int64_t chunk;        /* -c  reference sequences per index chunk (fsearch.py:2283-2295)   */
    int64_t step;         /* -j  reference seed step (2244); queries always use step 1 (2658) */
    int64_t max_hits;     /* -v  rows reported per query                                      */
    int64_t thr;          /* -t  >=1 overrides the per-chunk mu+2sd seed-frequency threshold  */
    double expect;        /* -e  e-value cutoff                                               */
    double max_miss;      /* -m  early-stop ratio (fsearch.py:2970, 3052-3054)                */
    int32_t filter;       /* -F  1 = SEG-like query masking ('T'), 0 = off                    */
    int32_t profile;      /* 1 = time the headline kernels with HIP events (so_get_counters)  */
} so_params;

/* One reported alignment == one output row (fsearch.py:3074-3076, 3242-3243).
 * qst/sst are the 1-based starts exactly as printed (reference prints qst+1, sst+1). */
typedef struct so_hit {
    int64_t qidx;     /* query ordinal in the query file (column 15)            */
    int64_t sidx;     /* subject ordinal in the reference file                  */
    double identity;  /* matches * (100. / aln), full precision (column 3 is truncated text) */
    double evalue;    /* D * qlen * slen * 2^-bit (column 11)                   */
    int32_t aln;      /* alignment length (column 4)                            */
    int32_t mis;      /* non-identical columns, gaps included (column 5)        */
    int32_t gap;      /* gap "openings": ceil(run/2) per gap run (column 6)     */
    int32_t qst, qed; /* columns 7, 8                                           */
    int32_t sst, sed; /* columns 9, 10                                          */
    int32_t bit;      /* truncated integer bit score (column 12)                */
    int32_t qlen;     /* column 13                                              */
    int32_t slen;     /* column 14                                              */
    int32_t matches;  /* identical columns                                      */
    int32_t ungapped; /* ungapped (seed-stage) score of the candidate           */
} so_hit;

/* Work and time counters of the last so_build_index()/so_search*() calls. */
typedef struct so_counters {
    int64_t n_queries, query_aa;       /* queries searched, their residues                 */
    int64_t ref_seqs, ref_aa, n_chunks;
    int64_t seed_windows;              /* query seed windows hashed                        */
    int64_t seed_hits;                 /* index entries visited by the lookup kernel (H)   */
    int64_t groups;                    /* distinct (subject, diagonal) groups              */
    int64_t candidates;                /* candidates with ungapped score >= 25             */
    int64_t alignments;                /* banded alignments computed                       */
    int64_t cells;                     /* banded DP cells computed                         */
    int64_t rows;                      /* reported rows                                    */
    int64_t index_entries;             /* sum of index entries over chunks                 */
    /* headline-kernel timing (HIP events on the ctx stream; only when params.profile)     */
    int64_t lookup_launches;           /* launches of the seed-lookup kernel               */
    double lookup_ms;                  /* their summed duration                            */
    int64_t lookup_bytes;              /* algorithmic bytes read by them       */
    int64_t bounds_launches;           /* launches of the query hash+bucket-bounds kernel  */
    double bounds_ms;
    int64_t bounds_bytes;
    int64_t align_launches;
    double align_ms;
    double index_ms, seed_ms, group_ms, phase2_ms, total_ms; /* host-side stage wall times */
    int64_t count_launches;            /* launches of the lookup kernel's COUNT pass (bucketed binning) */
    double count_ms;                   /* their summed duration; lookup_* then describe its SCATTER pass */
    /* which path the work took (round 4: both are per-task / per-pass decisions, not per-batch ones) */
    int64_t hits_bucketed;             /* seed hits binned by the bucketed passes (k_bkt_pass); the rest took the sorted path */
    int64_t align_wide;                /* score-only alignments the packed 16-bit aligner could not take (32-bit kernel)       */
    int64_t cells_wide;                /* their band cells (`cells` counts every task of the early-stop rounds once)            */
    int64_t seed_passes;               /* seed passes run (one per length class and chunk; sparse neighbouring classes share one) */
    /* round 5 (ABI 2).  With SOHIT_UG_COUNT=1 in the environment of so_create the extension kernels run their counting instances: */
    int64_t ungap_steps;               /* b62 lookups of the ungapped extension = the reference's `flag` (fsearch.py:2467, 2482)  */
    int64_t groups_single;             /* groups of one seed hit, extended by k_ungap1                                            */
    int64_t groups_chain;              /* groups of two and more hits, chained by k_ungap2 (the rest of `groups`: k_ungap)        */
    /* round 6 (ABI 3): the third kernel of the seed-lookup + diagonal-binning stage, so that the STAGE (count + scatter + grouping) can be
     * priced against the HBM roofline, not one pass of it (params.profile) */
    int64_t bgroup_launches;           /* launches of the bucket grouping kernel (k_bkt_group)                                    */
    double bgroup_ms;                  /* their summed duration                                                                   */
    /* sparse passes whose leftover hits (the ones k_ungapq does not extend itself) are sorted per query on chip -- a wave's registers, a
     * workgroup's LDS for long lists -- and chained from the list of their group heads (SOHIT_UQ_CHAINS); such groups count into `groups`
     * only.  Appended like the fields above: so_abi_version stays 3, a caller built against the shorter struct must not pass it here. */
    int64_t uq_chain_queries;          /* queries with leftover hits that took this flow                                          */
    int64_t uq_chain_groups;           /* their groups                                                                            */
    int64_t uq_chain_overcap;          /* ... of them, queries above the largest LDS tier (sorted in place in the key array)      */
    int64_t uq_left_max;               /* most leftover hits of one query in one pass                                             */
} so_counters;

/* Lifetime.  Replaces: spawning `fsearch-c` with its flags (find_hit.py:119-123). */
so_ctx *so_create(int device, const so_params *params);
void so_destroy(so_ctx *ctx);
const char *so_last_error(const so_ctx *ctx); /* ctx may be NULL: last so_create() error */
int so_abi_version(void);
/* One tuning / diagnostic switch (the SOHIT_* names of swiftortho_amd/csrc/tune.h, with or without the prefix; none changes results) for
 * this context from now on.  so_create reads the same names from the environment once. */
int so_set_option(so_ctx *ctx, const char *name, const char *value);

/* Reference side.  Replaces: Fasta(open(ref)) + DB.makedb()/build_msav() per chunk
 * (fsearch.py:2975-2979, 2990, 2208-2295).  r_lo/r_hi are -L/-U (-1 = all).
 * so_load_ref* parses the FASTA and makes the residues resident in HBM;
 * so_build_index builds every chunk's index on the device (idempotent until the next load). */
int so_load_ref(so_ctx *ctx, const char *fasta_path, int64_t r_lo, int64_t r_hi);
int so_load_ref_mem(so_ctx *ctx, const char *fasta_bytes, int64_t nbytes, int64_t r_lo, int64_t r_hi);
int so_build_index(so_ctx *ctx);
int so_drop_index(so_ctx *ctx); /* forget the built chunk indexes (residues stay resident) */
/* Replaces: Fasta.load (fsearch.py:2355-2444).  Reads the chunk indexes `<prefix>.<k>.idx / .soas / .bin`, k = 0, 1, ... (the files
 * Fasta.write produces, fsearch.py:2298-2352; swiftortho_amd.fsearch.makedb writes the same bytes) and makes them resident in place
 * of a built index: locus slots -> entries, start[] -> bucket directory, threshold from the .bin trailer.  As in the reference the
 * files hold no sequences -- so_load_ref() the FASTA file first -- and the context must have been created with the trailer's -M, -s
 * and -r (an error otherwise, as when sequence lengths and the .soas file disagree).  Searches then run from the loaded chunks until
 * the next so_load_ref / so_drop_index. */
int so_load_index(so_ctx *ctx, const char *prefix);

/* Query side.  Replaces: Fasta(open(qry)) (fsearch.py:2971-2973).  Parses the FASTA and
 * makes the query residues resident in HBM. */
int so_load_queries(so_ctx *ctx, const char *fasta_path);
int so_load_queries_mem(so_ctx *ctx, const char *fasta_bytes, int64_t nbytes);
int64_t so_num_queries(const so_ctx *ctx);
int64_t so_num_refs(const so_ctx *ctx);
int64_t so_query_len(const so_ctx *ctx, int64_t qidx);
int64_t so_ref_len(const so_ctx *ctx, int64_t sidx); /* residues of reference sequence sidx (the index exporter's `soas`) */

/* The search.  Replaces: blastp(qry, ref, ..., st=-l, ed=-u) (fsearch.py:2968-3121):
 * queries [q_lo, q_hi) of the loaded query file against the loaded reference; rows come
 * back in the order the reference yields them (ascending query, descending bit).
 * so_search() = so_load_queries() + so_build_index() (if needed) + so_search_loaded(). */
int so_search_loaded(so_ctx *ctx, int64_t q_lo, int64_t q_hi, so_hit **hits, int64_t *n_hits);
int so_search(so_ctx *ctx, const char *qry_fasta_path, int64_t q_lo, int64_t q_hi, so_hit **hits, int64_t *n_hits);
/* Releases a result array.  The library may keep ONE released array (the largest between 1 MiB and 2 GiB) for the next search of this process
 * instead of returning its pages to the system -- a 100k-protein result is 130 MB and unmapping + refaulting it costs ~17 ms per
 * search; so_destroy() drops it, SOHIT_HIT_CACHE=0 disables it. */
void so_free_hits(so_hit *hits);

/* The search with the alignment behind every row.  Same rows as so_search_loaded() (same kernels and bytes); in addition
 * *aln holds 2 * sum(hits[k].aln) bytes (*aln_bytes): row k's query string starts at byte 2 * sum_{m<k} hits[m].aln and
 * is hits[k].aln bytes long, its subject string follows it.  The strings are kswat_st's al0 / al1 (fsearch.py:1417-1444,
 * 3066-3070: al0 is the query side): the residues qst..qed of the query as the aligner saw it (SEG-masked when filtering is
 * on, as fsearch.py:2963 hands it over) and sst..sed of the subject, in order, with '-' in every column where the other
 * side advances alone.  A row of a 4096-wide tile (kswat_st_long, fsearch.py:1480-1498) carries its tile's strings.
 * The row statistics follow from the strings as in fsearch.py:1454-1471.  Released with so_free_aln(). */
int so_search_loaded_aln(so_ctx *ctx, int64_t q_lo, int64_t q_hi, so_hit **hits, int64_t *n_hits, char **aln, int64_t *aln_bytes);
void so_free_aln(char *aln);

/* The search with a CIGAR behind every row.  Same rows as so_search_loaded() (same kernels and bytes); in addition row k's
 * alignment path is ops[op_off[k] .. op_off[k + 1]) (op_off holds *n_hits + 1 offsets, op_off[0] = 0): one uint32 per run,
 * length << 4 | op with op 0 = M (both sides advance; match or mismatch), 1 = I (the query advances alone), 2 = D (the subject
 * advances alone) -- the BAM packing --, first column first.  Canonical: no run of length 0, neighbouring runs differ in op.
 * Per row: the lengths add up to hits[k].aln, the M + I lengths to qed - qst + 1, the M + D lengths to sed - sst + 1.  The runs
 * are coded on the GPU from the columns the traceback walks write; they describe the same path as so_search_loaded_aln()'s
 * strings (a row of a 4096-wide tile carries its tile's path) and, unlike the strings, stay unambiguous where a sequence holds a
 * literal '-' residue.  One call gives strings or CIGARs, not both.  Released with so_free_cigar().
 * so_format_cigar() renders runs as text, "<length><op>" per run with nothing between (35M2D10M): returns the length of the
 * text and writes at most cap - 1 characters and a NUL into buf (buf may be NULL); -1 for a run of length 0 or an unknown op.
 * Host-only: needs no ctx and no device. */
int so_search_loaded_cigar(so_ctx *ctx, int64_t q_lo, int64_t q_hi, so_hit **hits, int64_t *n_hits, uint32_t **ops, int64_t **op_off);
void so_free_cigar(uint32_t *ops, int64_t *op_off);
int64_t so_format_cigar(const uint32_t *ops, int64_t n_ops, char *buf, int64_t cap);

/* Multi-GPU support.  The reference runs one fsearch-c process per query block and joins the part files with `cat`
 * (find_hit.py:107-146); here one process per GPU searches a query shard and the hit records are exchanged over RCCL, so
 * they must be able to stay in HBM until after the exchange:
 * so_search_device() = so_search_loaded() whose so_hit records (same 80-byte layout, same values) are left in device
 * memory owned by the ctx (*d_hits, valid until the next so_search* call on the ctx or so_destroy);
 * so_device_hits_copy() copies the first n_hits of them device-to-device into a caller-owned device buffer (e.g. the
 * send buffer of a collective).
 * so_query_work() fills work[0 .. q_hi-q_lo) with the number of index entries each query visits over all chunks (one
 * hash + bucket-bounds + frequency-cap pre-pass, no search): the cost estimate used to balance query shards. */
int so_search_device(so_ctx *ctx, int64_t q_lo, int64_t q_hi, const so_hit **d_hits, int64_t *n_hits);
int so_device_hits_copy(so_ctx *ctx, void *dst_device, int64_t n_hits);
int so_query_work(so_ctx *ctx, int64_t q_lo, int64_t q_hi, uint64_t *work);

/* Output.  Replaces: the row formatter of entry_point (fsearch.py:3234-3258; f2s 43-61):
 * writes the 16-column tab-separated rows for hits of the currently loaded query and
 * reference files.  mode "w" or "a" (-O).  so_format_hit() renders one row into buf. */
int so_write_sc(so_ctx *ctx, const so_hit *hits, int64_t n_hits, const char *path, const char *mode);
int64_t so_format_hit(so_ctx *ctx, const so_hit *hit, char *buf, int64_t cap);
/* so_write_sc() with a 17th column: every row's first 16 columns are so_write_sc()'s bytes, followed by a tab and the row's CIGAR
 * as so_format_cigar() renders it (ops / op_off as so_search_loaded_cigar() returns them). */
int so_write_sc_cigar(so_ctx *ctx, const so_hit *hits, int64_t n_hits, const uint32_t *ops, const int64_t *op_off, const char *path,
                      const char *mode);

/* Introspection (tests, bench). */
/* switch params.profile (HIP-event kernel timers + stage laps, which synchronise the stream) on or off */
int so_set_profile(so_ctx *ctx, int on);
/* NC actually in use: -M, or the reference's `bins` default when -M < 1 (fsearch.py:2228-2231) */
int64_t so_bucket_count(const so_ctx *ctx);
/* Leftover hits per query the chain flow's wave tier (0) and workgroup tier (1) sort in LDS. */
int64_t so_uq_chain_tier(int tier);
/* Host-only helper of the row formatter (tests): for v[0..n) writes "<%f of v>\t<f2s(v)>\n" lines (f2s: fsearch.py:43-61) into out;
 * returns the bytes written or -1 when cap is too small (allow 1400 per value). */
int64_t so_fmt_rows(const double *v, int64_t n, char *out, int64_t cap);
int so_get_counters(const so_ctx *ctx, so_counters *out);
int so_reset_counters(so_ctx *ctx);
/* "stage=ms;stage=ms;..." wall-clock laps of the pipeline stages (only with params.profile) */
int64_t so_timing_report(const so_ctx *ctx, char *buf, int64_t cap);
int64_t so_chunk_threshold(const so_ctx *ctx, int64_t chunk);
int64_t so_chunk_entries(const so_ctx *ctx, int64_t chunk);
/* copies start[0..NC] (uint32, NC+1 values) / entries (uint64) of one chunk's index to host, every bucket's members in descending entry
 * order -- the slot order of the reference's CSR (fsearch.py:2240-2266) and of its index files.  (The build's grouping kernels place a
 * bucket's members with atomics; they are put in order by the chunk's first dense seed pass or by this call, whichever comes first.) */
int so_chunk_download(so_ctx *ctx, int64_t chunk, uint32_t *start, uint64_t *entries);
/* masked (SEG-filtered, upper-cased) bytes of query qidx as used for seeding and alignment */
int64_t so_masked_query(so_ctx *ctx, int64_t qidx, char *buf, int64_t cap);
/* candidates [subject, ungapped score, qi, qj] x uint32 of query qidx from the last
 * so_search_loaded() call, in the order the reference's spill file holds them (chunk-major) */
int64_t so_query_candidates(so_ctx *ctx, int64_t qidx, uint32_t *out4, int64_t cap);
/* tests (kept under the same switch as the candidates, SOHIT_KEEP_CANDS): query qidx's phase-2 state behind the alignment rounds of the
 * last so_search_loaded() call -- out[0..4] = next rank, consecutive misses, passing tiles, selected tiles, stopped; out[5] = ranks
 * considered (top vmax), out[6] = their alignment tasks, out[7] = band cells of the tasks aligned.  0, or -1 without a kept state. */
int so_query_phase2(so_ctx *ctx, int64_t qidx, int64_t out[8]);
/* tests: align explicit windows with ONE phase-2 aligner (not used by the search).  Queries are the loaded query file (raw residues, no
 * masking), subjects the loaded reference.
 * task6: n x {qidx, sidx, qi, qj, qe, se}: windows [qi, qe) of the query and [qj, se) of the subject, aligned from (qi, qj) as kswat_st does;
 *   qe / se = -1: the sequence's end (otherwise a kswat_st_long tile end; a window holds at most 4096 residues).
 * kernel: 0 k_align<false>, 1 k_align_pk<false>, 2 k_align_lane, 3 k_align<true> + k_traceback, 4 k_align_pk<true> + k_traceback
 *   (traced: variable trace offsets, as the final emission lays them out).
 * order: the launch list (n positions, any permutation or repeats of 0 .. n-1; traced kernels: every task once) or NULL = 0 .. n-1.
 * out: n x {maxscore, aln, matches, gap, qst, qed, sst, sed, cells, wide} per TASK (all -1 for a task the list does not hold): qst / sst
 *   0-based exclusive starts as kswat_st returns them; aln ... sed only from the traced kernels; wide = 1 when k_task_rows would send the
 *   task to the 32-bit kernel.
 * Refused, with a message and nothing written: a packed kernel (1, 2, 4) on a wide task, k_align_lane on a tile or on a sequence of 4096
 * residues or more, windows out of range. */
int so_align_pairs(so_ctx *ctx, int kernel, int64_t n, const int64_t *task6, const uint32_t *order, int32_t *out);
/* tests: so_align_pairs for the traced kernels (3, 4) that also returns every task's alignment, built by the search's own emission chain
 * (column slots, the emitting walk, compaction, the host decoder).  *aln holds 2 * sum(aln_t) bytes (*aln_bytes): task t's query string
 * starts at byte 2 * sum_{m<t} aln_m and is aln_t bytes long, its subject string follows it (as so_search_loaded_aln lays out rows).
 * Same tasks, order and refusals as so_align_pairs; released with so_free_aln(). */
int so_align_pairs_aln(so_ctx *ctx, int kernel, int64_t n, const int64_t *task6, const uint32_t *order, int32_t *out, char **aln,
                       int64_t *aln_bytes);

/* tests: so_align_pairs for the traced kernels (3, 4) that also returns every task's CIGAR, built by the search's own chain (column
 * slots, the emitting walk, the run counting, scan and run emitting kernels): task t's runs are ops[op_off[t] .. op_off[t + 1])
 * (op_off: n + 1), packed as so_search_loaded_cigar() packs them; a task without an alignment has no runs.  Same tasks, order and
 * refusals as so_align_pairs; released with so_free_cigar(). */
int so_align_pairs_cigar(so_ctx *ctx, int kernel, int64_t n, const int64_t *task6, const uint32_t *order, int32_t *out, uint32_t **ops,
                         int64_t **op_off);

/* Markov clustering of one block of the orthology graph.  Replaces: the matrix loop of bin/find_cluster.py
 * `mcl` (652-689) with `normalize` (636-646) as `mcl_xyz` (1425-1467) calls it on a float32 scipy csr_matrix -- column
 * normalisation, expansion (sparse x sparse), inflation, pruning below `prune`, at most max_rounds rounds, convergence test
 * every check_every-th round -- with scipy's arithmetic order (csrc/mcl.hip).  Input: an n x n CSR matrix (rows = indptr,
 * columns = indices, float32 data; inputs are borrowed).  Output: the matrix the loop ends with, in scipy's storage order and
 * with its explicitly stored zeros (the reference's read-out depends on both); arrays allocated by the library, released with
 * so_mcl_free().  Returns 0 / non-zero with a message in so_mcl_last_error().  No so_ctx: the call owns a stream of `device`
 * and reads the SOHIT_* switches itself (SOHIT_POISON, SOHIT_MCL_SCRATCH; so_apc: SOHIT_POISON).  check_every below 1 counts as 1;
 * an empty block (n = 0) is served: nothing moves, so the first convergence test succeeds. */
typedef struct so_mcl_result {
    int64_t n, nnz;
    int32_t rounds;    /* rounds executed                                  */
    int32_t converged; /* 1 = left the loop through the convergence test   */
    int64_t *indptr;   /* n + 1                                            */
    int32_t *indices;  /* nnz                                              */
    float *data;       /* nnz                                              */
} so_mcl_result;
int so_mcl(int device, int64_t n, const int64_t *indptr, const int32_t *indices, const float *data, double inflation, int32_t max_rounds,
           int32_t check_every, double prune, double rtol, double atol, so_mcl_result *out);
void so_mcl_free(so_mcl_result *result);
const char *so_mcl_last_error(void);

/* One batch of `find_cluster -a mcl` from its rows to its surviving pairs on the device (csrc/mcl.hip): the matrix never exists on the
 * host.  Replaces: the matrix `mcl_xyz` of bin/find_cluster.py (1425-1467) builds for a batch, as swiftortho_amd/find_cluster.py
 * `block_matrix_arrays()` restates it bit for bit, the upload, the loop of so_mcl, the download of the final matrix and the read-out
 * of `mcl` (686-689) as `surviving_pair_columns()` restates it, shifted pairing included.
 * Input: n_rows rows in batch order (host arrays, borrowed): gene labels gx / gy in 0 .. n_labels - 1 (any labelling; labels may be
 * unused), float64 weights z; the loop's parameters as so_mcl takes them (max_rounds = 0 skips the loop); flags & 1: the assembled matrix
 * comes back too.
 * Assembly: genes numbered by first appearance in x0, y0, x1, y1, ...; a (n_genes + 1)^2 matrix with an empty last row; weights rounded
 * to float32 once (nearest even, overflow = +-inf, denormals kept); per ordered pair the LAST row wins, (x, y) and (y, x) both stored;
 * the diagonal of a gene = the largest positive weight of any of its rows, overwritten repeats included, stored only where it is above
 * 0 (a denormal is, -0.0 is not); zeros of either sign are not stored; canonical CSR, columns ascending.
 * Read-out: the k-th non-zero entry in storage order gives the k-th coordinate, kept when the k-th RAW stored value exceeds
 * (float)prune; a NaN is non-zero and exceeds nothing, -0.0 is a zero.
 * Output (allocated by the library, released with so_mcl_rows_free()): gene[n_genes] = the label of matrix row k; rounds / converged
 * as so_mcl reports them; pair_r / pair_c[n_pairs] in read-out order; with flags & 1 the matrix as it entered the loop: indptr[n_genes + 2],
 * indices / data[nnz].  n_rows = 0 is served without a launch (no gene, no round, no pair, indptr = {0, 0}).
 * Refused with a message (so_mcl_last_error), nothing further launched and nothing left allocated: negative counts, n_labels or n_rows
 * >= 2^31, a label outside 0 .. n_labels - 1, a NaN weight, a row with x == y (the reference overwrites the diagonal in line order: the
 * host's sequential builder is the only implementation), no HIP device -- all before a device is touched -- and, found on the device
 * as equal neighbours of the sorted entries, a batch in which both (a, b) and (b, a) occur (numpy stores the coordinate twice); a
 * matrix of more than 2^31 - 16 entries.  No so_ctx: the call owns a stream of `device` and reads the SOHIT_* switches itself
 * (SOHIT_POISON, SOHIT_MCL_SCRATCH).
 * so_mcl_readout: the read-out kernels alone on an n x n host CSR (borrowed; stored zeros and any column order allowed) -> n_pairs,
 * pair_r, pair_c of the same structure, everything else 0.  Refused: n < 0, row pointers that do not start at 0 or that fall, more
 * than 2^31 - 16 entries, no HIP device. */
typedef struct so_mcl_rows_result {
    int64_t n_genes, n_pairs, nnz;
    int32_t rounds;    /* rounds executed                                  */
    int32_t converged; /* 1 = left the loop through the convergence test   */
    int64_t *gene;     /* n_genes                                          */
    int64_t *pair_r;   /* n_pairs                                          */
    int64_t *pair_c;
    int64_t *indptr;   /* flags & 1: n_genes + 2, else NULL                */
    int32_t *indices;  /* flags & 1: nnz                                   */
    float *data;       /* flags & 1: nnz                                   */
} so_mcl_rows_result;
int so_mcl_rows(int device, int64_t n_labels, int64_t n_rows, const int64_t *gx, const int64_t *gy, const double *z, double inflation,
                int32_t max_rounds, int32_t check_every, double prune, double rtol, double atol, int32_t flags, so_mcl_rows_result *out);
int so_mcl_readout(int device, int64_t n, const int64_t *indptr, const int32_t *indices, const float *data, double prune,
                   so_mcl_rows_result *out_pairs);
void so_mcl_rows_free(so_mcl_rows_result *result);

/* Affinity propagation on the edge list of the orthology graph.  Replaces: the loop of bin/find_cluster.py `apclust_blk` (404-513)
 * with its passes `max_row`, `update_R`, `sum_col`, `update_A`, `get_change` (309-401), which `main` runs for `-a apc` with a batch
 * size above zero -- in the reference's arithmetic order (csrc/apc.hip): float64 operations on float32-stored R and A, row maxima
 * carried over all rounds, column sums added in entry order, the first maximum of a row gives its label; always `rounds` rounds
 * (the reference's convergence counter never moves on this path).  Input: n_entries entries (row, col, score) in the reference's
 * order (borrowed), gene numbers in 0 .. n_genes - 1; repeated entries are entries of their own.  n_genes above 2^24 is refused
 * (the reference keeps gene numbers in float32 there).  `damp` is used as given.  Output: labels[n_genes] = the exemplar of every
 * gene (a gene without entries keeps its own number), r / a[n_entries] = the float32 stores after the last round, in entry order;
 * allocated by the library, released with so_apc_free().  Returns 0 / non-zero with a message in so_apc_last_error().  No so_ctx:
 * the call owns a stream of `device` and queues all rounds on it. */
typedef struct so_apc_result {
    int64_t n_genes, n_entries;
    int32_t rounds;
    int64_t *labels;
    float *r;
    float *a;
} so_apc_result;
int so_apc(int device, int64_t n_genes, int64_t n_entries, const int32_t *row, const int32_t *col, const float *score, double damp,
           int32_t rounds, so_apc_result *out);
void so_apc_free(so_apc_result *result);
const char *so_apc_last_error(void);

/* `find_cluster -a apc` from id-coded rows to exemplar labels in one device call (csrc/apc.hip).  Replaces: the column half of
 * fc2mat (767-858) -- gene numbers, the mirrored entries, the preference entries -- as swiftortho_amd/find_cluster.py
 * `apc_entry_columns()` restates it, field for field, and then the loop of so_apc on those entries, bit for bit.
 * Input: n_rows rows in file order (host arrays, borrowed): id codes cx <= cy in 0 .. n_codes - 1 (code order = the ids' byte order;
 * codes may be unused), float64 weights z (a NaN or an infinite weight is served: the loop defines what it does with them),
 * taxon_of_code[n_codes] = a code in 0 .. n_taxa - 1 of the id's text before its first '|'.  Genes are numbered by first appearance
 * in cx0, cy0, cx1, cy1, ...; entry 2r = (X_r, Y_r, float32(z_r)), entry 2r + 1 = (Y_r, X_r, float32(z_r)), entry 2 n_rows + g =
 * (g, g, float32(-20.0 * n_taxa_used)), n_taxa_used = the distinct taxon codes of the numbered genes.  The entry list never exists:
 * the row / column layout of the loop is built from the rows on the device.
 * Output: gene_code[n_genes] = the code of gene g, labels[n_genes] = its exemplar; R and A stay on the device.  With flags & 1 also
 * row, col, score, r, a [n_entries] in ENTRY order (the tests' view; otherwise NULL).  Arrays allocated by the library, released with
 * so_apc_rows_free().  `waits` = host waits of the call (the number of genes, the list lengths, the end: none per round).
 * n_rows = 0 is served without a launch (no gene, no entry, n_taxa_used = 0).  Refused before a device is touched: negative counts,
 * n_codes / n_rows / n_taxa of 2^31 and more, a code or a taxon code out of range, a row with cx > cy, 2 n_rows + n_codes above
 * 0x7FFFFFF0, no HIP device; after numbering: more than 2^24 genes (so_apc's rule).  Returns 0 / non-zero with a message in
 * so_apc_last_error().  No so_ctx: the call owns a stream of `device` and reads SOHIT_POISON itself. */
typedef struct so_apc_rows_result {
    int64_t n_codes, n_rows, n_genes, n_entries, n_taxa_used;
    int32_t rounds, waits;
    int32_t *gene_code; /* n_genes                                          */
    int64_t *labels;    /* n_genes                                          */
    int32_t *row;       /* n_entries, flags & 1 only (as col, score, r, a)  */
    int32_t *col;
    float *score;
    float *r;
    float *a;
} so_apc_rows_result;
int so_apc_rows(int device, int64_t n_codes, int64_t n_rows, const int32_t *cx, const int32_t *cy, const double *z,
                const int32_t *taxon_of_code, int64_t n_taxa, double damp, int32_t rounds, int32_t flags, so_apc_rows_result *out);
void so_apc_rows_free(so_apc_rows_result *result);

/* The component stage of `find_cluster -a mcl` on the device (csrc/cnc.hip).  Replaces: the first half of bin/find_cluster.py `cnc`
 * (1470-1590) -- every gene linked to its best-scoring neighbours, the connected components of those links numbered (level 1), the
 * components joined by a row whose two component numbers are non-zero merged and numbered (level 2), the rows inside one level-2
 * group other than group 0 kept -- as swiftortho_amd/find_cluster.py `group_numbers()` restates it, number for number.
 * Input: n_rows rows in file order (host arrays, borrowed): gene numbers x / y in 0 .. n_genes - 1, genes numbered by first
 * appearance (x of a row before its y), so every gene occurs in some row; float64 weights z.  -0.0 ties with +0.0, +inf and -inf are
 * ordinary weights.
 * Output (allocated by the library, released with so_cnc_free()): comp1[n_genes] = the number of level-1 components whose largest gene
 * exceeds that of the gene's own (component 0 holds gene n_genes - 1); grp[n_genes] = the rank, in file order, of the first row with
 * two non-zero component numbers that touches the gene's level-2 component, -1 for the genes of component 0 and of components no such
 * row touches; keep[n_rows] = 1 where grp[x] == grp[y] and that number is not 0.  n_comp1 / n_grp: level-1 components / level-2
 * groups; n_keep: rows kept; sweeps1 / sweeps2: label sweeps of the two levels, the confirming one included (diagnostic: they may
 * differ between two runs of one input, the arrays may not).  n_genes = 0 or n_rows = 0 is served and launches nothing (comp1 0,
 * grp -1); so is level 2 of an input with a single level-1 component (sweeps2 = 0).
 * Refused with a message (so_cnc_last_error), nothing launched and nothing left allocated: negative counts, n_genes or n_rows >= 2^31,
 * a gene number outside 0 .. n_genes - 1, a gene without a row, a NaN weight (numpy's answer to it has no integer order: the caller
 * keeps the host stage), no HIP device.  Labels that still move after nodes + 2 sweeps are an error, never a truncated answer.  No
 * so_ctx: the call owns a stream of `device` and reads the SOHIT_* switches itself (SOHIT_POISON). */
typedef struct so_cnc_result {
    int64_t n_genes, n_rows, n_comp1, n_grp, n_keep;
    int32_t sweeps1, sweeps2;
    int64_t *comp1, *grp;
    uint8_t *keep;        /* one byte per row */
} so_cnc_result;
int so_cnc_groups(int device, int64_t n_genes, int64_t n_rows, const int32_t *x, const int32_t *y, const double *z,
                  so_cnc_result *out);
void so_cnc_free(so_cnc_result *result);
const char *so_cnc_last_error(void);

/* The row plan of `find_cluster -a mcl` on the device (csrc/cnc.hip): one call from the id codes of the rows to everything cnc needs
 * before its batches.  Replaces: the part of bin/find_cluster.py `cnc` between reading the rows and `mcl_xyz` -- the gene dictionary
 * (numbered by first appearance), the component stage of so_cnc_groups, the selection of the kept rows and the `LC_ALL=C sort -n` of
 * the group-tagged lines (1590-1640) -- as swiftortho_amd/find_cluster.py `row_plan()` restates it, number for number.
 * Input: n_rows rows in file order (host arrays, borrowed) with cx <= cy: id codes in 0 .. n_codes - 1 whose order is the byte order of
 * the ids (codes may be unused), float64 weights z.  flags & 1: the order is made by two stable sort passes -- (cx, cy), then the group
 * -- also where the three fields fit one 64-bit key (bits(n_grp + 1) + 2 bits(n_codes) <= 64), which otherwise takes one pass.
 * Output (allocated by the library, released with so_cnc_plan_free()): gene_code[n_genes] = the codes in order of first appearance in
 * cx0, cy0, cx1, ...; x / y[n_rows] = the gene numbers of the rows; comp1 / grp[n_genes] as so_cnc_groups defines them; order[n_keep] =
 * the rows with grp[x] == grp[y] != 0, sorted by (grp as a signed number: the pool -1 first, cx, cy), rows with an equal triple in file
 * order; cut[n_cut] = the positions p >= 1 of `order` whose grp differs from that of p - 1; tied[n_tied] = the positions p >= 1 whose
 * (grp, cx, cy) equals that of p - 1.  sort_passes: 1 or 2 (0: no row kept); waits: host waits of the call -- one each for the number
 * of genes, of level-1 roots, of kept rows (with the number of groups), of cuts and ties (the arrays up to `order` arrive with it) and
 * one for cut / tied when there are any, plus one per label sweep (sweeps1 + sweeps2; level 2 is skipped when there is one level-1
 * component).  n_rows = 0 is served without a launch (nothing numbered, nothing kept).
 * Refused with a message (so_cnc_last_error), nothing launched and nothing left allocated: negative counts, n_codes or n_rows >= 2^31,
 * a code outside 0 .. n_codes - 1, a row with cx > cy, a NaN weight (the caller keeps the numpy plan), no HIP device.  Integer atomics
 * only: no value depends on scheduling.  No so_ctx: the call owns a stream of `device` and reads the SOHIT_* switches itself
 * (SOHIT_POISON). */
typedef struct so_cnc_plan_result {
    int64_t n_codes, n_rows, n_genes, n_comp1, n_grp, n_keep, n_cut, n_tied;
    int32_t sweeps1, sweeps2, sort_passes, waits;
    int32_t *gene_code;   /* n_genes */
    int32_t *x, *y;       /* n_rows  */
    int32_t *comp1, *grp; /* n_genes */
    int32_t *order;       /* n_keep  */
    int32_t *cut;         /* n_cut   */
    int32_t *tied;        /* n_tied  */
} so_cnc_plan_result;
int so_cnc_plan(int device, int64_t n_codes, int64_t n_rows, const int32_t *cx, const int32_t *cy, const double *z, int32_t flags,
                so_cnc_plan_result *out);
void so_cnc_plan_free(so_cnc_plan_result *result);

/* The candidate stage of find_orth on the device (csrc/orth.hip).  Replaces: the row loop of bin/find_orth.py -- coverage / identity
 * filter and -n normalisation (156-234), per query run the best hit per subject, the best score per subject taxon and out of the
 * query's taxon, the in-paralog / ortholog / co-ortholog candidates (298-348) and "a pair is a relation iff proposed exactly twice"
 * (351-377) -- as swiftortho_amd/find_orth.py `candidates()` restates it, bit for bit.
 * Input: n hit rows in file order -- name codes q / s in 0 .. n_names - 1 and the six float64 columns (host arrays, borrowed), or
 * so_hit records in DEVICE memory (d_hits: the pointer so_search_device hands out, or any device buffer of records such as the tensor
 * gathered on rank 0) with the host maps query ordinal -> code (qmap, n_q) and subject ordinal -> code (smap, n_s); the identity
 * column of a record is cut to the two decimals its text row carries.  tax[n_names]: taxon code of every name, in 0 .. n_taxa - 1.
 * norm: 0 = no, 1 = bsr, 2 = bal.
 * Output (allocated by the library, released with so_orth_free()): ot_* / ip_*: the ortholog / in-paralog pairs proposed exactly twice,
 * ascending by (a, b), in-paralogs in both orientations, scored with the mean of the two proposals -- the last proposed pair of each
 * list, when it is among them, with the larger one; co_key / co_best: the distinct keys a * max(n_names, 1) + b of the co-ortholog
 * candidates, ascending, and their best scores; n_rows rows passed the filter, in n_runs runs of one query code, with n_groups distinct
 * (run, subject).  n = 0 is served and launches nothing.
 * Ordering: the records call reads d_hits on a stream of its own.  It first waits for ALL work queued on the device, so records
 * written by any stream before the call are complete (so_search_device has synchronised its stream when it returns); work queued
 * from another thread while the call runs is not ordered with it.  The records are only read.
 * Refused with a message (so_orth_last_error): n >= 2^31, n_names * n_names >= 2^63, a name code outside 0 .. n_names - 1, a qidx /
 * sidx outside its map, a taxon outside 0 .. n_taxa - 1, no HIP device.  No so_ctx: the call owns a stream of `device` and reads the
 * SOHIT_* switches itself (SOHIT_POISON, SOHIT_ORTH_TIER). */
typedef struct so_orth_cand {
    int64_t n_ot, n_ip, n_co, n_rows, n_runs, n_groups;
    int64_t *ot_a, *ot_b; double *ot_s;
    int64_t *ip_a, *ip_b; double *ip_s;
    int64_t *co_key;      double *co_best;
} so_orth_cand;
int so_orth_candidates_cols(int device, int64_t n, const int32_t *q, const int32_t *s, const double *idy, const double *aln,
                            const double *qst, const double *qed, const double *score, const double *qlen, int64_t n_names,
                            const int32_t *tax, int64_t n_taxa, double coverage, double identity, int norm, so_orth_cand *out);
int so_orth_candidates_records(int device, const so_hit *d_hits, int64_t n, const int32_t *qmap, int64_t n_q, const int32_t *smap,
                               int64_t n_s, int64_t n_names, const int32_t *tax, int64_t n_taxa, double coverage, double identity,
                               int norm, so_orth_cand *out);
void so_orth_free(so_orth_cand *result);
const char *so_orth_last_error(void);
/* The rest of find_orth but the text, on the candidate tables above while they are still on the device (csrc/orth.hip).  Replaces: the
 * in-paralog normalisers of bin/find_orth.py (507-543), the co-ortholog cross products (547-617) and the normalisation of the ortholog
 * and co-ortholog lines inside runs of one query taxon with its "repeats inside a run are dropped, one repeat of the run's first pair
 * survives" rule (681-762) -- as swiftortho_amd/find_orth.py `relation_tables()` restates them, bit for bit: every float64 sum is one
 * chain over its group's rows in table order, as numpy's bincount adds them.
 * Input, ordering, stream ownership and refusals: those of so_orth_candidates_cols / so_orth_candidates_records, argument for argument.
 * Output (allocated by the library, released with so_orth_rel_free()), in output order: ip_*: the forward in-paralog pairs (a < b) whose
 * taxon normaliser is not zero, with score / normaliser; ot_* / co_*: the ortholog / co-ortholog rows that survive the repeat rule, with
 * score / (mean score of their (run of one taxon of a, taxon of b) group); n_rows, n_runs, n_groups as above.  Only these tables come to
 * the host.  n = 0 and inputs whose every row is filtered are served and launch nothing for this stage.
 * Refused with a message (so_orth_last_error), never truncated: what the candidates calls refuse, and an input whose ortholog pairs expand
 * to 2^31 co-ortholog products ((in-paralogs of a + 1) * (in-paralogs of b + 1), summed in 64 bits) or more.  Scores are expected to be
 * numbers: a NaN score (-n bsr with a zero reference score) is outside what the call defines. */
typedef struct so_orth_rel {
    int64_t n_ip, n_ot, n_co, n_rows, n_runs, n_groups;
    int64_t *ip_a, *ip_b; double *ip_v;
    int64_t *ot_a, *ot_b; double *ot_v;
    int64_t *co_a, *co_b; double *co_v;
} so_orth_rel;
int so_orth_relations_cols(int device, int64_t n, const int32_t *q, const int32_t *s, const double *idy, const double *aln,
                           const double *qst, const double *qed, const double *score, const double *qlen, int64_t n_names,
                           const int32_t *tax, int64_t n_taxa, double coverage, double identity, int norm, so_orth_rel *out);
int so_orth_relations_records(int device, const so_hit *d_hits, int64_t n, const int32_t *qmap, int64_t n_q, const int32_t *smap,
                              int64_t n_s, int64_t n_names, const int32_t *tax, int64_t n_taxa, double coverage, double identity,
                              int norm, so_orth_rel *out);
void so_orth_rel_free(so_orth_rel *result);

/* Reciprocal best hits and the core-gene table on the device (csrc/rbh.hip).  Replaces: scripts/get_rbh.py -- per run of one query id the
 * best hit per subject taxon (get_rbh, 33-48) and "a pair is printed at every second proposal of its key" (51-65) -- and the two passes
 * of scripts/rbh2phy.py over the hit file (78-161): the forward best hits of the reference taxon's genes and the flags of those a best
 * hit back confirms -- as swiftortho_amd/rbh.py `reciprocal_best_hits()` and `core_table()` restate them, id for id and in their order.
 * Input: n hit rows in file order -- name codes q / s in 0 .. n_names - 1 and the float64 score column (host arrays, borrowed), or
 * so_hit records in DEVICE memory with the host maps query ordinal -> code (qmap, n_q) and subject ordinal -> code (smap, n_s), whose
 * score is `bit`.  Name codes ascend in the ids' string order.  tax[n_names]: taxon code of every name, in 0 .. n_taxa - 1.
 * ref_taxon: the reference taxon of the core table, or -1: the pairs only.  flags: reserved, 0.
 * A run = consecutive rows of one query code.  Per run and subject taxon other than the query's, the winner is the FIRST row holding the
 * largest score (+0 and -0 are equal); winners are listed by the first row of their (run, taxon) group.
 * Output (allocated by the library, released with so_rbh_free()): rbh_a / rbh_b: every winner proposes (smaller code, larger code); the
 * pair is listed at each even-numbered proposal of its key, in stream order.  core_gene[n_core]: the genes of ref_taxon that have a
 * winner, by their first one; core_fwd[n_core * n_taxa]: per gene and taxon the subject of the gene's LAST winner in that taxon, or -1;
 * core_rec[n_core * n_taxa]: 1 where a run of core_fwd's gene has its winner in ref_taxon at this gene.  n_runs runs, n_winners
 * winners; n_runs_long / n_rows_long: what the sorted tier took (the rest: one wave per run); waits: host waits of the call.
 * n = 0 is served and launches nothing.
 * Ordering of the records call: that of so_orth_*_records -- it first waits for ALL work queued on the device, works on a stream of its
 * own and has synchronised it when it returns.  The records are only read.
 * Refused with a message (so_rbh_last_error) and nothing left allocated: n >= 2^31, n_core * n_taxa >= 2^31, a name code, map index,
 * taxon or ref_taxon out of range, flags != 0, a NaN score (Python's `<` and sort disagree on it: the caller decides), no HIP device.
 * No so_ctx: the call reads the SOHIT_* switches itself (SOHIT_POISON, SOHIT_RBH_TIER). */
typedef struct so_rbh_result {
    int64_t n_rbh, n_core, n_taxa, n_runs, n_winners, n_runs_long, n_rows_long;
    int32_t waits;
    int32_t reserved;
    int32_t *rbh_a, *rbh_b;   /* n_rbh */
    int32_t *core_gene;       /* n_core */
    int32_t *core_fwd;        /* n_core * n_taxa */
    uint8_t *core_rec;        /* n_core * n_taxa */
} so_rbh_result;
int so_rbh_cols(int device, int64_t n, const int32_t *q, const int32_t *s, const double *score, int64_t n_names, const int32_t *tax,
                int64_t n_taxa, int32_t ref_taxon, int32_t flags, so_rbh_result *out);
int so_rbh_records(int device, const so_hit *d_hits, int64_t n, const int32_t *qmap, int64_t n_q, const int32_t *smap, int64_t n_s,
                   int64_t n_names, const int32_t *tax, int64_t n_taxa, int32_t ref_taxon, int32_t flags, so_rbh_result *out);
void so_rbh_free(so_rbh_result *result);
const char *so_rbh_last_error(void);

/* The pan-genome statistics of ortholog groups on the device (csrc/pan.hip).  Replaces: scripts/pan_genome.py -- the family-by-taxon count
 * table and the type of every family (108-157, the singleton rows 161-188) and the rarefaction pan_feature() over 20 seeded genome orders
 * (274-375, the branch taken without numexpr: 327-335) -- as swiftortho_amd/pan.py `count_matrix()`, `row_types()` and `rarefaction()`
 * restate them, count for count.  All of it is integer work; the host rounds the reference's float thresholds once.
 * Input (host arrays, borrowed): m kept members as pairs (row[k], taxon[k]), a pair listed twice counting twice; n_rows rows, of which the
 * first n_file_rows are lines of the groups file (the rest: one row per ungrouped gene); n_taxa taxa.  spec_max / core_min: with thr =
 * the taxa present in a row, a file row is Specific (type 0) when thr <= spec_max, Share (1) when thr < core_min, else Core (2); the
 * rows behind the file rows are Specific.  size genome orders perm[size * n_taxa], each a permutation of 0 .. n_taxa - 1; S[n_taxa] and
 * C[n_taxa]: the thresholds of step i = 1 .. n_taxa - 1 (entry 0 is not read).  want_counts: 0 = no count matrix.  flags: reserved, 0.
 * Curves: per order p, ys = presence (count > 0) of genome perm[p][0] per row; at step i, with yn the presence of genome perm[p][i]:
 * spec = rows with ys <= S[i] and yn, then ys += yn, core = rows with ys >= C[i], panz = rows with ys > 0.
 * Output (allocated by the library, released with so_pan_free()): counts[n_rows * n_taxa] (want_counts), type[n_rows], n_core / n_share /
 * n_spec: the types of the FILE rows counted; core / spec / panz [p * (n_taxa - 1) + i - 1]; tier: 1 = counters in the LDS, 2 = in global
 * memory, 0 = no curve launched; waits: host waits of the call.  n_rows = 0 is served and launches nothing (the curves are zeros).
 * Refused with a message (so_pan_last_error) and nothing left allocated: a row or taxon out of range, a perm row that is not a permutation,
 * n_rows, m or n_taxa >= 2^31, n_rows * n_taxa >= 2^31 when the matrix is wanted, size * n_taxa >= 2^31, flags != 0, no HIP device.
 * No so_ctx: the call reads the SOHIT_* switches itself (SOHIT_POISON, SOHIT_PAN_TIER). */
typedef struct so_pan_result {
    int64_t n_rows, n_taxa, size, n_core, n_share, n_spec;
    int32_t waits;
    int32_t tier;
    int32_t *counts;              /* n_rows * n_taxa, or empty */
    uint8_t *type;                /* n_rows */
    int64_t *core, *spec, *panz;  /* size * (n_taxa - 1) */
} so_pan_result;
int so_pan_genome(int device, int64_t m, const int32_t *row, const int32_t *taxon, int64_t n_rows, int64_t n_file_rows, int64_t n_taxa,
                  int32_t spec_max, int32_t core_min, int64_t size, const int32_t *perm, const int32_t *S, const int32_t *C,
                  int32_t want_counts, int32_t flags, so_pan_result *out);
void so_pan_free(so_pan_result *result);
const char *so_pan_last_error(void);

/* The families every pair of genomes shares, on the device (csrc/pan.hip): what swiftortho_amd/pan.py `shared_counts()` and `boot_shared()`
 * define, integer for integer -- the numbers the gene-content distances (Jaccard; overlap, Snel et al. 1999) and the gene-content tree with
 * its bootstrap support are made from.  The reference has no such product; the numpy functions are the definition.
 * Input as for so_pan_genome: m members as pairs (row[k], taxon[k]) (a pair listed twice counts once here), n_rows rows, n_taxa taxa.
 * n_reps == 0: shared[a * n_taxa + b] = the rows present in both a and b over all rows (seed and b0 are not read); n_reps >= 1: the matrices
 * of the bootstrap replicates b0 .. b0 + n_reps - 1, replicate b over the n_rows rows drawn with replacement as so_phy_boot_counts draws
 * columns: draw k = ((z >> 32) * n_rows) >> 32 with z = splitmix64's output for the counter (b << 32) + k + 1 added to `seed`; a row drawn
 * twice counts twice.  The full symmetric matrix with its diagonal (the families of a genome); every entry lies below 2^31.
 * flags bit 0: no matrix in the result (measurements); bit 1: events around the passes -- draw_ms, product_ms, summed over the batches.
 * Output (allocated by the library, released with so_pan_shared_free()): shared[max(n_reps, 1) * n_taxa * n_taxa]; n_reps: the matrices
 * in it; bytes: their size; batches: the groups of replicates whose presence words lay in device memory together (sized from the free
 * device memory, SOHIT_PAN_BOOT_BATCH forces the size); ranges: the ranges the row words of the last launch were cut into
 * (SOHIT_PAN_SHARED_RANGES forces the number); waits: host waits of the call -- one, whatever the batches.  n_rows = 0 with n_reps = 0 is
 * served and launches nothing.  Integers only: nothing depends on scheduling.
 * Refused with a message (so_pan_last_error) and nothing left allocated: a row or taxon out of range, n_taxa below 1 or above 4096, n_rows
 * or m >= 2^31, n_reps below 0 or above 32768, b0 + n_reps above 2^31, n_reps >= 1 with n_rows == 0, a result that does not fit half of
 * the free device memory (the message says how many bytes it would take), unknown flag bits, no HIP device.
 * No so_ctx: the call reads the SOHIT_* switches itself (SOHIT_POISON, SOHIT_PAN_BOOT_BATCH, SOHIT_PAN_SHARED_RANGES). */
typedef struct so_pan_shared_result {
    int64_t n_taxa, n_reps, bytes;
    int32_t waits, batches;
    int32_t ranges;
    int32_t reserved;
    double draw_ms, product_ms;   /* flags bit 1: device time of the draws and of the products */
    int32_t *shared;              /* n_reps * n_taxa * n_taxa, or empty (flags bit 0) */
} so_pan_shared_result;
int so_pan_shared(int device, int64_t m, const int32_t *row, const int32_t *taxon, int64_t n_rows, int64_t n_taxa, uint64_t seed, int64_t b0,
                  int64_t n_reps, int32_t flags, so_pan_shared_result *out);
void so_pan_shared_free(so_pan_shared_result *result);

/* Phyletic profiles on the device (csrc/phyletic.hip): the pairs of gene FAMILIES that co-occur across the genomes -- the product the other
 * way round, P P^T over the rows of the presence matrix (phylogenetic profiling, Pellegrini et al. 1999) -- as swiftortho_amd/phyletic.py
 * `linked_pairs()` defines them, integer for integer.  The reference has no such product; the numpy function is the definition.
 * Input as for so_pan_genome: m members as pairs (row[k], taxon[k]) (a pair listed twice counts once), n_rows rows of which the first
 * n_file_rows are lines of the groups file, n_taxa taxa.  present[r] = the distinct taxa of row r.  A row is ELIGIBLE iff r < n_file_rows and
 * n_min <= present[r] <= n_max.  Two eligible rows a < b that share k taxa, u = present[a] + present[b] - k, are LINKED iff k >= k_min and
 * k * den >= num * u: num / den is the Jaccard threshold, equality passes, no float takes part.
 * flags bit 0: no pair arrays in the result (measurements); bit 1: events around the passes -- count_ms, emit_ms, sort_ms.
 * Output (allocated by the library, released with so_phyletic_free()): present[n_rows]; the n_pairs linked pairs as a[], b[] (the rows' own
 * numbers) and shared[] (k), ordered by (a, b), the same arrays from call to call; n_eligible; tiles: the pairs I <= J of tiles of 64
 * eligible rows that were multiplied; waits: host waits of the call -- two, the count that sizes the output and the result (one when no
 * pair is linked, none for n_rows = 0).  The product is never stored: every tile is thresholded where it is computed, once to count and
 * once to emit.  n_rows = 0, fewer than two eligible rows (n_max < n_min included) and no linked pair are served.
 * Refused with a message (so_phyletic_last_error) and nothing left allocated: a row or taxon out of range, n_taxa below 1 or above 4096,
 * n_rows or m >= 2^31, n_file_rows outside 0 .. n_rows, n_min < 1, k_min < 1, num < 1, num > den, den >= 2^20, more than 64 * 65535 eligible
 * rows, 2^31 linked pairs and more, pairs that with their sort scratch do not fit half of the free device memory (the message says how
 * many bytes they would take), unknown flag bits, no HIP device.
 * No so_ctx: the call reads the SOHIT_* switches itself (SOHIT_POISON). */
typedef struct so_phyletic_result {
    int64_t n_rows, n_eligible, n_pairs, tiles;
    int32_t waits;
    int32_t reserved;
    double count_ms, emit_ms, sort_ms;   /* flags bit 1: device time of the count pass, the emit pass and the sort */
    int32_t *present;                    /* n_rows */
    int32_t *a, *b, *shared;             /* n_pairs, or empty (flags bit 0) */
} so_phyletic_result;
int so_phyletic_pairs(int device, int64_t m, const int32_t *row, const int32_t *taxon, int64_t n_rows, int64_t n_file_rows, int64_t n_taxa,
                      int32_t n_min, int32_t n_max, int32_t k_min, int32_t num, int32_t den, int32_t flags, so_phyletic_result *out);
void so_phyletic_free(so_phyletic_result *result);
const char *so_phyletic_last_error(void);

/* Gene-fusion links on the device (csrc/fusion.hip): the pairs of proteins that align side by side on one composite protein and are not
 * homologous to each other (the "Rosetta stone" method, Marcotte et al. 1999, Enright et al. 1999) -- as swiftortho_amd/fusion.py
 * `fusion_links()` defines them, integer for integer.  The reference has no such script; the numpy function is the definition.
 * Input: n hit rows in file order -- name codes q / s in 0 .. n_names - 1 and the int32 columns qst, qed, sst, sed (1-based, inclusive, as
 * printed), slen and qlen (host arrays, borrowed; qlen is only copied into `link`), or so_hit records in DEVICE memory with the host maps
 * query ordinal -> code (qmap, n_q) and subject ordinal -> code (smap, n_s).  tax[n_names]: taxon code of every name, in 0 .. n_taxa - 1.
 * max_overlap >= 0; num / den: the subject coverage, 0 <= num <= den < 2^20, den >= 1.  flags bit 0: same_taxon; bit 1: events around the
 * stages -- prep_ms (runs, eligibility, representatives, scan), keys_ms (the sort of all rows' keys), count_ms, count_again_ms (such a call runs
 * the count pass a second time, for its time alone), emit_ms, sort_ms.
 * A run = consecutive rows of one query code.  A row is ELIGIBLE iff s != q, (sed - sst + 1) * den >= num * slen (64-bit products, equality
 * passes) and, with same_taxon, tax[s] != tax[q].  The REPRESENTATIVE of a run and a subject is the first eligible row of that subject in
 * the run.  Two names are HOMOLOGOUS iff any of the n rows holds them as (q, s) or (s, q).  A LINK is a pair of representatives ra < rb of
 * one run with min(qed) - max(qst) + 1 <= max_overlap, with same_taxon tax[s[ra]] == tax[s[rb]], and s[ra], s[rb] not homologous.
 * Output (allocated by the library, released with so_fusion_free()): the n_links links as row_a[], row_b[], ascending by (row_a, row_b),
 * the same arrays from call to call; link[8 * n_links]: per link q, s[ra], s[rb], qst[ra], qed[ra], qst[rb], qed[rb], qlen[ra] -- what a
 * line of the text needs, so the records call downloads no record.  n_runs; n_eligible rows; n_reps representatives; n_pairs = the sum over
 * the runs of m (m - 1) / 2 for m representatives; n_disjoint = the pairs that passed the interval and the taxon test, before the homology
 * look-up; waits: host waits of the call -- two, the counters that size the output and the result (one without a link, none for n = 0).
 * The pairs are never stored: a fixed grid walks them twice, once to count and once to emit.  n = 0 is served and launches nothing.
 * Ordering of the records call: that of so_rbh_records -- it first waits for ALL work queued on the device, works on a stream of its own
 * and has synchronised it when it returns.  The records are only read.
 * Refused with a message (so_fusion_last_error) and nothing left allocated: a row with qst < 1, qed < qst, sst < 1, sed < sst or slen < 0,
 * max_overlap, num or den outside their ranges, unknown flag bits, n >= 2^31, a name code, map index or taxon out of range, 2^31 links and
 * more, links that with their sort scratch do not fit half of the free device memory (the message says how many bytes they would take),
 * no HIP device.
 * No so_ctx: the call reads the SOHIT_* switches itself (SOHIT_POISON). */
typedef struct so_fusion_result {
    int64_t n_runs, n_eligible, n_reps, n_pairs, n_disjoint, n_links;
    int32_t waits;
    int32_t reserved;
    double prep_ms, keys_ms, count_ms, count_again_ms, emit_ms, sort_ms;   /* flags bit 1: device time of the stages */
    int32_t *row_a, *row_b;                                /* n_links */
    int32_t *link;                                         /* 8 * n_links */
} so_fusion_result;
int so_fusion_cols(int device, int64_t n, const int32_t *q, const int32_t *s, const int32_t *qst, const int32_t *qed, const int32_t *sst,
                   const int32_t *sed, const int32_t *slen, const int32_t *qlen, int64_t n_names, const int32_t *tax, int64_t n_taxa,
                   int64_t max_overlap, int32_t num, int32_t den, int32_t flags, so_fusion_result *out);
int so_fusion_records(int device, const so_hit *d_hits, int64_t n, const int32_t *qmap, int64_t n_q, const int32_t *smap, int64_t n_s,
                      int64_t n_names, const int32_t *tax, int64_t n_taxa, int64_t max_overlap, int32_t num, int32_t den, int32_t flags,
                      so_fusion_result *out);
void so_fusion_free(so_fusion_result *result);
const char *so_fusion_last_error(void);

/* The operon pairs of the operon-clustering step on the device (csrc/operon.hip).  Replaces: the pair loop of scripts/operon_cluster.py
 * `operon_clust()` (136-168) -- for every operon the operons listed under the families of its genes, and per such pair the size of the
 * intersection of the two family sets -- as swiftortho_amd/operon.py `candidate_pairs()` restates it, count for count.  All of it is
 * integer work: the score and the text stay on the host.
 * Input (host arrays, borrowed): n_ops operons; fam[start[i] .. start[i + 1]) = the distinct indexed families (1 .. n_fam - 1; family 0 is
 * never indexed) of operon i in order of first token; length[i] = tokens of operon i (>= 1); has0[i] != 0: operon i holds a gene of
 * family 0; n_fam: families of the groups file.  flags bit 0: all candidates (below); every other bit must be 0.
 * A pair (i, j), i == j included, is a CANDIDATE when the two slices share a family; nshr = the families they share, + 1 when both have
 * has0; rank = the position in i's slice of the first family that j holds too.  A candidate PASSES when nshr > 2 and
 * 2 * nshr > min(length[i], length[j]).
 * Output (allocated by the library, released with so_operon_free()):
 *   flags = 0: the n_pairs passing pairs as i[], j[], nshr[], ordered by (i, j); cand_start is empty;
 *   flags = 1: all n_candidates candidates as i[], j[], nshr[], ordered by (i, rank, j) -- per operon the order in which j first occurs in
 *     the concatenation of the (ascending) operon lists of i's families -- and cand_start[n_ops + 1], the bounds of every operon's rows.
 *   n_pairs (passing) and n_candidates are filled in both modes; n_expansions = the sum over the entries of the size of their family's
 *   operon list (64-bit); batches: the consecutive ranges of operons the expansion was cut into (SOHIT_OPERON_EXPAND expansions each;
 *   an operon above that is a batch of its own); waits: host waits of the call (a constant per batch, whatever n_ops).  n_ops = 0, and
 *   operons without any indexed family, are served and launch nothing.
 * Refused with a message (so_operon_last_error) before any device work and with nothing left allocated: a null array or negative counts,
 * a start that does not rise from 0, a family outside 1 .. n_fam - 1, a family repeated inside one operon's slice, length[i] < 1, n_ops,
 * n_fam or the number of entries >= 2^31, an operon that alone expands to 2^32 - 16 pairs or more, unknown flag bits, no HIP device.
 * No so_ctx: the call reads the SOHIT_* switches itself (SOHIT_POISON, SOHIT_OPERON_EXPAND). */
typedef struct so_operon_result {
    int64_t n_ops, n_pairs, n_candidates, n_expansions;
    int32_t batches;
    int32_t waits;
    int32_t *i, *j, *nshr;        /* n_pairs (flags = 0) or n_candidates (flags = 1) */
    int64_t *cand_start;          /* n_ops + 1 (flags = 1), or empty */
} so_operon_result;
int so_operon_pairs(int device, int64_t n_ops, const int64_t *start, const int32_t *fam, const int32_t *length, const uint8_t *has0,
                    int64_t n_fam, int32_t flags, so_operon_result *out);
void so_operon_free(so_operon_result *result);
const char *so_operon_last_error(void);

/* The core-gene supermatrix from the hits' own alignments, and the counts its distances are made from, on the device (csrc/phy.hip).
 * Replaces: the second half of scripts/rbh2phy.py (the aligner it shells out to, and its join of the family alignments) by what
 * swiftortho_amd/phy.py `pick_rows()`, `project()`, `supermatrix()` and `pair_counts()` define, array for array.  Integer and byte work only.
 * so_phy_rows: n hit rows as host columns q, s (name codes) and score, in any order, and n_pairs wanted (pair_q, pair_s) pairs ->
 *   row[n_pairs]: the row with q == pair_q, s == pair_s and the highest score, the lowest such row among equal scores (0.0 == -0.0), -1
 *   when there is none.  A pair listed twice gets the same answer twice.  Refused: a NaN score, a negative code in a wanted pair, n or
 *   n_pairs >= 2^31, flags != 0.
 * so_phy_build: n_fam families, family f owning columns col_off[f] .. col_off[f + 1] (its anchor's length) of n_taxa rows; every task fills
 *   the block (fam, slot), at most one task per block, a block without a task stays '-':
 *     kind 1  the anchor itself: the block's row is residues[res_off .. res_off + res_len), res_len == the block's length;
 *     kind 0  a member: walk the runs runs[run_off[t] .. run_off[t + 1]) (length << 4 | op; 0 M, 1 I, 2 D) from anchor position qst - 1
 *             and member position sst - 1: M copies residues, I leaves the columns '-', D drops residues.
 *   Then gaps[c] = the '-' of column c, keep = the ascending columns with gaps[c] <= floor(gap_share * n_taxa), and over the kept columns
 *   cmp[a * n_taxa + b] = columns where neither row is '-', same[a * n_taxa + b] = those of them where the two bytes are equal.
 *   flags bit 0: no matrix in the result (the counts only).  n_keep entries of keep are valid.
 *   Refused with a message (so_phy_last_error) and nothing left allocated: n_taxa or n_fam of 0, more than 2^31 - 1 columns, 46341 taxa
 *   and more, offsets that do not rise from 0 or leave their arrays, a family or slot out of range, two tasks for one block, a gap share
 *   outside [0, 1], and -- found on the device, before the task stores anything -- qst or sst < 1, a run of length 0 or an unknown
 *   operation, runs that lead past the anchor or past the member, an anchor whose residues are not as many as its columns; the message names
 *   the lowest such task.
 * One result type for both calls (a call fills what it computes, the other arrays are empty); waits: host waits of the call.
 * No so_ctx: the calls read the SOHIT_* switches themselves (SOHIT_POISON). */
typedef struct so_phy_result {
    int64_t n_pairs, n_taxa, n_cols, n_keep;
    int32_t waits;
    int32_t reserved;
    int64_t *row;                 /* so_phy_rows: n_pairs */
    uint8_t *matrix;              /* n_taxa * n_cols, or empty (flags bit 0) */
    int32_t *gaps;                /* n_cols */
    int32_t *keep;                /* n_cols allocated, n_keep valid */
    int64_t *cmp, *same;          /* n_taxa * n_taxa */
} so_phy_result;
int so_phy_rows(int device, int64_t n, const int32_t *q, const int32_t *s, const double *score, int64_t n_pairs, const int32_t *pair_q,
                const int32_t *pair_s, int32_t flags, so_phy_result *out);
int so_phy_build(int device, int64_t n_taxa, int64_t n_fam, const int64_t *col_off, int64_t n_tasks, const int32_t *fam, const int32_t *slot,
                 const uint8_t *kind, const int64_t *res_off, const int32_t *res_len, const int32_t *qst, const int32_t *sst,
                 const int64_t *run_off, const uint32_t *runs, int64_t n_runs, const uint8_t *residues, int64_t n_res, double gap_share,
                 int32_t flags, so_phy_result *out);
void so_phy_free(so_phy_result *result);
const char *so_phy_last_error(void);

/* Bootstrap support for the neighbour-joining tree over the kept columns of a supermatrix, on the device (csrc/phy.hip): what
 * swiftortho_amd/phy.py `boot_columns()`, `boot_counts()`, `nj_splits()`, `split_support()` and `bootstrap()` define, array for array
 * (integers and bit sets; the float64 walk of nj_splits is the same sequence of IEEE operations).
 * matrix: n_taxa rows of n_cols bytes (host); keep: n_keep columns in 0 .. n_cols - 1; replicate b draws n_keep of them with replacement:
 *   draw k = ((z >> 32) * n_keep) >> 32 with z = splitmix64's output for the counter (b << 32) + k + 1 added to `seed`.
 * so_phy_boot_counts: cmp, same [n_reps][n_taxa][n_taxa] of the replicates b0 .. b0 + n_reps - 1 (the pair counts of so_phy_build over
 *   the drawn columns).  flags must be 0.
 * so_phy_nj_splits: D [n_reps][n_taxa][n_taxa] float64 (host), each finite and symmetric bit for bit -> splits [n_reps][n_taxa - 3][n_words],
 *   n_words = ceil(n_taxa / 64): the clade every join of the neighbour-joining walk makes (bit t = taxon t), complemented inside n_taxa
 *   bits where it holds taxon 0, in join order.  Row sums run left to right over the live nodes in ascending order; Q = ((n - 2) * D[i][j] -
 *   r[i]) - r[j], the minimum over i < j with ties to the lowest (i, j); the new row is ((D[i] + D[j]) - D[i][j]) / 2 at position i.
 *   A workgroup per matrix.  n_taxa < 4: no splits.  flags bit 0 (tests): the clade bit sets in global scratch whatever n_taxa.
 * so_phy_boot: the fused path of the p distance -- per replicate the counts, D = 1 - same / cmp, the walk and the comparison with the
 *   n_taxa - 3 splits of the printed tree (ref_splits, the same form) stay in device memory.  ok[b] = 0: a pair of replicate b shares no
 *   compared column, the replicate is dropped; valid = the others; count[s] = the valid replicates whose tree holds ref split s.
 *   flags bit 0: splits [n_reps][n_taxa - 3][n_words] of every replicate come back too (zeros for a dropped one); bit 1: events around the
 *   stages of every batch -- counts_ms (columns, pair counts, distances), trees_ms, support_ms.  Replicates run in
 *   batches sized from the free device memory (SOHIT_PHY_BOOT_BATCH forces the size), one host wait per batch: waits == batches.
 * nj_tier (both calls that walk): 1 while row sums, live lists and clade bit sets fit the walk's LDS budget (n_taxa <= 640), 2 beyond it or
 *   under so_phy_nj_splits' flags bit 0 (the bit sets in global scratch), 0 where n_taxa < 4 leaves nothing to walk.
 * Refused with a message (so_phy_last_error) and nothing left allocated: n_taxa below 2 or above 4096, n_keep of 0, n_reps below 1 or
 * b0 + n_reps above 2^31, a keep entry outside 0 .. n_cols - 1, a D that is not finite or not symmetric, unknown flag bits. */
typedef struct so_phy_boot_result {
    int64_t n_taxa, n_reps, n_splits, n_words, valid;
    int32_t waits, batches;
    double counts_ms, trees_ms, support_ms;   /* so_phy_boot with flags bit 1: device time of the three stages, summed over the batches */
    int64_t *cmp, *same;          /* so_phy_boot_counts: n_reps * n_taxa * n_taxa */
    uint64_t *splits;             /* so_phy_nj_splits, so_phy_boot with flags bit 0: n_reps * n_splits * n_words */
    int32_t *count;               /* so_phy_boot: n_splits */
    uint8_t *ok;                  /* so_phy_boot: n_reps */
    int32_t nj_tier;              /* so_phy_nj_splits, so_phy_boot: where the walk kept its clade bit sets -- 0: no walk (n_taxa < 4), 1: LDS, 2: global scratch */
    int32_t reserved;
} so_phy_boot_result;
int so_phy_boot_counts(int device, int64_t n_taxa, int64_t n_cols, const uint8_t *matrix, int64_t n_keep, const int64_t *keep, uint64_t seed,
                       int64_t b0, int64_t n_reps, int32_t flags, so_phy_boot_result *out);
int so_phy_nj_splits(int device, int64_t n_reps, int64_t n_taxa, const double *D, int32_t flags, so_phy_boot_result *out);
int so_phy_boot(int device, int64_t n_taxa, int64_t n_cols, const uint8_t *matrix, int64_t n_keep, const int64_t *keep, uint64_t seed,
                int64_t n_reps, const uint64_t *ref_splits, int32_t flags, so_phy_boot_result *out);
void so_phy_boot_free(so_phy_boot_result *result);

/* Gene concordance factors of the species tree on the device (csrc/phy.hip): what swiftortho_amd/phy.py `family_counts()`,
 * `family_present()`, `gene_distances()` (model p), `nj_splits_subset()` and `concordance()` define, array for array.  For every inner branch
 * of the printed tree: the families able to decide it, and those among them whose own neighbour-joining tree holds it.
 * matrix: n_taxa rows of n_cols bytes (host); keep: n_keep columns in 0 .. n_cols - 1; family f owns keep[fam_off[f] .. fam_off[f + 1]) (fam_off
 *   rises from 0 to n_keep; a family may own nothing).  Taxon t is PRESENT in family f iff one of the family's kept columns holds a byte other
 *   than '-' in row t (cmp[f][t][t] > 0); bit sets are n_words = ceil(n_taxa / 64) words, bit t & 63 of word t >> 6.
 * so_phy_gene_counts: cmp, same [n][n_taxa][n_taxa] of the families f0 .. f0 + n - 1 (the pair counts of so_phy_build over each family's kept
 *   columns): k_phy_fam_gather lays the families' columns side by side, each padded with '-' to a multiple of 16 bytes; k_phy_fam_pairs is
 *   k_phy_pairs' tile walk with a workgroup per (tile, family) and plain 32-bit stores.  flags must be 0.
 * so_phy_nj_subsets: D [n_reps][n_taxa][n_taxa] float64 and present [n_reps][n_words] (host) -> splits [n_reps][n_taxa - 3][n_words]: the walk
 *   of so_phy_nj_splits over the present taxa alone (the same body: the live list starts as the present taxa, ascending), each clade in the
 *   original bits, complemented inside the present set where it holds the LOWEST PRESENT taxon; with n present taxa the rows n - 3 .. are zeros,
 *   n < 4: all zeros.  Only present x present of D is read: there it is finite and symmetric bit for bit.  flags bit 0 (tests): the clade bit
 *   sets in global scratch whatever n_taxa.
 * so_phy_gene: the fused path of the p distance -- per family the counts, D = 1 - same / cmp, the present words, n_present, the walk and the
 *   comparison with the n_taxa - 3 splits of the printed tree (ref_splits, so_phy_nj_splits' form) stay in device memory.  ok[f] = 0: two
 *   present taxa of family f share no compared column, the family is dropped (its splits are zeros).  For split s with clade C and an ok
 *   family with present set P: A = C & P, B = P & ~C; decisive[s] counts the families where both hold two taxa, concordant[s] those among them
 *   whose tree holds the one of A and B without P's lowest taxon.  flags bit 0: present [n_fam][n_words] and splits [n_fam][n_taxa - 3][n_words]
 *   come back too; bit 1: events around the stages of every batch -- counts_ms (the gather, pair counts, distances and presence), trees_ms,
 *   concord_ms.  Families run in batches sized from the free device memory (SOHIT_PHY_GENE_BATCH forces the size), one host wait per batch:
 *   waits == batches.  nj_tier: as so_phy_boot's.
 * Refused with a message (so_phy_last_error) and nothing left allocated: n_taxa below 2 or above 4096, n_fam below 1, a fam_off that does not
 * rise from 0 to n_keep, a keep entry outside 0 .. n_cols - 1, families outside 0 .. n_fam - 1 or more than 32768 of them in so_phy_gene_counts,
 * padded rows beyond 2^31 - 16 bytes, a present bit at n_taxa or beyond, a D that is not finite or not symmetric between present taxa, unknown
 * flag bits, no device. */
typedef struct so_phy_gene_result {
    int64_t n_taxa, n_fam, n_splits, n_words;   /* n_fam: the families (so_phy_nj_subsets: the matrices) of the result */
    int32_t waits, batches;
    double counts_ms, trees_ms, concord_ms;   /* so_phy_gene with flags bit 1: device time of the three stages, summed over the batches */
    int64_t *cmp, *same;          /* so_phy_gene_counts: n_fam * n_taxa * n_taxa */
    uint64_t *splits;             /* so_phy_nj_subsets, so_phy_gene with flags bit 0: n_fam * n_splits * n_words */
    uint64_t *present;            /* so_phy_gene with flags bit 0: n_fam * n_words */
    int32_t *decisive, *concordant;   /* so_phy_gene: n_splits */
    int32_t *n_present;           /* so_phy_gene: n_fam */
    uint8_t *ok;                  /* so_phy_gene: n_fam */
    int32_t nj_tier;              /* so_phy_nj_subsets, so_phy_gene: 0: no walk (n_taxa < 4), 1: clade bit sets in the LDS, 2: in global scratch */
    int32_t reserved;
} so_phy_gene_result;
int so_phy_gene_counts(int device, int64_t n_taxa, int64_t n_cols, const uint8_t *matrix, int64_t n_keep, const int64_t *keep, int64_t n_fam,
                       const int64_t *fam_off, int64_t f0, int64_t n, int32_t flags, so_phy_gene_result *out);
int so_phy_nj_subsets(int device, int64_t n_reps, int64_t n_taxa, const double *D, const uint64_t *present, int32_t flags, so_phy_gene_result *out);
int so_phy_gene(int device, int64_t n_taxa, int64_t n_cols, const uint8_t *matrix, int64_t n_keep, const int64_t *keep, int64_t n_fam,
                const int64_t *fam_off, const uint64_t *ref_splits, int32_t flags, so_phy_gene_result *out);
void so_phy_gene_free(so_phy_gene_result *result);

/* The substitution-count tensor of a supermatrix on the matrix cores (csrc/phy.hip): what swiftortho_amd/phy.py `subst_counts()` and
 * `boot_subst()` define, integer for integer.  It is what the Kimura and LogDet distances of the species tree are made from.
 * Residue code a = the index of a byte in ARNDCQEGHILKMFPSTWYV; every other byte ('-', X, B, Z, U, '*', lower case, 0x00, 0xFF) is uncoded.
 * The pairs (i, j), i < j, of n_taxa taxa in row-major order: (0,1), (0,2), .., (n_taxa - 2, n_taxa - 1); n_pairs = n_taxa (n_taxa - 1) / 2.
 * so_phy_subst: subst[t][p][a][b] = the columns k of tensor t where taxon i of pair p holds residue a and taxon j residue b; a column where
 *   either byte is uncoded adds nothing to the pair.  n_reps == 0: one tensor over the kept columns (seed and b0 are not read); n_reps >= 1:
 *   the tensors of the bootstrap replicates b0 .. b0 + n_reps - 1, their columns drawn as so_phy_boot_counts draws them.
 *   k_phy_code writes the codes (0xFF: uncoded, and the padding of a row to the k-step of the product), k_phy_subst is the product
 *   N = E E^T of the one-hot matrix E (row 20 i + a over the columns is code[i][k] == a) by v_mfma_i32_32x32x32_i8 with 32-bit integer
 *   accumulators: E is never written -- a lane builds its operand bytes from 16 staged codes by a byte-wise compare --, only tiles that hold
 *   a pair i < j are walked, the columns are cut into ranges that flush with integer atomics.  No floating point: determinants and
 *   logarithms are the host's (numpy's), so the distances are the same bytes with and without the device.
 *   flags bit 0: no tensor in the result (measurements); bit 1: events around the two passes -- code_ms, product_ms.  One host wait.
 * Refused with a message (so_phy_last_error) and nothing left allocated: n_taxa below 2 or above 4096, n_keep of 0, a keep entry outside
 * 0 .. n_cols - 1, n_reps below 0 or above 32768, b0 + n_reps above 2^31, a tensor that does not fit half of the free device memory (the
 * message says how many bytes it would take), no device, unknown flag bits. */
typedef struct so_phy_subst_result {
    int64_t n_taxa, n_pairs, n_reps, bytes;   /* n_reps: the tensors in subst (1 for the kept columns); bytes: their size */
    int32_t waits;
    int32_t reserved;
    double code_ms, product_ms;   /* flags bit 1: device time of the coding pass and of the product */
    int32_t *subst;               /* n_reps * n_pairs * 400, or empty (flags bit 0) */
} so_phy_subst_result;
int so_phy_subst(int device, int64_t n_taxa, int64_t n_cols, const uint8_t *matrix, int64_t n_keep, const int64_t *keep, uint64_t seed,
                 int64_t b0, int64_t n_reps, int32_t flags, so_phy_subst_result *out);
void so_phy_subst_free(so_phy_subst_result *result);

/* The expansion of a collapsed search on the device (csrc/nr.hip).  Replaces: scripts/nr2full.py (14-44) -- every row of the search of
 * the collapsed proteome multiplied out to the cross product of the ';;;'-joined query ids and subject ids (23-33), inside a run of
 * rows of one collapsed query the expanded rows grouped by individual query in order of first appearance (35-44) -- as
 * swiftortho_amd/nr.py `expand_records()` restates it on records, byte for byte.
 * Input: n so_hit records in DEVICE memory (d_hits: the pointer so_search_device hands out, or any 16-byte aligned device buffer of
 * records), in the order the search returns them (ascending qidx; a run = consecutive records of one qidx), and two member tables (host
 * arrays, borrowed): qmem[qoff[c] .. qoff[c + 1]) = the ordinals, in the full file, of the members of collapsed query c, in file order
 * (qoff: n_q + 1 offsets); soff / smem the same for the subjects.
 * Output: n_out records in device memory the library owns until so_nr_expand_free(): for the run of collapsed query c with members m_0 ..
 * m_{k-1}, rows j = 0 .. t-1, n_j members of row j's subject, S = sum n_j, P_j = sum_{i<j} n_i, the record of (member a, row j, subject
 * member b) stands at base_c + a * S + P_j + b (base_c: the expanded records of all earlier runs) and equals row j with qidx = m_a and
 * sidx = subject member b; every other field is unchanged.  All totals are 64-bit.  n_runs: runs of the input; waits: host waits of
 * the call (the totals, the end).  flags & 1: count only -- n_out and n_runs are filled, d_out stays NULL.  n = 0 launches nothing.
 * Ordering: that of so_orth_*_records -- the call first waits for ALL work queued on the device, works on a stream of its own and has
 * synchronised it when it returns.  The records are only read.
 * Refused with a message (so_nr_last_error) and nothing left allocated: before a device is touched negative counts, n >= 2^31, a member
 * table that does not rise from 0, a table whose members are not each named exactly once, records that are not 16-byte aligned, no HIP
 * device; found on the device before d_out is allocated a qidx outside 0 .. n_q - 1 or a sidx outside 0 .. n_s - 1, and n_out >= 2^31
 * (what the orthology stage refuses too).  No so_ctx: the call reads the SOHIT_* switches itself (SOHIT_POISON). */
typedef struct so_nr_expand_result {
    int64_t n_in, n_out, n_runs;
    int32_t waits;
    int32_t reserved;
    so_hit *d_out;     /* n_out records, device memory */
} so_nr_expand_result;
int so_nr_expand(int device, const so_hit *d_hits, int64_t n, const int64_t *qoff, const int32_t *qmem, int64_t n_q, const int64_t *soff,
                 const int32_t *smem, int64_t n_s, int32_t flags, so_nr_expand_result *out);
void so_nr_expand_free(so_nr_expand_result *result);
const char *so_nr_last_error(void);

/* Host-side tokeniser of tab-separated text for the stages behind the search (csrc/tsv.hip; no device, no so_ctx).  Replaces: the
 * per-line `split('\t')` + `float()` loops of bin/find_orth.py (blastparse, 58-125) and bin/find_cluster.py (1425-1467) as the
 * numpy tokeniser of swiftortho_amd/find_orth.py restates them.
 *   so_tsv_lines  start offset of every line of buf[0..n) (a line ends at its '\n'); returns the number of lines.
 *   so_tsv_scan   for every line and each requested column cols[c]: [beg, beg + len) of the field (numeric columns: stripped of ASCII
 *                 white space), the number of tabs of the line, and for numeric columns the value with status 0 = plain decimal
 *                 number (strtod), 1 = empty or missing, 2 = anything else (the caller applies Python's float()).  Arrays are
 *                 [ncols][nline].  numeric[c]: 0 = text column (bounds), 1 = number (bounds, value, status), 2 = number, status only,
 *                 3 = number, value and status -- what is not asked for is not written.  Returns 0.
 *   so_tsv_codes  two columns of byte strings -> codes into their sorted distinct list (byte order, a proper prefix first: numpy's
 *                 order of fixed-width byte strings); returns the number of distinct strings, or minus it when cap is too small. */
int64_t so_tsv_lines(const char *buf, int64_t n, int64_t *line_start, int64_t cap);
int so_tsv_scan(const char *buf, int64_t n, const int64_t *line_start, int64_t nline, int32_t ncols, const int32_t *cols, const uint8_t *numeric,
                int32_t *ntab, int64_t *beg, int32_t *len, double *val, uint8_t *status);
int64_t so_tsv_codes(const char *buf, int64_t nrows, const int64_t *beg_a, const int32_t *len_a, const int64_t *beg_b, const int32_t *len_b,
                     int64_t *code_a, int64_t *code_b, int64_t *name_beg, int32_t *name_len, int64_t cap);
/* The output side of the same stages: n lines  kind \t name[x] \t name[y] \t repr(v) \n  (find_orth.py prints its relations with
 * Python's repr of the score, 1181-1226); names = concatenated ids, name_off[k] .. name_off[k + 1] the k-th.  Returns the bytes written,
 * or minus the bytes needed when cap is too small.  so_py_repr: repr() of n doubles, one per line (tests). */
int64_t so_format_pairs(const char *kind, int32_t kind_len, const char *names, const int64_t *name_off, const int64_t *x, const int64_t *y,
                        const double *v, int64_t n, char *out, int64_t cap);
int64_t so_py_repr(const double *v, int64_t n, char *out, int64_t cap);

/* The shared device primitives, one at a time (csrc/prim.hip) -- for the tests: every stage stands on the scans and run helpers of
 * csrc/k_util.hip and on the library sorts of csrc/k_sort.hip / k_sortseg.hip, and these calls run the wrappers the stages call
 * (csrc/kernels.h) on host arrays.  All arrays are the caller's (borrowed inputs, outputs of the stated length); 0 = done, 1 = refused with
 * a message (so_prim_last_error).  No so_ctx: each call reads the SOHIT_* switches itself (SOHIT_POISON).
 *   so_prim_scan_path  no device: the way scan_u32 takes n values (0 nothing launched, 1 one launch, 2 three kernels), *tiles its tiles.
 *   so_prim_sort_tier  no device: the library's algorithm for a device-wide sort (kind 0 .. 2 below) of n keys: 0 one block, 1 merge sort,
 *                      2 onesweep; *single_block / *merge_limit: the largest n of tiers 0 and 1, from the library's configuration types.
 *   so_prim_seg_variant  no device: the instance a segmented sort (kind 3 .. 6) runs for n keys in nseg segments of a field `width` bits
 *                      wide: kinds 3, 4: 0 library default, 2, 6 the tuned ones; kind 5: 0, 1, 2; kind 6: 0.
 *   so_prim_scan       out[n] = exclusive (inclusive != 0: inclusive) prefix sums mod 2^32 of in[n]; the device input / output start
 *                      in_skew / out_skew words (0 .. 3) behind a 16-byte boundary; in_place: one device range for both (the skews are
 *                      equal).  guards[8]: the four words in front of and the four behind the device output range, set to 0xA5C3F00D
 *                      before the scan.  *total: the sum; *path, *tiles: as so_prim_scan_path.
 *   so_prim_effscan    hoff[n], cidx[n] = exclusive prefixes of c(t) = mark[t] ? scnt[t] : 0 and of [c(t) != 0]; the device mark starts
 *                      mark_skew BYTES behind a 16-byte boundary, scnt, hoff and cidx scnt_skew words; guards[16]: hoff's eight, cidx's
 *                      eight; totals[2] = {sum of c mod 2^32, non-zero c}.
 *   so_prim_runs       n >= 1 keys of key_bytes 4 (int) or 8 (u64): head[n], rid[n] (key_runs), *n_runs, start[n + 2] (run_starts; set to
 *                      0xA5C3F00D before: start[r] for every run, start[*n_runs] = n, the sentinel behind).
 *   so_prim_number     number_by_first_appearance of nr >= 1 rows (cx, cy) of codes 0 .. n_codes - 1: X[nr], Y[nr],
 *                      gene_code[min(n_codes, 2 nr)] (-1 behind the *n_genes genes), first[n_codes], flag[2 nr].
 *   so_prim_sort       kind 0 sort_keys_u64, 1 sort_pairs_u64_u32, 2 sort_pairs_u64_u64 (begin_bit = 0), 3 sort_keys_u64_seg,
 *                      4 sort_keys_u64_seg2, 5 sort_cand_keys_seg, 6 sort_keys_u64_seg_desc on key bits [begin_bit, end_bit).  Segments:
 *                      kind 4 seg_begin[nseg] and seg_end[nseg], the others seg_begin[nseg + 1] (seg_end unused); they rise and end within
 *                      n.  kout[n] (every byte 0xD6 before the sort), vout[n] for the pairs.  The scratch is what the matching
 *                      *_temp_bytes asks for, asked before any array is read.  info[4] = {variant (so_prim_seg_variant; -1 for kinds
 *                      0 .. 2), tier (so_prim_sort_tier -- kind 0 with begin_bit > 0 and end_bit = 64 has no tier 1: 2; -1 for kinds 3 .. 6), scratch bytes, bytes changed among the 256 behind the scratch}.
 *                      kind | 0x100, n >= 2^31: the sort itself is asked, without scratch or arrays, and must refuse as its
 *                      *_temp_bytes does.
 * Refused: counts out of range (n >= 2^31 by the sorts themselves), null arrays, skews outside 0 .. 3, codes outside 0 .. n_codes - 1,
 * segments that fall, overlap or end behind n, end_bit = 64 for the segmented sorts (by the sorts themselves), no HIP device. */
int32_t so_prim_scan_path(int64_t n, int64_t *tiles);
int32_t so_prim_sort_tier(int32_t kind, int64_t n, int64_t *single_block, int64_t *merge_limit);
int32_t so_prim_seg_variant(int32_t kind, int64_t n, int64_t nseg, int32_t width);
int so_prim_scan(int device, int64_t n, const uint32_t *in, int32_t in_skew, int32_t out_skew, int32_t inclusive, int32_t in_place, uint32_t *out,
                 uint32_t *guards, uint32_t *total, int32_t *path, int64_t *tiles);
int so_prim_effscan(int device, int64_t n, const uint8_t *mark, int32_t mark_skew, const uint32_t *scnt, int32_t scnt_skew, uint32_t *hoff,
                    uint32_t *cidx, uint32_t *guards, uint32_t *totals, int64_t *tiles);
int so_prim_runs(int device, int64_t n, int32_t key_bytes, const void *key, uint32_t *head, uint32_t *rid, uint32_t *start, int64_t *n_runs);
int so_prim_number(int device, int64_t nr, int64_t n_codes, const int32_t *cx, const int32_t *cy, int32_t *X, int32_t *Y, int32_t *gene_code,
                   uint32_t *first, uint32_t *flag, int64_t *n_genes);
int so_prim_sort(int device, int32_t kind, int64_t n, const uint64_t *kin, const void *vin, int64_t nseg, const uint32_t *seg_begin,
                 const uint32_t *seg_end, int32_t begin_bit, int32_t end_bit, uint64_t *kout, void *vout, int64_t *info);
const char *so_prim_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SOHIT_H */
