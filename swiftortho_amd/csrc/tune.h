// tune.h -- every SOHIT_* switch of libsohit.so in ONE table.  The environment is read ONCE, by so_create (Tune::read), into the
// context's Tune; the launch helpers in the k_*.hip files read the current context's copy through tune() -- no getenv() anywhere else.
// (so_mcl, so_apc and so_cnc_groups run without a context: each call reads the table into a Tune of its own at entry.)
// None of the switches changes results, except the two ablation variants marked so.  tools/diag/README.md lists what they are for.
#pragma once
#include <cstdlib>

//   kind  field            environment variable      default   meaning
//   B = boolean (unset: default, else atoi != 0), I = integer (atoll), D = double (atof), P = presence (set to anything),
//   T = tier of k_orth_run (auto | wave | lds | scratch, or 0 .. 3)
#define SOHIT_TUNE_TABLE(X)                                                                                                                                     \
    /* ---- ungapped extension ---- */                                                                                                                          \
    X(B, ug1, "SOHIT_UG1", 1, "bucketed passes: singleton groups to k_ungap1 (0: everything to k_ungap)")                                                     \
    X(B, ug1_chain, "SOHIT_UG1_CHAIN", 1, "... and the groups of two and more hits to k_ungap2 (0: to k_ungap, which then skips the singletons)")              \
    X(B, count_steps, "SOHIT_UG_COUNT", 0, "counting instances of the extension kernels: so_counters.ungap_steps, groups_single, groups_chain")                \
    X(B, ungapq, "SOHIT_UNGAPQ", 1, "sparse passes of queries up to 512 residues: hits alone on their diagonal by k_ungapq, a wave per query (0: every hit through the sorted keys)")     \
    X(I, uq_cache, "SOHIT_UQ_CACHE", -1, "... its hit ordinals per query whose index entries stay in registers between the two walks, in steps of 64 (-1: the compiled 1024; 0: every entry read twice; tests move the boundary)") \
    X(I, uq_chains, "SOHIT_UQ_CHAINS", -1, "... what it leaves over sorted per query (k_uqsort_wave: a wave's registers, k_uqsort_wg: a workgroup's LDS) and chained by k_ungap2 from the list of group heads (0: library segmented sort + k_ungap + k_first_touch; N > 0: the largest tier holds N keys -- tests reach the in-place instance with small inputs)") \
    X(B, ug_w32, "SOHIT_UG_W32", 1, "bucketed passes hand k_ungap the buckets' 32-bit words (0: 64-bit keys; no k_ungap1 then)")                               \
    /* ---- seed stage: which path a pass takes ---- */                                                                                                         \
    X(B, bucket, "SOHIT_BUCKET", 1, "bucketed diagonal binning (0: every pass on the sorted path)")                                                            \
    X(I, bucket_min, "SOHIT_BUCKET_MIN", 192, "hits per bucket below which a pass takes the sorted path (0: bucketed whenever possible)")                      \
    X(I, bucket_avg, "SOHIT_BUCKET_AVG", 2560, "average bucket size the band-range width is chosen for")                                                       \
    X(I, count_tab, "SOHIT_COUNT_TAB", 1, "bucketed passes: hits per (tile, range) from the range boundaries of the ordered index buckets when a batch brings a chunk two passes and more (0: always the counting pass over the entries; 2: always both, compared -- tests; 3: always)") \
    X(B, bucket_best, "SOHIT_BUCKET_BEST", 1, "best diagonal per subject by the per-bucket reduction (0: sort of the pass records)")                           \
    X(B, bands, "SOHIT_BANDS", 1, "diagonal bands follow the subjects' lengths (0: one band per subject)")                                                     \
    X(B, lk_wide, "SOHIT_LK_WIDE", 0, "8-byte index addends whatever the field widths")                                                                        \
    X(B, qclass, "SOHIT_QCLASS", 1, "queries of a batch in length-class order (0: file order)")                                                                \
    X(B, pass_merge, "SOHIT_PASS_MERGE", 1, "neighbouring length classes that take the sorted path anyway share one pass")                                     \
    X(B, ksc_lazy, "SOHIT_KSC_LAZY", 1, "k-mer orders computed for the queries that reach their frequency cap, when they do (a query below it keeps every window whatever the order; 0: for every query, with the batch)") \
    X(B, bounds_ahead, "SOHIT_BOUNDS_AHEAD", 1, "the next chunk's bucket bounds (k_bounds) on the side stream beside this chunk's seed stage (0: in front of its own)")     \
    X(I, segsort, "SOHIT_SEGSORT", 1, "sorted path: segmented sort of the keys inside each query (0: device-wide sort)")                                        \
    X(I, write_threads, "SOHIT_WRITE_THREADS", 48, "so_write_sc: formatter threads (at most the host's cores)")                                                                          \
    /* ---- candidate order ---- */                                                                                                                             \
    X(I, cand_limit, "SOHIT_CAND_LIMIT", 0, "tests: candidate-store size at which a batch is split (0: 2^32 - 16)")                                            \
    /* ---- phase 2 ---- */                                                                                                                                     \
    X(B, align_pk, "SOHIT_ALIGN_PK", 1, "packed 16-bit score-only aligner where the scores fit")                                                               \
    X(B, align_lane, "SOHIT_ALIGN_LANE", 1, "score-only rounds: one lane per alignment pair (k_align_lane) when no sequence reaches 4096 residues (0: k_align_pk)")            \
    X(I, align_lane_min, "SOHIT_ALIGN_LANE_MIN", 1 << 18, "... for rounds of at least this many packed tasks (below: k_align_pk; tests: 0)")                 \
    X(B, align_sort, "SOHIT_ALIGN_SORT", 1, "launch lists ordered by band rows")                                                                               \
    X(I, trace_wave_rows, "SOHIT_TRACE_WAVE_ROWS", 1024, "traceback: bands of this many rows and more are walked by a wave of their own (0: never)")         \
    X(I, trace_wave_max, "SOHIT_TRACE_WAVE_MAX", 32768, "... among the first this many positions of a launch list")                                            \
    X(I, spec, "SOHIT_SPEC", -1, "speculative traces in the first round: 0 off, 1 on, -1 from 2^21 tasks on")                                                  \
    X(D, spec_slack, "SOHIT_SPEC_SLACK", 1e6, "... the guess tests the ungapped score against expect x this (tests: 1e30 = every first-round task traced, 1e-30 = none)")          \
    X(I, spec_cap, "SOHIT_SPEC_CAP", -1, "tests: most speculative traces kept (-1: all)")                                                                      \
    X(I, trace_var_max, "SOHIT_TRACE_VAR_MAX", -1, "tests: trace words a launch list's own-size traces may take, and the fixed-stride slabs' budget (-1: 2^31 / 2^30)") \
    X(I, emit_parts, "SOHIT_EMIT_PARTS", 4, "... and otherwise")                                                                                               \
    X(I, emit_min_rows, "SOHIT_EMIT_MIN_ROWS", 1 << 18, "rows below which the emission is one part")                                                           \
    X(P, test_oom_phase2, "SOHIT_TEST_OOM_PHASE2", 0, "tests: phase 2 of the first batch fails once with an out-of-memory error")                              \
    /* ---- batches, memory ---- */                                                                                                                             \
    X(I, batch, "SOHIT_BATCH", 0, "queries per device batch (0: 131072, lowered when the candidate estimate asks)")                                            \
    X(I, max_hits, "SOHIT_MAX_HITS", 0, "seed hits per pass (0: 2^30)")                                                                                        \
    X(I, poison, "SOHIT_POISON", -1, "tests: byte every fresh device allocation is filled with (-1: none)")                                                    \
    X(B, hit_cache, "SOHIT_HIT_CACHE", 1, "one released result array is kept for the next search")                                                             \
    X(P, keep_cands, "SOHIT_KEEP_CANDS", 0, "tests: keep every query's candidate list (so_query_candidates)")                                                  \
    X(P, keep_masked, "SOHIT_KEEP_MASKED", 0, "tests: keep the masked queries (so_masked_query)")                                                              \
    X(I, mcl_scratch, "SOHIT_MCL_SCRATCH", -1, "tests: u32 words of expansion / convergence scratch per range of rows (-1: 2^28)")                             \
    /* ---- find_orth candidates (so_orth_candidates_*: read per call) ---- */                                                                                  \
    X(T, orth_tier, "SOHIT_ORTH_TIER", 0, "tests: every run of query rows through one tier of k_orth_run wherever that tier can take it (0 = auto: by run length)") \
    /* ---- reciprocal best hits (so_rbh_*: read per call) ---- */                                                                                              \
    X(T, rbh_tier, "SOHIT_RBH_TIER", 0, "tests: wave = runs of up to 64 rows through k_rbh_run_wave (what auto does), long or sort = every run through the sorted tier (0 = auto: by run length)") \
    /* ---- pan-genome statistics (so_pan_genome: read per call) ---- */                                                                                        \
    X(T, pan_tier, "SOHIT_PAN_TIER", 0, "tests: lds = what auto does where the taxa fit the LDS of k_pan_curve, global = words, orders and counters in global memory (0 = auto: by the number of taxa)") \
    X(I, pan_boot_batch, "SOHIT_PAN_BOOT_BATCH", 0, "so_pan_shared: replicates whose presence words are in device memory at a time (0: what half of the free device memory holds; tests move the batch edges)") \
    X(I, pan_shared_ranges, "SOHIT_PAN_SHARED_RANGES", 0, "so_pan_shared: ranges the row words of k_pan_shared are cut into (0: whole chunks until about 1024 workgroups exist; tests make a small input walk several)") \
    /* ---- operon pairs (so_operon_pairs: read per call) ---- */                                                                                               \
    X(I, operon_expand, "SOHIT_OPERON_EXPAND", -1, "tests: expansions per batch (-1: 2^28)")                                                                   \
    /* ---- bootstrap of the species tree (so_phy_boot: read per call) ---- */                                                                                  \
    X(I, phy_boot_batch, "SOHIT_PHY_BOOT_BATCH", 0, "replicates per batch (0: what half of the free device memory holds; tests move the batch edges)")        \
    /* ---- gene concordance factors of the species tree (so_phy_gene: read per call) ---- */                                                                  \
    X(I, phy_gene_batch, "SOHIT_PHY_GENE_BATCH", 0, "families per batch (0: what half of the free device memory holds; tests move the batch edges)")          \
    /* ---- index ---- */                                                                                                                                       \
    X(P, exact_threshold, "SOHIT_EXACT_THRESHOLD", 0, "threshold always by the sequential fp64 replay")                                                        \
    X(I, dir_max, "SOHIT_DIR_MAX", -1, "largest -M served by the bitmap + rank directory (-1: 2^31)")                                                          \
    X(I, ixs_k, "SOHIT_IXS_K", -1, "pair grouping, second hop: slices per workgroup, a power of two up to 64 (-1: the compiled 16)")                            \
    X(I, ixs_cap, "SOHIT_IXS_CAP", -1, "pair grouping, bins: most pairs of a bin ordered in the LDS, up to 4096 (-1: 4096; 0: every bin by the counters per id; tests move the boundary)") \
    /* ---- traces ---- */                                                                                                                                      \
    X(P, debug, "SOHIT_DEBUG", 0, "per-pass lines on stderr")                                                                                                  \
    X(P, debug_index, "SOHIT_DEBUG_INDEX", 0, "wall laps of the index build on stderr")

// ---- find_orth candidates (orth.hip): which tier of k_orth_run takes a run of query rows ----
#define ORTH_WAVE_ROWS 64     // longest run one wave holds in registers, a row per lane
#define ORTH_LDS_ROWS 1024    // longest run whose subjects fit the LDS table (2 slots per row) ...
#define ORTH_LDS_TAXA 512     // ... when the taxa fit the per-taxon LDS table; beyond either: tables in global scratch
enum { ORTH_TIER_AUTO = 0, ORTH_TIER_WAVE = 1, ORTH_TIER_LDS = 2, ORTH_TIER_SCRATCH = 3 };
static inline int orth_tier_of(const char* v) {
    switch (v[0]) {
        case 'w': case '1': return ORTH_TIER_WAVE;
        case 'l': case '2': return ORTH_TIER_LDS;
        case 's': case '3': return ORTH_TIER_SCRATCH;
        case 'g': return ORTH_TIER_SCRATCH;   // g[lobal]: SOHIT_PAN_TIER's name for the tier without LDS tables
        default: return ORTH_TIER_AUTO;
    }
}

// ---- reciprocal best hits (rbh.hip): SOHIT_RBH_TIER is read with orth_tier_of -- w[ave] = 1; l[ong], s[ort] (2, 3) = the sorted tier ----
#define RBH_WAVE_ROWS 64      // longest run k_rbh_run_wave holds, a row per lane; longer runs go through the (run, taxon) sort

// ---- pan-genome statistics (pan.hip): SOHIT_PAN_TIER is read with orth_tier_of -- l[ds] = 2; g[lobal] (3) = the tier without LDS tables ----
#define PAN_LDS_BYTES 65536u  // most LDS k_pan_curve asks for: 80 bytes per taxon (a tile's words, four orders, thresholds, 12 counters per step)
#define PAN_TILE_RANGES 256u  // ranges the row tiles are cut into: a workgroup walks one range for four orders and flushes its counters once
// ... and the shared-family counts (k_pan_shared): 64 x 64 taxon pairs per workgroup, a 4 x 4 block per lane; a chunk of 32 row words (2048
// rows) of both sides is 32 KiB of LDS; the row words are cut into ranges of whole chunks until about PAN_SH_TARGET_WGS workgroups exist.
// k_pan_draw walks PAN_DRAW_BLOCKS blocks of 64 taxa per wave: the 64 bytes of a drawn row's words that share a cache line
#define PAN_SH_TILE 64u
#define PAN_SH_CHUNK 32u
// ... and the family pairs the other way round (phyletic.hip, k_pp_tile): the same tile over 64 x 64 eligible families, whose K dimension is
// the taxon words (at most 64): a chunk of 16 words of both sides is 16 KiB of LDS, so it is the registers, not the LDS, that say how many workgroups a CU holds
#define PP_CHUNK 16u
#define PAN_SH_TARGET_WGS 1024u
#define PAN_DRAW_BLOCKS 8u
#define PAN_MAX_TAXA 4096
#define PAN_BOOT_MAX_REPS 32768

// ---- operon pairs (operon.hip): expansions of one batch.  A memory bound, not a tuned value: the sort helpers take 12 bytes per element
// (u64 key, u32 payload) for input and output each, so 2^28 expansions are about 6 GB of keys, payloads and sort scratch ----
#define OPERON_EXPAND_DEFAULT (1ull << 28)

// ---- supermatrix and pair counts (phy.hip): the tile of k_phy_pairs.  64 x 64 taxon pairs per workgroup, a 4 x 4 block per lane; a chunk
// of 32 words (128 kept columns) of both row sets and their non-gap masks is 32 KiB of LDS, five workgroups to a CU.  The LDS image is
// [word][row]: a lane's four rows are one 16-byte read, the 16 lanes of a row group read 256 consecutive bytes (no bank is asked twice)
// and the four row groups of the other side read one address each (a broadcast) ----
#define PHY_TILE 64u
#define PHY_CHUNK_WORDS 32u
#define PHY_TARGET_WGS 1024u   // the kept columns are cut into ranges until about this many workgroups exist (each flushes its counts once)
// ... and the bootstrap on top of them: k_phy_boot_gather walks the taxa in groups of PHY_BOOT_TAXA per workgroup (a draw is computed once per
// group); k_phy_nj keeps the clade bit sets of a replicate in the LDS while row sums, live lists and bit sets fit PHY_NJ_LDS_BYTES (T <= 640),
// beyond that in global scratch; a batch holds at most PHY_BOOT_MAX_BATCH replicates (a grid dimension)
#define PHY_BOOT_TAXA 32u
#define PHY_NJ_THREADS 256u
#define PHY_NJ_LDS_BYTES 61440u
#define PHY_BOOT_MAX_BATCH 32768
#define PHY_MAX_TAXA 4096
// ... and the substitution counts (k_phy_subst): the one-hot matrix E has 20 rows per taxon; a workgroup owns PHS_TILE x PHS_TILE of
// N = E E^T, its four waves 64 x 64 each as 2 x 2 tiles of v_mfma_i32_32x32x32_i8.  PHS_TILE rows of E touch at most PHS_TAXA taxa
// ((PHS_TILE + 18) / 20 + 1), whose codes are staged in the LDS PHS_CHUNK_COLS columns at a time (a multiple of the k-step 32; 2 x 4 KiB);
// the kept columns are cut into ranges of whole chunks until about PHS_TARGET_WGS workgroups exist
#define PHS_TILE 128u
#define PHS_TAXA 8u
#define PHS_CHUNK_COLS 512u
#define PHS_TARGET_WGS 1024u

struct Tune {
#define X_B(f, d) bool f = (d) != 0;
#define X_I(f, d) long long f = (d);
#define X_D(f, d) double f = (d);
#define X_P(f, d) bool f = false;
#define X_T(f, d) int f = (d);
#define X(kind, field, env, dflt, text) X_##kind(field, dflt)
    SOHIT_TUNE_TABLE(X)
#undef X
#undef X_B
#undef X_I
#undef X_D
#undef X_P
#undef X_T
    void read() {
#define X_B(f, e) if (const char* v = getenv(e)) f = atoi(v) != 0;
#define X_I(f, e) if (const char* v = getenv(e)) f = strtoll(v, nullptr, 0);
#define X_D(f, e) if (const char* v = getenv(e)) f = atof(v);
#define X_P(f, e) f = getenv(e) != nullptr;
#define X_T(f, e) if (const char* v = getenv(e)) f = orth_tier_of(v);
#define X(kind, field, env, dflt, text) X_##kind(field, env)
        SOHIT_TUNE_TABLE(X)
#undef X
#undef X_B
#undef X_I
#undef X_D
#undef X_P
#undef X_T
    }
};

// the switches of the context whose API call runs on this thread (set by so_create and by every guarded entry point)
const Tune& tune();
void set_tune(const Tune* t);
