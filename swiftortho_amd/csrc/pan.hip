// pan.hip -- the pan-genome statistics of ortholog groups on the device: from the (family row, taxon) pairs of the kept members to what
// swiftortho_amd/pan.py `count_matrix()`, `row_types()` and `rarefaction()` define -- the family-by-taxon count table scripts/pan_genome.py
// prints, the type of every row with the three totals, and the rarefaction curves of its pan_feature() (core, new and present families
// after every genome added, for every one of the seeded genome orders).
//
// The numpy functions are the definition; all of it is integer work:
//   * counts[row][taxon] = how often the pair occurs; presence = counts > 0;
//   * thr = taxa present in the row; a file row is Specific when thr <= spec_max, Share when thr < core_min, else Core; the rows behind
//     the file rows (one per ungrouped gene) are Specific; the totals count the file rows;
//   * curves: per order p, ys = presence of genome perm[p][0]; at step i = 1 .. T - 1 with yn = presence of genome perm[p][i]:
//     spec = #(ys <= S[i] and yn), then ys += yn, core = #(ys >= C[i]), panz = #(ys > 0).  S and C come from the host, which rounds the
//     reference's float thresholds (floor(Ts - 1), ceil(Tc)) once per step.
// Nothing depends on scheduling: every atomic is an integer add or or, exact whatever the order.
//
// Kernels.  k_pan_count (atomicAdd into the table, only when it is wanted) and k_pan_bits (atomicOr into the presence bit matrix, from the
// members, never from the table) both refuse a pair outside the table by flagging it and writing nothing.  The bit matrix is tile-major:
// 64-bit word bits[w * T + t] holds rows 64 w .. 64 w + 63 of taxon t, so the word of a genome IS the wave's ballot of yn for the tile,
// a row per lane; the bits behind the last row stay 0.  k_pan_type: a wave per tile, thr by a walk over the tile's words.  k_pan_curve: a
// workgroup takes a range of tiles and four orders, a wave per order; the three counts of a step are popcounts of ballots.
//   LDS tier     the tile's words, the four orders, the step thresholds and the counters per (order, step) live in the LDS; the counters
//                are flushed once per workgroup with integer atomics (tune.h PAN_LDS_BYTES bounds the taxa);
//   global tier  words, orders and thresholds are read where they lie and every step adds to the global counters.
// SOHIT_PAN_TIER forces either (the LDS tier only where it fits).  One host wait per call (DeviceCall, device_call.h), counted.
#include "device_call.h"
#include "../../include/sohit.h"

#include <cstring>
#include <string>
#include <vector>

namespace {

typedef unsigned long long ull;

enum { PAN_SPECIFIC = 0, PAN_SHARE = 1, PAN_CORE = 2 };
enum { PAN_TIER_NONE = 0, PAN_TIER_LDS = 1, PAN_TIER_GLOBAL = 2 };

// LDS bytes of k_pan_curve<true> for T taxa: words, 4 orders, (S, C) per step, 4 x 3 counters per step
size_t pan_lds_bytes(u64 T) { return (size_t)(T * 8u + 4u * T * 4u + T * 8u + 12u * (T > 0 ? T - 1 : 0) * 4u); }

// err |= 1: a row outside 0 .. n_rows - 1; err |= 2: a taxon outside 0 .. T - 1 (nothing is written for such a pair)
__device__ __forceinline__ bool pan_pair(u32 i, const int* __restrict__ row, const int* __restrict__ tax, u32 n_rows, u32 T, u32& r, u32& t, u32* __restrict__ err) {
    r = (u32)row[i], t = (u32)tax[i];
    if (r >= n_rows) {
        atomicOr(err, 1u);
        return false;
    }
    if (t >= T) {
        atomicOr(err, 2u);
        return false;
    }
    return true;
}

__global__ __launch_bounds__(256) void k_pan_count(u32 m, const int* __restrict__ row, const int* __restrict__ tax, u32 n_rows, u32 T, int* __restrict__ counts,
                                                   u32* __restrict__ err) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    u32 r, t;
    if (i < m && pan_pair(i, row, tax, n_rows, T, r, t, err)) atomicAdd(counts + (size_t)r * T + t, 1);
}

__global__ __launch_bounds__(256) void k_pan_bits(u32 m, const int* __restrict__ row, const int* __restrict__ tax, u32 n_rows, u32 T, ull* __restrict__ bits,
                                                  u32* __restrict__ err) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    u32 r, t;
    if (i < m && pan_pair(i, row, tax, n_rows, T, r, t, err)) atomicOr(bits + (size_t)(r >> 6) * T + t, 1ull << (r & 63u));
}

// a wave per tile of 64 rows, a row per lane; totals[0 .. 2] = Core, Share, Specific among the file rows
__global__ __launch_bounds__(256) void k_pan_type(const ull* __restrict__ bits, u32 n_rows, u32 n_file, u32 T, int spec_max, int core_min, u8* __restrict__ type,
                                                  ull* __restrict__ totals) {
    const u32 w = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (w >= (n_rows + 63u) / 64u) return;   // (a whole wave)
    const u32 lane = threadIdx.x & 63u, row = w * 64u + lane;
    const ull* b = bits + (size_t)w * T;
    int thr = 0;
    for (u32 t = 0; t < T; ++t) thr += (int)((b[t] >> lane) & 1ull);
    const bool file = row < n_file;   // (n_file <= n_rows)
    int ty = PAN_SPECIFIC;
    if (file && thr > spec_max) ty = thr < core_min ? PAN_SHARE : PAN_CORE;
    if (row < n_rows) type[row] = (u8)ty;
    const u32 nc = (u32)__popcll(__ballot(file && ty == PAN_CORE)), nh = (u32)__popcll(__ballot(file && ty == PAN_SHARE)),
              ns = (u32)__popcll(__ballot(file && ty == PAN_SPECIFIC));
    const u32 v = lane == 0 ? nc : lane == 1 ? nh : ns;
    if (lane < 3u && v) atomicAdd(totals + lane, (ull)v);
}

// out[(k * size + p) * (T - 1) + i - 1], k = 0 core, 1 spec, 2 panz.  grid: (ranges of `tiles` tiles, groups of 4 orders); T >= 2.
// perm rows are permutations of 0 .. T - 1 (checked on the host): every word index lies inside the tile.
template <bool LDS>
__global__ __launch_bounds__(256) void k_pan_curve(const ull* __restrict__ bits, u32 n_rows, u32 T, u32 size, const int* __restrict__ perm, const int2* __restrict__ sc,
                                                   u32 tiles, ull* __restrict__ out) {
    extern __shared__ ull pan_lds[];
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const u32 p = blockIdx.y * 4u + wave;   // this wave's order
    const bool live = p < size;
    const u32 W = (n_rows + 63u) / 64u, steps = T - 1u;
    // LDS tier: [T words][4 x T order entries][T (S, C)][4 x 3 x steps counters]
    ull* words = pan_lds;
    int* lperm = (int*)(pan_lds + T);
    int2* lsc = (int2*)(lperm + 4u * T);
    u32* acc_all = (u32*)(lsc + T);
    u32* acc = acc_all + wave * 3u * steps;
    if (LDS) {
        for (u32 k = threadIdx.x; k < 4u * T; k += 256u) {
            const u32 pp = blockIdx.y * 4u + k / T;
            lperm[k] = pp < size ? perm[(size_t)pp * T + k % T] : 0;
        }
        for (u32 k = threadIdx.x; k < T; k += 256u) lsc[k] = sc[k];
        for (u32 k = threadIdx.x; k < 12u * steps; k += 256u) acc_all[k] = 0u;
    }
    const int* pm = LDS ? lperm + wave * T : perm + (size_t)(live ? p : 0u) * T;
    const int2* thr = LDS ? lsc : sc;
    const u32 w0 = blockIdx.x * tiles, w1 = min(W, w0 + tiles);
    for (u32 w = w0; w < w1; ++w) {   // (the same range for every wave of the workgroup: the barriers below are met by all)
        const ull* b = bits + (size_t)w * T;
        if (LDS) {
            __syncthreads();   // the last tile's readers are done (first round: the tables above are complete)
            for (u32 k = threadIdx.x; k < T; k += 256u) words[k] = b[k];
            __syncthreads();
        }
        if (!live) continue;
        const ull* src = LDS ? words : b;
        const ull mask = (w == W - 1u && (n_rows & 63u)) ? (1ull << (n_rows & 63u)) - 1ull : ~0ull;   // the rows the last tile has
        int ys = (int)((src[pm[0]] >> lane) & 1ull);
        ull word = src[pm[1]];   // == ballot(yn) of step 1
        int2 t = thr[1];
        for (u32 i = 1; i < T; ++i) {
            const u32 nx = i + 1u < T ? i + 1u : i;   // the next step's word and thresholds travel while this step counts
            const ull word_nx = src[pm[nx]];
            const int2 t_nx = thr[nx];
            const u32 nspec = (u32)__popcll(__ballot(ys <= t.x) & word & mask);
            ys += (int)((word >> lane) & 1ull);
            const u32 ncore = (u32)__popcll(__ballot(ys >= t.y) & mask);
            const u32 npanz = (u32)__popcll(__ballot(ys > 0) & mask);
            const u32 v = lane == 0 ? ncore : lane == 1 ? nspec : npanz;
            if (lane < 3u) {
                if (LDS)
                    acc[lane * steps + i - 1u] += v;   // (the wave owns its counters: no other wave touches them)
                else if (v)
                    atomicAdd(out + ((size_t)lane * size + p) * steps + i - 1u, (ull)v);
            }
            word = word_nx, t = t_nx;
        }
    }
    if (LDS) {
        __syncthreads();
        for (u32 k = threadIdx.x; k < 12u * steps; k += 256u) {
            const u32 pp = blockIdx.y * 4u + k / (3u * steps), kind = (k % (3u * steps)) / steps, i = k % steps;
            const u32 v = acc_all[k];
            if (pp < size && v) atomicAdd(out + ((size_t)kind * size + pp) * steps + i, (ull)v);
        }
    }
}

thread_local std::string g_pan_err;

auto slots(so_pan_result* r) { return result_slots(&r->counts, &r->type, &r->core, &r->spec, &r->panz); }

}  // namespace

extern "C" {

const char* so_pan_last_error(void) { return g_pan_err.c_str(); }

void so_pan_free(so_pan_result* r) {
    if (r) release_slots(r, slots(r));
}

int so_pan_genome(int device, int64_t m, const int32_t* row, const int32_t* taxon, int64_t n_rows, int64_t n_file_rows, int64_t n_taxa, int32_t spec_max, int32_t core_min,
                  int64_t size, const int32_t* perm, const int32_t* S, const int32_t* C, int32_t want_counts, int32_t flags, so_pan_result* out) {
    const std::string who = "so_pan_genome";
    return guarded_call(g_pan_err, out, so_pan_free, [&] {
        if (!out) throw SoError(who + ": result pointer is NULL");
        memset(out, 0, sizeof *out);
        if (flags != 0) throw SoError(who + ": flags is reserved and must be 0");
        if (m < 0 || n_rows < 0 || n_file_rows < 0 || n_file_rows > n_rows || n_taxa < 0 || size < 0) throw SoError(who + ": bad arguments");
        if (n_rows >= (1ll << 31)) throw SoError(who + ": 2^31 rows and more are not supported");
        if (m >= (1ll << 31)) throw SoError(who + ": 2^31 members and more are not supported");
        if (n_taxa >= (1ll << 31)) throw SoError(who + ": 2^31 taxa and more are not supported");
        if (want_counts && (u64)n_rows * (u64)n_taxa >= (1ull << 31)) throw SoError(who + ": a count matrix of 2^31 cells and more (rows x taxa) is not supported");
        const u64 steps = n_taxa > 1 ? (u64)n_taxa - 1 : 0, cells = (u64)size * steps;
        if (cells >= (1ull << 31) || (u64)size * (u64)n_taxa >= (1ull << 31)) throw SoError(who + ": 2^31 curve points and more (orders x taxa) are not supported");
        if (m > 0 && (!row || !taxon)) throw SoError(who + ": a member column is NULL");
        if (cells > 0 && (!perm || !S || !C)) throw SoError(who + ": perm, S or C is NULL");
        if (m > 0 && n_rows == 0) throw SoError(who + ": a row outside 0 .. n_rows - 1");
        if (m > 0 && n_taxa == 0) throw SoError(who + ": a taxon outside 0 .. n_taxa - 1");
        if (cells > 0) {   // every order a permutation: the kernel indexes a tile's words with it
            std::vector<u8> seen((size_t)n_taxa);
            for (i64 p = 0; p < size; ++p) {
                std::fill(seen.begin(), seen.end(), (u8)0);
                for (i64 t = 0; t < n_taxa; ++t) {
                    const int32_t v = perm[p * n_taxa + t];
                    if (v < 0 || v >= n_taxa || seen[(size_t)v]) throw SoError(who + ": perm row " + std::to_string(p) + " is not a permutation of 0 .. n_taxa - 1");
                    seen[(size_t)v] = 1;
                }
            }
        }
        out->n_rows = n_rows, out->n_taxa = n_taxa, out->size = size;
        check_device(who.c_str(), device);
        if (n_rows == 0) {   // nothing to launch: no rows, every count 0
            out->core = host_array<int64_t>(who.c_str(), cells), out->spec = host_array<int64_t>(who.c_str(), cells), out->panz = host_array<int64_t>(who.c_str(), cells);
            memset(out->core, 0, cells * 8), memset(out->spec, 0, cells * 8), memset(out->panz, 0, cells * 8);
            fill_empty_slots(slots(out));
            return;
        }
        DeviceCall call(device);
        hipStream_t st = call.st;
        const u32 M = (u32)m, R = (u32)n_rows, T = (u32)n_taxa, W = (R + 63u) / 64u;
        DevBuf<int> d_row, d_tax, d_perm, d_counts;
        DevBuf<int2> d_sc;
        DevBuf<ull> bits, curve, totals;
        DevBuf<u32> err;
        DevBuf<u8> type;
        const size_t nbits = (size_t)W * T, ncount = want_counts ? (size_t)R * T : 0;
        upload(d_row, row, (size_t)m, st), upload(d_tax, taxon, (size_t)m, st);
        bits.ensure(nbits + 2), totals.ensure(4), err.ensure(4), type.ensure((size_t)R + 2), curve.ensure(3 * (size_t)cells + 2);
        if (nbits) HIP_CHECK(hipMemsetAsync(bits.p, 0, nbits * sizeof(ull), st));
        HIP_CHECK(hipMemsetAsync(totals.p, 0, 3 * sizeof(ull), st));
        HIP_CHECK(hipMemsetAsync(err.p, 0, sizeof(u32), st));
        if (want_counts) {
            d_counts.ensure(ncount + 2);
            if (ncount) HIP_CHECK(hipMemsetAsync(d_counts.p, 0, ncount * sizeof(int), st));
        }
        if (M) {
            if (want_counts) hipLaunchKernelGGL(k_pan_count, grid256(M), dim3(256), 0, st, M, d_row.p, d_tax.p, R, T, d_counts.p, err.p);
            hipLaunchKernelGGL(k_pan_bits, grid256(M), dim3(256), 0, st, M, d_row.p, d_tax.p, R, T, bits.p, err.p);
        }
        hipLaunchKernelGGL(k_pan_type, dim3((W + 3u) / 4u), dim3(256), 0, st, bits.p, R, (u32)n_file_rows, T, (int)spec_max, (int)core_min, type.p, totals.p);
        if (cells) {
            std::vector<int2> sc((size_t)T);
            for (u32 i = 0; i < T; ++i) sc[i] = make_int2(S[i], C[i]);
            upload(d_sc, sc.data(), sc.size(), st), upload(d_perm, perm, (size_t)size * T, st);
            HIP_CHECK(hipMemsetAsync(curve.p, 0, 3 * (size_t)cells * sizeof(ull), st));
            const size_t lds = pan_lds_bytes(T);
            const bool use_lds = lds <= PAN_LDS_BYTES && call.tn.pan_tier != ORTH_TIER_SCRATCH;   // (forcing the LDS tier changes nothing: it takes what it can hold)
            const u32 tiles = (W + PAN_TILE_RANGES - 1u) / PAN_TILE_RANGES;
            const dim3 grid((W + tiles - 1u) / tiles, (u32)((size + 3) / 4));
            if (use_lds)
                hipLaunchKernelGGL(k_pan_curve<true>, grid, dim3(256), lds, st, bits.p, R, T, (u32)size, d_perm.p, d_sc.p, tiles, curve.p);
            else
                hipLaunchKernelGGL(k_pan_curve<false>, grid, dim3(256), 0, st, bits.p, R, T, (u32)size, d_perm.p, d_sc.p, tiles, curve.p);
            out->tier = use_lds ? PAN_TIER_LDS : PAN_TIER_GLOBAL;
        }
        HIP_CHECK(hipGetLastError());
        u32 e = 0;
        ull tot[3] = {0, 0, 0};
        call.fetch(&e, err.p), call.fetch(tot, totals.p, 3);
        const char* w = who.c_str();
        out->type = host_copy(w, type.p, (size_t)R, st);
        if (want_counts) out->counts = host_copy(w, d_counts.p, ncount, st);
        static_assert(sizeof(ull) == sizeof(int64_t), "the counters are copied out as int64");
        out->core = (int64_t*)host_copy(w, curve.p, (size_t)cells, st);
        out->spec = (int64_t*)host_copy(w, curve.p + cells, (size_t)cells, st);
        out->panz = (int64_t*)host_copy(w, curve.p + 2 * cells, (size_t)cells, st);
        call.wait();
        out->waits = call.waits;
        if (e & 1u) throw SoError(who + ": a row outside 0 .. n_rows - 1");
        if (e & 2u) throw SoError(who + ": a taxon outside 0 .. n_taxa - 1");
        out->n_core = (i64)tot[0], out->n_share = (i64)tot[1], out->n_spec = (i64)tot[2];
        fill_empty_slots(slots(out));
    });
}

}  // extern "C"
