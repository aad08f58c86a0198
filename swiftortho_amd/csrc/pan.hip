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
//
// so_pan_shared: what pan.py `shared_counts()` and `boot_shared()` define -- S[a][b] = the rows present in both a and b, over all rows or
// over the rows a bootstrap replicate draws (a row drawn twice counts twice).  S = P^T P of the presence bits is AND + popcount over the
// tile-major words: k_pan_shared, a workgroup per 64 x 64 tile of taxon pairs (the upper triangle of tiles only) and range of row words,
// 4 x 4 sums per lane, integer adds into the int32 result.  A replicate is a presence matrix of its own: k_pan_rowbits writes the bits
// row-major, k_pan_draw draws 64 rows per wave (phy.py boot_columns with K = n_rows), reads each drawn row's word for a block of 64 taxa
// and transposes the 64 x 64 bits with 64 ballots into the replicate's tile-major words.  Replicates run along the grid, in batches whose
// words fit half of the free device memory (SOHIT_PAN_BOOT_BATCH forces the size); SOHIT_PAN_SHARED_RANGES forces the number of ranges.
// Integers only, one host wait per call whatever the number of batches.
#include "pan_bits.h"
#include "../../include/sohit.h"

#include <cstring>
#include <string>
#include <tuple>
#include <vector>

namespace {

enum { PAN_SPECIFIC = 0, PAN_SHARE = 1, PAN_CORE = 2 };
enum { PAN_TIER_NONE = 0, PAN_TIER_LDS = 1, PAN_TIER_GLOBAL = 2 };

// LDS bytes of k_pan_curve<true> for T taxa: words, 4 orders, (S, C) per step, 4 x 3 counters per step
size_t pan_lds_bytes(u64 T) { return (size_t)(T * 8u + 4u * T * 4u + T * 8u + 12u * (T > 0 ? T - 1 : 0) * 4u); }

// (pan_pair, the check of a member pair, and k_pan_rowbits, the row-major presence words of the draws: pan_bits.h)
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

// ---- so_pan_shared: the families every pair of genomes shares, S = P^T P of the presence matrix, for the table or for bootstrap replicates ----
// grid (groups of 4 draw tiles, groups of PAN_DRAW_BLOCKS blocks of 64 taxa, replicates); a wave per tile of 64 draws, a draw per lane.
// Lane k reads the row-major word of its drawn row for a block of 64 taxa; ballot j is then bit j of all 64 lanes -- the tile-major word
// of taxon 64 tb + j over the 64 drawn rows, which lane j keeps and stores: words[z][w * T + t] as k_pan_bits writes them.  A lane behind
// the last draw holds 0, so the bits behind the last row stay 0.  A draw lies below R and tb below TW: every read is inside rowbits.
__global__ __launch_bounds__(256) void k_pan_draw(const ull* __restrict__ rowbits, u32 R, u32 T, u32 TW, ull seed, u32 b0, ull* __restrict__ words, size_t wrep) {
    const u32 w = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (w >= (R + 63u) / 64u) return;   // (a whole wave)
    const u32 lane = threadIdx.x & 63u, d = w * 64u + lane;
    const bool live = d < R;
    const ull* src = rowbits + (live ? (size_t)replicate_draw(seed, (ull)b0 + blockIdx.z, d, R) * TW : 0);
    ull* dst = words + (size_t)blockIdx.z * wrep + (size_t)w * T;
    const u32 tb0 = blockIdx.y * PAN_DRAW_BLOCKS, tb1 = min(TW, tb0 + PAN_DRAW_BLOCKS);
    for (u32 tb = tb0; tb < tb1; ++tb) {   // (the same bounds for every lane: the ballots are met by the whole wave)
        const ull word = live ? src[tb] : 0ull;
        ull mine = 0ull;
#pragma unroll
        for (u32 j = 0; j < 64u; ++j) {
            const ull bal = __ballot((word >> j) & 1ull);
            if (lane == j) mine = bal;
        }
        const u32 t = tb * 64u + lane;
        if (t < T) dst[t] = mine;
    }
}

// S += A^T B over a range of row words.  grid (tiles of 64 x 64 taxon pairs with I <= J, ranges of `wps` row words, matrices); words: per
// matrix W row words of T taxa, tile-major.  Lane (ty, tx) of the 16 x 16 holds taxa I * 64 + ty * 4 + r against J * 64 + tx * 4 + c.  A
// chunk of PAN_SH_CHUNK row words of both sides lies in the LDS as [word][taxon]: a lane's four taxa are 32 consecutive bytes, the 16
// lanes of one ty read one address (a broadcast).  The range's sums (below 2^31: 64 per word, fewer than 2^25 words) flush with integer
// adds, the mirror entry too; a diagonal tile holds both (x, y) and (y, x) itself and writes each once.
__global__ __launch_bounds__(256) void k_pan_shared(const ull* __restrict__ words, u32 W, u32 T, u32 nt, u32 wps, int* __restrict__ out, size_t wrep, size_t orep) {
    words += (size_t)blockIdx.z * wrep, out += (size_t)blockIdx.z * orep;
    __shared__ __attribute__((aligned(16))) ull sA[PAN_SH_CHUNK][PAN_SH_TILE];
    __shared__ __attribute__((aligned(16))) ull sB[PAN_SH_CHUNK][PAN_SH_TILE];
    u32 I = 0, J = blockIdx.x;   // the blockIdx.x-th pair I <= J in row-major order
    while (J >= nt - I) J -= nt - I, ++I;
    J += I;
    const u32 w_begin = blockIdx.y * wps, w_end = min(W, w_begin + wps);
    if (w_begin >= w_end) return;   // (the whole workgroup)
    const u32 tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const u32 lcol = threadIdx.x & 63u, lpart = threadIdx.x >> 6;
    const u32 ta = I * PAN_SH_TILE + lcol, tb = J * PAN_SH_TILE + lcol;
    u32 acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0u;
    for (u32 w0 = w_begin; w0 < w_end; w0 += PAN_SH_CHUNK) {
        const u32 nw = min((u32)PAN_SH_CHUNK, w_end - w0);
        __syncthreads();   // the last chunk's readers are done
        for (u32 k = lpart; k < nw; k += 4u) {
            const ull* src = words + (size_t)(w0 + k) * T;   // w0 + k < w_end <= W
            sA[k][lcol] = ta < T ? src[ta] : 0ull;
            sB[k][lcol] = tb < T ? src[tb] : 0ull;
        }
        __syncthreads();
        for (u32 k = 0; k < nw; ++k) {
            const ulonglong2 a0 = *reinterpret_cast<const ulonglong2*>(&sA[k][ty * 4u]), a1 = *reinterpret_cast<const ulonglong2*>(&sA[k][ty * 4u + 2u]);
            const ulonglong2 b0 = *reinterpret_cast<const ulonglong2*>(&sB[k][tx * 4u]), b1 = *reinterpret_cast<const ulonglong2*>(&sB[k][tx * 4u + 2u]);
            const ull av[4] = {a0.x, a0.y, a1.x, a1.y}, bv[4] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] += (u32)__popcll(av[r] & bv[c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const u32 x = I * PAN_SH_TILE + ty * 4u + (u32)r, y = J * PAN_SH_TILE + tx * 4u + (u32)c;
            if (x >= T || y >= T || !acc[r][c]) continue;
            atomicAdd(out + (size_t)x * T + y, (int)acc[r][c]);
            if (I != J) atomicAdd(out + (size_t)y * T + x, (int)acc[r][c]);
        }
}

// the grid of k_pan_shared over W row words and `reps` matrices of nt x nt tiles: (row words per range, ranges).  forced > 0: that many
// ranges (as far as there are words); else whole chunks, until about PAN_SH_TARGET_WGS workgroups exist.  Never more than 2^23 workgroups.
std::pair<u32, u32> shared_grid(u32 W, u32 nt, u32 reps, long long forced) {
    const u64 tiles = (u64)(nt * (nt + 1u) / 2u) * reps;
    return range_grid(W, PAN_SH_CHUNK, tiles, PAN_SH_TARGET_WGS, forced, (u32)std::max<u64>(1, std::min<u64>(65535, (1ull << 23) / tiles)));
}

thread_local std::string g_pan_err;

auto slots(so_pan_result* r) { return result_slots(&r->counts, &r->type, &r->core, &r->spec, &r->panz); }
auto slots(so_pan_shared_result* r) { return result_slots(&r->shared); }

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
        if (cells) {   // k_pan_curve's grid is ceil(size / 4) workgroups high: with few taxa the bounds above allow far more than a launch takes
            int max_y = 0;
            HIP_CHECK(hipDeviceGetAttribute(&max_y, hipDeviceAttributeMaxGridDimY, device));   // hipDeviceProp_t::maxGridSize[1]
            if ((size + 3) / 4 > (i64)max_y)
                throw SoError(who + ": " + std::to_string(size) + " orders are more than one call serves: the curve kernel's grid is a workgroup per 4 orders and at most " +
                              std::to_string(max_y) + " high on this device (the largest size served is " + std::to_string(4 * (i64)max_y) + ")");
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

void so_pan_shared_free(so_pan_shared_result* r) {
    if (r) release_slots(r, slots(r));
}

int so_pan_shared(int device, int64_t m, const int32_t* row, const int32_t* taxon, int64_t n_rows, int64_t n_taxa, uint64_t seed, int64_t b0, int64_t n_reps, int32_t flags,
                  so_pan_shared_result* out) {
    const std::string who = "so_pan_shared";
    return guarded_call(g_pan_err, out, so_pan_shared_free, [&] {
        if (!out) throw SoError(who + ": result pointer is NULL");
        memset(out, 0, sizeof *out);
        if (flags & ~3) throw SoError(who + ": unknown flag bits (bit 0: no matrix in the result, bit 1: draw and product timed by events)");
        if (m < 0 || n_rows < 0) throw SoError(who + ": bad arguments");
        if (n_taxa < 1 || n_taxa > PAN_MAX_TAXA) throw SoError(who + ": the taxa number 1 .. " + std::to_string(PAN_MAX_TAXA) + " (n_taxa is " + std::to_string(n_taxa) + ")");
        if (n_rows >= (1ll << 31)) throw SoError(who + ": 2^31 rows and more are not supported");
        if (m >= (1ll << 31)) throw SoError(who + ": 2^31 members and more are not supported");
        if (n_reps < 0) throw SoError(who + ": n_reps is 0 (all rows) or the number of replicates (n_reps is " + std::to_string(n_reps) + ")");
        if (n_reps > PAN_BOOT_MAX_REPS) throw SoError(who + ": more than " + std::to_string(PAN_BOOT_MAX_REPS) + " replicates in one call are not supported");
        const bool draw = n_reps > 0;
        if (draw && (b0 < 0 || b0 >= (1ll << 31) || b0 + n_reps > (1ll << 31))) throw SoError(who + ": replicates beyond 2^31 - 1 are not supported");
        if (draw && n_rows == 0) throw SoError(who + ": no row to draw from (n_rows is 0)");
        if (m > 0 && (!row || !taxon)) throw SoError(who + ": a member column is NULL");
        if (m > 0 && n_rows == 0) throw SoError(who + ": a row outside 0 .. n_rows - 1");
        const bool want = !(flags & 1), timed = flags & 2;
        const u32 M = (u32)m, R = (u32)n_rows, T = (u32)n_taxa, W = (R + 63u) / 64u, TW = (T + 63u) / 64u, nrep = draw ? (u32)n_reps : 1u;
        const size_t TT = (size_t)T * T, bytes = (size_t)nrep * TT * sizeof(int);
        out->n_taxa = n_taxa, out->n_reps = nrep, out->bytes = (int64_t)bytes;
        check_device(who.c_str(), device);
        if (n_rows == 0) {   // nothing to launch: no rows, every count 0
            if (want) {
                out->shared = host_array<int32_t>(who.c_str(), TT);
                memset(out->shared, 0, TT * sizeof(int32_t));
            }
            fill_empty_slots(slots(out));
            return;
        }
        DeviceCall call(device);
        hipStream_t st = call.st;
        refuse_over_half_free(who, "result of " + std::to_string(nrep) + " x " + std::to_string(T) + " x " + std::to_string(T) + " counts", bytes);
        DevBuf<int> d_row, d_tax, d_out;
        DevBuf<ull> bits, words;
        DevBuf<u32> err;
        upload(d_row, row, (size_t)m, st), upload(d_tax, taxon, (size_t)m, st);
        const size_t per = (size_t)W * T, nbits = draw ? (size_t)R * TW : per;   // words of one matrix; of the presence bits (row-major for the draws)
        d_out.ensure((size_t)nrep * TT + 2), bits.ensure(nbits + 2), err.ensure(4);
        HIP_CHECK(hipMemsetAsync(d_out.p, 0, bytes, st));
        HIP_CHECK(hipMemsetAsync(bits.p, 0, nbits * sizeof(ull), st));
        HIP_CHECK(hipMemsetAsync(err.p, 0, sizeof(u32), st));
        if (M) {
            if (draw)
                hipLaunchKernelGGL(k_pan_rowbits, grid256(M), dim3(256), 0, st, M, d_row.p, d_tax.p, R, T, TW, bits.p, err.p);
            else
                hipLaunchKernelGGL(k_pan_bits, grid256(M), dim3(256), 0, st, M, d_row.p, d_tax.p, R, T, bits.p, err.p);
        }
        const u32 nt = (T + PAN_SH_TILE - 1u) / PAN_SH_TILE;
        StageEvents ev(timed);   // no draw: marks 0, 1 around the product; else marks 3 k .. 3 k + 2 around the draw and the product of batch k; read behind the call's one wait
        u32 wps = 0, ranges = 0;
        if (!draw) {
            std::tie(wps, ranges) = shared_grid(W, nt, 1u, call.tn.pan_shared_ranges);
            ev.mark(0, st);
            hipLaunchKernelGGL(k_pan_shared, dim3(nt * (nt + 1u) / 2u, ranges, 1u), dim3(256), 0, st, bits.p, W, T, nt, wps, d_out.p, (size_t)0, (size_t)0);
            ev.mark(1, st);
            out->batches = 1;
        } else {
            // a batch: as many replicates' words as half of what is free now holds, below 2^31 words and 2^22 tiles (grid sizes)
            const size_t cap = std::min({(size_t)nrep, ((size_t)1 << 31) / per, ((size_t)1 << 22) / (nt * (nt + 1u) / 2u)});
            const size_t batch = std::max<size_t>(1, device_batch(call, call.tn.pan_boot_batch, (per + 64) * sizeof(ull), cap));
            words.ensure(batch * per + 2);
            for (u32 r0 = 0; r0 < nrep; r0 += (u32)batch) {
                const u32 nb = std::min((u32)batch, nrep - r0);
                const size_t k = 3u * (size_t)out->batches++;   // the batch's first mark
                std::tie(wps, ranges) = shared_grid(W, nt, nb, call.tn.pan_shared_ranges);
                ev.mark(k, st);
                hipLaunchKernelGGL(k_pan_draw, dim3((W + 3u) / 4u, (TW + PAN_DRAW_BLOCKS - 1u) / PAN_DRAW_BLOCKS, nb), dim3(256), 0, st, bits.p, R, T, TW, (ull)seed,
                                   (u32)b0 + r0, words.p, per);
                ev.mark(k + 1, st);
                hipLaunchKernelGGL(k_pan_shared, dim3(nt * (nt + 1u) / 2u, ranges, nb), dim3(256), 0, st, words.p, W, T, nt, wps, d_out.p + (size_t)r0 * TT, per, TT);
                ev.mark(k + 2, st);
            }
        }
        out->ranges = (int32_t)ranges;
        HIP_CHECK(hipGetLastError());
        u32 e = 0;
        call.fetch(&e, err.p);
        static_assert(sizeof(int) == sizeof(int32_t), "the counts are copied out as int32");
        if (want) out->shared = host_copy(who.c_str(), d_out.p, (size_t)nrep * TT, st);
        call.wait();
        out->waits = call.waits;
        if (e & 1u) throw SoError(who + ": a row outside 0 .. n_rows - 1");
        if (e & 2u) throw SoError(who + ": a taxon outside 0 .. n_taxa - 1");
        if (!draw) out->product_ms = ev.ms(0);
        else
            for (size_t k = 0; k < 3u * (size_t)out->batches; k += 3) out->draw_ms += ev.ms(k), out->product_ms += ev.ms(k + 1);
        fill_empty_slots(slots(out));
    });
}

}  // extern "C"
