// phy.hip -- the core-gene supermatrix from the hits' own alignments, on the device: what swiftortho_amd/phy.py `pick_rows()`, `project()`,
// `supermatrix()` and `pair_counts()` define.  Every member of a core family is the best hit of the family's anchor gene in its taxon, so the
// search has aligned exactly that pair: the member's residues are laid onto the anchor's coordinates along the row's CIGAR (M: copied,
// I: the columns stay '-', D: the residues are dropped), the blocks of the families side by side are the supermatrix, and the counts of
// compared and equal columns per pair of taxa are what the distances are made from.
//
// The numpy functions are the definition; all of it is integer and byte work, so every result is exact whatever the scheduling:
//   so_phy_rows   the wanted (anchor, member) pairs as 64-bit keys, sorted once; every hit row finds its key by binary search.  Pass 1: an
//                 integer atomicMax of the order-preserving bit pattern of the score (-0.0 counts as 0.0); pass 2: an atomicMin of the
//                 row number among the rows that hold the maximum.  No float is ever compared on the device.
//   so_phy_build  k_phy_project   a wave per (family, slot) task: the run lengths are summed and checked against both sequences BEFORE any
//                                 store (a bad task flags itself and writes nothing), a wave-wide scan gives every run its two starts,
//                                 and the wave copies the M runs one after the other, a byte per lane;
//                 k_phy_gaps      '-' per column and the keep flag gaps <= floor(g * T); scan_u32 + k_phy_keep compact the kept columns;
//                 k_phy_gather    the kept columns of every taxon side by side, padded with '-' to a multiple of 16 bytes;
//                 k_phy_pairs     a workgroup owns a tile of 64 x 64 taxon pairs and a range of kept columns, staged chunk by chunk in the
//                                 LDS as [word][row] with the non-gap masks next to them; four residues per 32-bit word: a byte is
//                                 non-zero where ((x & 0x7f7f7f7f) + 0x7f7f7f7f | x) has its top bit; counts in registers, one flush per
//                                 workgroup with 64-bit integer atomics.  Only tiles I <= J are walked; the flush writes both halves.
// One host wait per call (DeviceCall, device_call.h), counted.
//
// Bootstrap support of the neighbour-joining tree (phy.py boot_columns, boot_counts, nj_splits, split_support, bootstrap):
//   so_phy_boot_counts  k_phy_boot_gather  a lane per drawn column: the draw is splitmix64 of (replicate, column) in 64-bit integers, scaled by
//                                          a multiply and a shift; the replicate's columns side by side, padded as k_phy_gather pads;
//                       k_phy_pairs        the same tiles, the replicates of a batch along the grid's third dimension.
//   so_phy_nj_splits    k_phy_nj           a workgroup per matrix.  D stays in global memory; the live list, the row sums and the clade bit
//                                          sets are LDS (the bit sets move to global scratch beyond 640 taxa).  A row sum runs left to right
//                                          over the live nodes -- the one order a lane can reproduce --, the minimum of (Q, i, j) is a
//                                          lexicographic reduction, the new row is written on both sides of the diagonal.  Plain IEEE
//                                          doubles, nothing fused: the splits equal numpy's bit for bit.
//   so_phy_boot         the fused path of the p distance: gather, pairs, k_phy_boot_dist (D = 1 - same / cmp; a pair without a compared
//                       column drops the replicate), k_phy_nj, k_phy_boot_support (a lane per split of the printed tree).  Batches of
//                       replicates sized from the free device memory (SOHIT_PHY_BOOT_BATCH), one host wait per batch.
//
// The substitution counts the Kimura and LogDet distances need (phy.py subst_counts, boot_subst):
//   so_phy_subst        k_phy_code         a lane per kept (or drawn) column: the residue codes 0 .. 19, 0xFF for every other byte and for the
//                                          padding of a row to the k-step;
//                       k_phy_subst        N = E E^T on the matrix cores (v_mfma_i32_32x32x32_i8, i32 accumulators), E the one-hot matrix
//                                          of 20 rows per taxon, never written: a lane compares 16 staged codes with its row's residue.
//                                          Integers only; determinants and logarithms stay on the host.
//
// Gene concordance factors of the species tree (phy.py family_counts, family_present, gene_distances, nj_splits_subset, concordance):
//   so_phy_gene_counts  k_phy_fam_gather   the kept columns family by family, each family's range padded with '-' to a multiple of 16 bytes;
//                       k_phy_fam_pairs    the tile walk of k_phy_pairs (pairs_tile_walk) over one family's words, a workgroup per (tile,
//                                          family): plain 32-bit stores, no atomics, nothing to clear.
//   so_phy_nj_subsets   k_phy_nj_subset    the walk of k_phy_nj (nj_walk) over the taxa a family holds: the live list starts as the present
//                                          bits, a clade with the lowest present taxon is complemented inside the present set.
//   so_phy_gene         the fused path of the p distance: gather, pairs, k_phy_gene_dist (D = 1 - same / cmp among the present taxa, the present
//                       words and their count from the diagonal; two present taxa without a compared column drop the family), k_phy_nj_subset,
//                       k_phy_gene_concord (a lane per (split of the printed tree, family): popcounts, the canonical side, a search in the
//                       family's splits, integer atomicAdd).  Batches of families sized from the free device memory
//                       (SOHIT_PHY_GENE_BATCH), one host wait per batch.
//
// What the bootstrap and the concordance stage share with each other and with pan.hip is in tree_stage.h: the draw (replicate_draw), the
// grids of the kernels that walk a length in ranges (range_grid), the batch size (device_batch) and the stage timer (StageEvents).  Here:
// matrix_check (what every call over a matrix and its kept columns checks), nj_call (so_phy_nj_splits and so_phy_nj_subsets: one body) and
// nj_launch (either kernel of the walk).  The flush of a lane's 4 x 4 block stays written out in k_phy_pairs, k_phy_fam_pairs and
// k_pan_shared, and the search of a split in k_phy_boot_support and k_phy_gene_concord: through a shared inline function the compiler gave
// these kernels other code (two more scalar registers in two of them, k_pan_shared's product 4 % slower by events).
#include "tree_stage.h"
#include "../../include/sohit.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

namespace {

#define PHY_DASH 0x2Du
#define PHY_DASH4 0x2D2D2D2Du
enum { PHY_E_START = 1, PHY_E_RUN = 2, PHY_E_QEND = 4, PHY_E_SEND = 8, PHY_E_ANCHOR = 16 };

// ---- so_phy_rows ---------------------------------------------------------------------------------------------------------------------
// the bits of a double (no NaN) -> an unsigned number that orders like the value; -0.0 and 0.0 give the same number, every number is > 0
__device__ __forceinline__ ull score_order(ull bits) {
    if (bits == 0x8000000000000000ull) bits = 0ull;
    return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);
}
// first position of key among the m sorted keys, or NONE32
__device__ __forceinline__ u32 phy_find(const ull* __restrict__ sk, u32 m, ull key) {
    u32 lo = 0, hi = m;
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (sk[mid] < key) lo = mid + 1u;
        else hi = mid;
    }
    return (lo < m && sk[lo] == key) ? lo : NONE32;
}
__device__ __forceinline__ ull phy_key(int q, int s) { return ((ull)(u32)q << 32) | (ull)(u32)s; }

__global__ __launch_bounds__(256) void k_phy_row_max(u32 n, const int* __restrict__ q, const int* __restrict__ s, const ull* __restrict__ score, const ull* __restrict__ sk,
                                                     u32 m, u32* __restrict__ slot_of, ull* __restrict__ best) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const u32 slot = phy_find(sk, m, phy_key(q[i], s[i]));
    slot_of[i] = slot;
    if (slot != NONE32) atomicMax(best + slot, score_order(score[i]));
}
__global__ __launch_bounds__(256) void k_phy_row_first(u32 n, const ull* __restrict__ score, const u32* __restrict__ slot_of, const ull* __restrict__ best,
                                                       u32* __restrict__ first) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const u32 slot = slot_of[i];
    if (slot != NONE32 && score_order(score[i]) == best[slot]) atomicMin(first + slot, i);
}
__global__ __launch_bounds__(256) void k_phy_row_out(u32 np, const ull* __restrict__ pkey, const ull* __restrict__ sk, const u32* __restrict__ first, u32* __restrict__ row) {
    const u32 p = blockIdx.x * 256u + threadIdx.x;
    if (p >= np) return;
    const u32 slot = phy_find(sk, np, pkey[p]);   // (always found: sk holds the same keys)
    row[p] = slot == NONE32 ? NONE32 : first[slot];
}

// ---- so_phy_build ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 wave_incl_scan(u32 v, u32 lane) {
#pragma unroll
    for (u32 d = 1; d < 64u; d <<= 1) {
        const u32 t = (u32)__shfl_up((int)v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ ull wave_sum64(ull v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (ull)__shfl_xor((long long)v, d, 64);
    return v;
}

struct PhyTasks {
    const int *fam, *slot, *res_len, *qst, *sst;
    const u8* kind;
    const i64 *res_off, *run_off;
};

// a wave per task.  The host has checked what a task names (family, slot, its slice of the residues and of the runs); the wave checks what
// the runs do inside the block and inside the member before it stores anything.  err[0]: the PHY_E_* bits, err[1]: the lowest bad task.
__global__ __launch_bounds__(256) void k_phy_project(u32 n_tasks, PhyTasks tk, const u32* __restrict__ runs, const u8* __restrict__ res, const i64* __restrict__ col_off, u64 L,
                                                     u8* __restrict__ matrix, u32* __restrict__ err) {
    const u32 t = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (t >= n_tasks) return;   // (a whole wave)
    const u32 lane = threadIdx.x & 63u;
    const int f = tk.fam[t];
    const i64 c0 = col_off[f];
    const u32 alen = (u32)(col_off[f + 1] - c0), rlen = (u32)tk.res_len[t];
    u8* dst = matrix + (size_t)tk.slot[t] * L + (size_t)c0;
    const u8* src = res + tk.res_off[t];
    u32 bad = 0;
    if (tk.kind[t]) {   // the anchor itself: its residues are the block's row
        if (rlen != alen) bad = PHY_E_ANCHOR;
        else
            for (u32 x = lane; x < alen; x += 64u) dst[x] = src[x];
    } else {
        const i64 r0 = tk.run_off[t];
        const u64 nr = (u64)(tk.run_off[t + 1] - r0);
        const int qs = tk.qst[t], ss = tk.sst[t];
        if (qs < 1 || ss < 1) bad |= PHY_E_START;
        ull qsum = 0, ssum = 0;
        bool badrun = false;
        for (u64 k = lane; k < nr; k += 64u) {
            const u32 v = runs[r0 + (i64)k], len = v >> 4, op = v & 15u;
            if (len == 0u || op > 2u) badrun = true;
            else {
                if (op != 2u) qsum += len;
                if (op != 1u) ssum += len;
            }
        }
        qsum = wave_sum64(qsum), ssum = wave_sum64(ssum);
        if (__any(badrun)) bad |= PHY_E_RUN;
        if (!bad) {
            if ((ull)(qs - 1) + qsum > (ull)alen) bad |= PHY_E_QEND;
            if ((ull)(ss - 1) + ssum > (ull)rlen) bad |= PHY_E_SEND;
        }
        if (!bad) {   // (wave-uniform: every sum above is)
            u32 qp = (u32)(qs - 1), sp = (u32)(ss - 1);
            for (u64 base = 0; base < nr; base += 64u) {
                const u64 k = base + lane;
                const u32 v = k < nr ? runs[r0 + (i64)k] : 0u, len = v >> 4, op = v & 15u;
                const u32 qa = op != 2u ? len : 0u, sa = op != 1u ? len : 0u;
                const u32 qi = wave_incl_scan(qa, lane), si = wave_incl_scan(sa, lane);
                const u32 my_q = qp + qi - qa, my_s = sp + si - sa;
                ull m = __ballot(k < nr && op == 0u);
                while (m) {   // the M runs of these 64, one after the other, the wave copying each
                    const int j = __ffsll((long long)m) - 1;
                    m &= m - 1ull;
                    const u32 n = (u32)__shfl((int)len, j, 64), q0 = (u32)__shfl((int)my_q, j, 64), s0 = (u32)__shfl((int)my_s, j, 64);
                    for (u32 x = lane; x < n; x += 64u) dst[q0 + x] = src[s0 + x];
                }
                qp += (u32)__shfl((int)qi, 63, 64), sp += (u32)__shfl((int)si, 63, 64);
            }
        }
    }
    if (bad && lane == 0u) {
        atomicOr(err, bad);
        atomicMin(err + 1, t);
    }
}

// a lane per column: the '-' of the column and whether it is kept
__global__ __launch_bounds__(256) void k_phy_gaps(const u8* __restrict__ matrix, u32 T, u32 L, u32 gmax, int* __restrict__ gaps, u32* __restrict__ flag) {
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= L) return;
    u32 g = 0;
    for (u32 t = 0; t < T; ++t) g += matrix[(size_t)t * L + c] == PHY_DASH ? 1u : 0u;
    gaps[c] = (int)g;
    flag[c] = g <= gmax ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_phy_keep(const u32* __restrict__ flag, const u32* __restrict__ pos, u32 L, int* __restrict__ keep) {
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c < L && flag[c]) keep[pos[c]] = (int)c;
}
// grid (columns of the padded row, taxa): the kept columns side by side, '-' behind them
__global__ __launch_bounds__(256) void k_phy_gather(const u8* __restrict__ matrix, u32 L, u32 Lp, const int* __restrict__ keep, const u32* __restrict__ d_nk, u8* __restrict__ K) {
    const u32 j = blockIdx.x * 256u + threadIdx.x, t = blockIdx.y;
    if (j >= Lp) return;
    K[(size_t)t * Lp + j] = j < *d_nk ? matrix[(size_t)t * L + (u32)keep[j]] : (u8)PHY_DASH;
}

// 0x80 in every byte of x that is not 0 (no carry leaves a byte: 0x7f + 0x7f < 0x100)
__device__ __forceinline__ u32 nonzero_bytes(u32 x) { return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; }

// The walk of one tile of 64 x 64 taxon pairs over the words [w_begin, w_end) of K: T rows of Lpw words (Lpw and w_begin multiples of 4),
// staged chunk by chunk in the LDS.  lane (ty, tx) of the 16 x 16 holds rows I * 64 + ty * 4 + r against rows J * 64 + tx * 4 + c; a row
// beyond T is staged as '-' and counts nothing.  The whole workgroup calls it (it synchronises); cs, ss: the lane's 4 x 4 sums, added to.
__device__ __forceinline__ void pairs_tile_walk(const u32* __restrict__ K, u32 T, u32 Lpw, u32 I, u32 J, u32 w_begin, u32 w_end, u32 (&cs)[4][4], u32 (&ss)[4][4]) {
    __shared__ __attribute__((aligned(16))) u32 sA[PHY_CHUNK_WORDS][PHY_TILE];
    __shared__ __attribute__((aligned(16))) u32 sNA[PHY_CHUNK_WORDS][PHY_TILE];
    __shared__ __attribute__((aligned(16))) u32 sB[PHY_CHUNK_WORDS][PHY_TILE];
    __shared__ __attribute__((aligned(16))) u32 sNB[PHY_CHUNK_WORDS][PHY_TILE];
    const u32 tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const u32 lrow = threadIdx.x & 63u, lpart = threadIdx.x >> 6;
    const u32 ra = I * PHY_TILE + lrow, rb = J * PHY_TILE + lrow;
    for (u32 w0 = w_begin; w0 < w_end; w0 += PHY_CHUNK_WORDS) {
        __syncthreads();   // the last chunk's readers are done
        for (u32 qd = lpart; qd < PHY_CHUNK_WORDS / 4u; qd += 4u) {
            const u32 w = w0 + qd * 4u;   // a multiple of 4 below Lpw, itself one: the 16 bytes lie inside the row
            uint4 va = make_uint4(PHY_DASH4, PHY_DASH4, PHY_DASH4, PHY_DASH4), vb = va;
            if (w < w_end) {
                if (ra < T) va = *reinterpret_cast<const uint4*>(K + (size_t)ra * Lpw + w);
                if (rb < T) vb = *reinterpret_cast<const uint4*>(K + (size_t)rb * Lpw + w);
            }
            const u32 a4[4] = {va.x, va.y, va.z, va.w}, b4[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
            for (u32 i = 0; i < 4u; ++i) {
                sA[qd * 4u + i][lrow] = a4[i], sNA[qd * 4u + i][lrow] = nonzero_bytes(a4[i] ^ PHY_DASH4);
                sB[qd * 4u + i][lrow] = b4[i], sNB[qd * 4u + i][lrow] = nonzero_bytes(b4[i] ^ PHY_DASH4);
            }
        }
        __syncthreads();
        const u32 nw = min((u32)PHY_CHUNK_WORDS, w_end - w0);
        for (u32 w = 0; w < nw; ++w) {
            const uint4 a = *reinterpret_cast<const uint4*>(&sA[w][ty * 4u]), na = *reinterpret_cast<const uint4*>(&sNA[w][ty * 4u]);
            const uint4 b = *reinterpret_cast<const uint4*>(&sB[w][tx * 4u]), nb = *reinterpret_cast<const uint4*>(&sNB[w][tx * 4u]);
            const u32 av[4] = {a.x, a.y, a.z, a.w}, nav[4] = {na.x, na.y, na.z, na.w}, bv[4] = {b.x, b.y, b.z, b.w}, nbv[4] = {nb.x, nb.y, nb.z, nb.w};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    cs[r][c] += (u32)__popc(nav[r] & nbv[c]);
                    ss[r][c] += (u32)__popc(nav[r] & ~nonzero_bytes(av[r] ^ bv[c]));   // equal bytes that are not '-' (then neither is the other)
                }
        }
    }
}

// grid (nt * nt tiles of 64 x 64 pairs, ranges of `wps` words); K: T rows of Lpw words (Lpw a multiple of 4), '-' behind the kept columns.
// blockIdx.z: the replicate of a bootstrap batch -- its rows lie krep words, its counters orep elements behind the last one's (0, 0: one matrix).
__global__ __launch_bounds__(256) void k_phy_pairs(const u32* __restrict__ K, u32 T, u32 Lpw, const u32* __restrict__ d_nk, u32 nt, u32 wps, ull* __restrict__ cmp,
                                                   ull* __restrict__ same, size_t krep, size_t orep) {
    K += (size_t)blockIdx.z * krep, cmp += (size_t)blockIdx.z * orep, same += (size_t)blockIdx.z * orep;
    const u32 I = blockIdx.x / nt, J = blockIdx.x % nt;
    if (I > J) return;
    const u32 nkw = min(Lpw, (*d_nk + 3u) >> 2);   // words that hold a kept column; the last one may be partial: its tail is '-'
    const u32 w_begin = blockIdx.y * wps, w_end = min(nkw, w_begin + wps);
    if (w_begin >= w_end) return;   // (the whole workgroup)
    const u32 tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    u32 cs[4][4], ss[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) cs[r][c] = 0u, ss[r][c] = 0u;
    pairs_tile_walk(K, T, Lpw, I, J, w_begin, w_end, cs, ss);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const u32 x = I * PHY_TILE + ty * 4u + (u32)r, y = J * PHY_TILE + tx * 4u + (u32)c;
            if (x >= T || y >= T) continue;
            if (cs[r][c]) {
                atomicAdd(cmp + (size_t)x * T + y, (ull)cs[r][c]);
                if (I != J) atomicAdd(cmp + (size_t)y * T + x, (ull)cs[r][c]);
            }
            if (ss[r][c]) {
                atomicAdd(same + (size_t)x * T + y, (ull)ss[r][c]);
                if (I != J) atomicAdd(same + (size_t)y * T + x, (ull)ss[r][c]);
            }
        }
}

// the grid of k_phy_pairs over T taxa, rows of Lpw words and `reps` matrices: tiles per side, (words per column range, ranges)
u32 pair_tiles(u32 T) { return (T + PHY_TILE - 1u) / PHY_TILE; }
std::pair<u32, u32> pair_grid(u32 nt, u32 Lpw, u32 reps) { return range_grid(Lpw, PHY_CHUNK_WORDS, (u64)(nt * (nt + 1u) / 2u) * reps, PHY_TARGET_WGS); }

// ---- bootstrap: so_phy_boot_counts, so_phy_nj_splits, so_phy_boot -------------------------------------------------------------------------
// grid (columns of the padded row, groups of PHY_BOOT_TAXA taxa, replicates): replicate b0 + z's drawn columns side by side, '-' behind them
// as k_phy_gather leaves them.  keep[] lies inside [0, L) (the host has checked), a draw inside [0, K).
__global__ __launch_bounds__(256) void k_phy_boot_gather(const u8* __restrict__ matrix, u32 T, u32 L, u32 K, u32 Kp, const int* __restrict__ keep, ull seed, u32 b0,
                                                         u8* __restrict__ out) {
    const u32 j = blockIdx.x * 256u + threadIdx.x;
    if (j >= Kp) return;
    const u32 t0 = blockIdx.y * PHY_BOOT_TAXA, t1 = min(T, t0 + PHY_BOOT_TAXA);
    u8* dst = out + (size_t)blockIdx.z * T * Kp + j;
    if (j >= K) {
        for (u32 t = t0; t < t1; ++t) dst[(size_t)t * Kp] = (u8)PHY_DASH;
        return;
    }
    const u32 c = (u32)keep[replicate_draw(seed, (ull)b0 + blockIdx.z, j, K)];
    for (u32 t = t0; t < t1; ++t) dst[(size_t)t * Kp] = matrix[(size_t)t * L + c];
}

// grid (pairs, replicates): D = 1 - same / cmp in IEEE doubles, as numpy divides; a pair without a compared column clears the replicate's ok
__global__ __launch_bounds__(256) void k_phy_boot_dist(const ull* __restrict__ cmp, const ull* __restrict__ same, u32 TT, double* __restrict__ D, u8* __restrict__ ok) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= TT) return;
    const size_t at = (size_t)blockIdx.y * TT + i;
    const ull c = cmp[at];
    if (c == 0ull) ok[blockIdx.y] = 0;   // (every writer stores the same byte)
    D[at] = 1. - (double)same[at] / (double)c;
}

__device__ __forceinline__ bool nj_before(double q, u32 a, u32 b, double q2, u32 a2, u32 b2) { return q < q2 || (q == q2 && (a < a2 || (a == a2 && b < b2))); }

// phy.py nj_splits() and nj_splits_subset(): the walk of one workgroup over one matrix, T >= 4.  D (the matrix's own T x T doubles,
// symmetric bit for bit where it is read, changed in place) stays in global memory; the row sums r, the two live lists (positions ->
// original rows, ascending; u16: T <= 4096) and -- where `scratch` is null -- the clade bit sets are LDS: r[T] | clade[T * W] | live[2][T].
// present == null: every taxon is live, n0 == T.  Else the live list starts as the n0 >= 4 set bits of present[W], ascending, and the rows
// and columns of D outside them are never read; a clade that holds the lowest live taxon is complemented inside the live set (inside the
// T bits without `present`: the same rule), and the rows n0 - 3 .. T - 4 of out are zeroed.
// Every index is a position below n <= n0 <= T or an entry of the live list, which only ever holds 0 .. T - 1 (a present bit at T or
// beyond is refused by the host); out is written at step * W + w with step < T - 3, w < W.
// Plain IEEE + - * / on doubles in the order of the definition (the build passes -ffp-contract=off: nothing is fused).
__device__ __forceinline__ void nj_walk(double* D, u32 T, u32 W, ull* out, ull* clade_scratch, const ull* __restrict__ present, u32 n0) {
    extern __shared__ __attribute__((aligned(16))) u8 nj_lds[];
    __shared__ double red_q[PHY_NJ_THREADS / 64u];
    __shared__ u32 red_a[PHY_NJ_THREADS / 64u], red_b[PHY_NJ_THREADS / 64u], pick[2];
    const u32 tid = threadIdx.x;
    double* r = reinterpret_cast<double*>(nj_lds);
    ull* clade = clade_scratch ? clade_scratch : reinterpret_cast<ull*>(r + T);
    unsigned short* live = reinterpret_cast<unsigned short*>(r + T + (clade_scratch ? 0u : T * W));
    unsigned short* next = live + T;
    for (u32 k = tid; k < T; k += PHY_NJ_THREADS) {
        if (!present) live[k] = (unsigned short)k;
        else if ((present[k >> 6] >> (k & 63u)) & 1ull) {   // its position: the present taxa below it (fewer than n0)
            u32 pos = (u32)__popcll(present[k >> 6] & ((1ull << (k & 63u)) - 1ull));
            for (u32 w = 0; w < (k >> 6); ++w) pos += (u32)__popcll(present[w]);
            live[pos] = (unsigned short)k;
        }
    }
    for (u32 x = tid; x < T * W; x += PHY_NJ_THREADS) {
        const u32 t = x / W, w = x % W;
        clade[x] = (t >> 6) == w ? 1ull << (t & 63u) : 0ull;
    }
    const ull last_mask = (T & 63u) ? (1ull << (T & 63u)) - 1ull : ~0ull;
    __syncthreads();
    u32 n = n0;
    const u32 steps = n0 - 3u;
    for (u32 step = 0; step < steps; ++step, --n) {
        // r[a]: the row of position a summed left to right over the live nodes; D[k][i] for D[i][k]: the wave reads consecutive addresses
        for (u32 a = tid; a < n; a += PHY_NJ_THREADS) {
            const u32 i = live[a];
            double s = 0.;
            for (u32 b = 0; b < n; ++b) s = s + D[(size_t)live[b] * T + i];
            r[a] = s;
        }
        __syncthreads();
        // the smallest (Q, a, b) over a < b; a lane owns the columns b, so it meets its pairs in ascending (b, a) and compares in full
        const double nm2 = (double)(n - 2u);
        double bq = INFINITY;
        u32 ba = 0u, bb = 1u;
        for (u32 b = tid; b < n; b += PHY_NJ_THREADS) {
            const u32 j = live[b];
            const double rb = r[b];
            for (u32 a = 0; a < b; ++a) {
                const double q = (nm2 * D[(size_t)live[a] * T + j] - r[a]) - rb;
                if (nj_before(q, a, b, bq, ba, bb)) bq = q, ba = a, bb = b;
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const double q2 = __shfl_xor(bq, d, 64);
            const u32 a2 = (u32)__shfl_xor((int)ba, d, 64), b2 = (u32)__shfl_xor((int)bb, d, 64);
            if (nj_before(q2, a2, b2, bq, ba, bb)) bq = q2, ba = a2, bb = b2;
        }
        if ((tid & 63u) == 0u) red_q[tid >> 6] = bq, red_a[tid >> 6] = ba, red_b[tid >> 6] = bb;
        __syncthreads();
        if (tid == 0u) {
            for (u32 v = 1; v < PHY_NJ_THREADS / 64u; ++v)
                if (nj_before(red_q[v], red_a[v], red_b[v], bq, ba, bb)) bq = red_q[v], ba = red_a[v], bb = red_b[v];
            pick[0] = ba, pick[1] = bb;
        }
        __syncthreads();
        const u32 pa = pick[0], pb = pick[1];   // pa < pb < n
        const u32 I = live[pa], J = live[pb];
        const double dij = D[(size_t)I * T + J];
        // the new node's row at position pa: a lane owns the columns k, reads rows I and J there and writes (I, k) and (k, I); nobody
        // writes row J or (I, J)
        for (u32 c = tid; c < n; c += PHY_NJ_THREADS) {
            const u32 k = live[c];
            if (k == J) continue;
            if (k == I) {
                D[(size_t)I * T + I] = 0.;
                continue;
            }
            const double v = ((D[(size_t)I * T + k] + D[(size_t)J * T + k]) - dij) / 2.;
            D[(size_t)I * T + k] = v, D[(size_t)k * T + I] = v;
        }
        // the clades: position 0 is never removed and every join keeps the lower position, so the lowest live taxon (taxon 0 when all
        // are live) sits in position 0's clade and nowhere else
        for (u32 w = tid; w < W; w += PHY_NJ_THREADS) {
            const ull c = clade[(size_t)I * W + w] | clade[(size_t)J * W + w];
            clade[(size_t)I * W + w] = c;
            out[(size_t)step * W + w] = pa == 0u ? ~c & (present ? present[w] : (w == W - 1u ? last_mask : ~0ull)) : c;
        }
        for (u32 c = tid; c + 1u < n; c += PHY_NJ_THREADS) next[c] = c < pb ? live[c] : live[c + 1u];
        __syncthreads();
        unsigned short* t = live;
        live = next, next = t;
    }
    for (u32 x = steps * W + tid; x < (T - 3u) * W; x += PHY_NJ_THREADS) out[x] = 0ull;   // (nothing without `present`: steps == T - 3)
}

// a workgroup per replicate over all T >= 4 taxa; ok (may be null): a dropped replicate has no tree, its splits are zeros
__global__ __launch_bounds__(PHY_NJ_THREADS) void k_phy_nj(double* Dall, u32 T, u32 W, const u8* __restrict__ ok, ull* __restrict__ splits, ull* scratch) {
    const u32 S = T - 3u;
    const size_t rep = blockIdx.x;
    ull* out = splits + rep * S * W;
    if (ok && !ok[rep]) {   // (the whole workgroup)
        for (u32 x = threadIdx.x; x < S * W; x += PHY_NJ_THREADS) out[x] = 0ull;
        return;
    }
    nj_walk(Dall + rep * T * T, T, W, out, scratch ? scratch + rep * T * W : nullptr, nullptr, T);
}

// a workgroup per family over its present taxa (present[fam][W], n_present[fam] of them); a dropped family and one with fewer than four
// present taxa have no split: zeros
__global__ __launch_bounds__(PHY_NJ_THREADS) void k_phy_nj_subset(double* Dall, u32 T, u32 W, const u8* __restrict__ ok, const u32* __restrict__ n_present,
                                                                  const ull* __restrict__ present, ull* __restrict__ splits, ull* scratch) {
    const u32 S = T - 3u;
    const size_t fam = blockIdx.x;
    ull* out = splits + fam * S * W;
    const u32 n0 = n_present[fam];
    if ((ok && !ok[fam]) || n0 < 4u || n0 > T) {   // (the whole workgroup; n0 <= T always: a count of bits below T)
        for (u32 x = threadIdx.x; x < S * W; x += PHY_NJ_THREADS) out[x] = 0ull;
        return;
    }
    nj_walk(Dall + fam * T * T, T, W, out, scratch ? scratch + fam * T * W : nullptr, present + fam * W, n0);
}

// grid (splits of the printed tree, replicates): does the replicate's tree hold the split?  (its T - 3 splits are distinct: one per inner edge)
__global__ __launch_bounds__(256) void k_phy_boot_support(const ull* __restrict__ ref, const ull* __restrict__ splits, u32 S, u32 W, const u8* __restrict__ ok,
                                                          u32* __restrict__ count) {
    const u32 s = blockIdx.x * 256u + threadIdx.x;
    if (s >= S || !ok[blockIdx.y]) return;
    const ull* rep = splits + (size_t)blockIdx.y * S * W;
    const ull* want = ref + (size_t)s * W;
    bool found = false;
    for (u32 x = 0; x < S && !found; ++x) {
        bool eq = true;
        for (u32 w = 0; w < W && eq; ++w) eq = rep[(size_t)x * W + w] == want[w];
        found = eq;
    }
    if (found) atomicAdd(count + s, 1u);
}

// ---- gene concordance: so_phy_gene, so_phy_gene_counts, so_phy_nj_subsets ------------------------------------------------------------------
// grid (bytes of the padded row, taxa): the kept columns family by family, each family's range padded with '-' to a multiple of 16 bytes, so
// that no family shares a 16-byte fragment with its neighbour.  src[j]: the matrix column of byte j of the row, -1 for padding (from the
// host, which has checked every column against L).
__global__ __launch_bounds__(256) void k_phy_fam_gather(const u8* __restrict__ matrix, u32 L, u32 Lp, const int* __restrict__ src, u8* __restrict__ K) {
    const u32 j = blockIdx.x * 256u + threadIdx.x, t = blockIdx.y;
    if (j >= Lp) return;
    const int c = src[j];
    K[(size_t)t * Lp + j] = c >= 0 ? matrix[(size_t)t * L + (u32)c] : (u8)PHY_DASH;
}

// grid (nt * nt tiles, 1, families of the batch): the pair counts of family f0 + z over the words [woff[z], woff[z + 1]) of the gathered
// rows (multiples of 4, rising, the last one at most Lpw: the host has made them).  One workgroup owns a (tile, family): plain 32-bit stores,
// both halves of the matrix (a family has fewer than 2^31 columns), zeros included -- no atomics, nothing to clear, an empty family too.
__global__ __launch_bounds__(256) void k_phy_fam_pairs(const u32* __restrict__ K, u32 T, u32 Lpw, const u32* __restrict__ woff, u32 nt, u32* __restrict__ cmp,
                                                       u32* __restrict__ same) {
    const u32 I = blockIdx.x / nt, J = blockIdx.x % nt;
    if (I > J) return;   // (tile (J, I) writes this one's elements)
    const size_t at = (size_t)blockIdx.z * T * T;
    const u32 tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    u32 cs[4][4], ss[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) cs[r][c] = 0u, ss[r][c] = 0u;
    pairs_tile_walk(K, T, Lpw, I, J, woff[blockIdx.z], min(Lpw, woff[blockIdx.z + 1u]), cs, ss);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const u32 x = I * PHY_TILE + ty * 4u + (u32)r, y = J * PHY_TILE + tx * 4u + (u32)c;
            if (x >= T || y >= T) continue;
            cmp[at + (size_t)x * T + y] = cs[r][c], same[at + (size_t)x * T + y] = ss[r][c];
            if (I != J) cmp[at + (size_t)y * T + x] = cs[r][c], same[at + (size_t)y * T + x] = ss[r][c];
        }
}

// grid (pairs, families): D = 1 - same / cmp in IEEE doubles, as k_phy_boot_dist divides, where both taxa are present (cmp[t][t] > 0), 0.0
// elsewhere (nothing reads it); two present taxa without a compared column clear the family's ok (every writer stores the same byte).
// The first wave of the first workgroup of a family also writes its present words and n_present.
__global__ __launch_bounds__(256) void k_phy_gene_dist(const u32* __restrict__ cmp, const u32* __restrict__ same, u32 T, u32 W, double* __restrict__ D, u8* __restrict__ ok,
                                                       ull* __restrict__ present, u32* __restrict__ n_present) {
    const u32 TT = T * T, i = blockIdx.x * 256u + threadIdx.x;
    const size_t base = (size_t)blockIdx.y * TT;
    if (blockIdx.x == 0u && threadIdx.x < 64u) {
        u32 cnt = 0;
        for (u32 w = threadIdx.x; w < W; w += 64u) {
            ull bits = 0ull;
            for (u32 t = w * 64u; t < min(T, w * 64u + 64u); ++t) bits |= cmp[base + (size_t)t * T + t] ? 1ull << (t & 63u) : 0ull;
            present[(size_t)blockIdx.y * W + w] = bits;
            cnt += (u32)__popcll(bits);
        }
        cnt = (u32)wave_sum64((ull)cnt);
        if (threadIdx.x == 0u) n_present[blockIdx.y] = cnt;
    }
    if (i >= TT) return;
    const u32 x = i / T, y = i % T, c = cmp[base + i];
    const bool both = cmp[base + (size_t)x * T + x] && cmp[base + (size_t)y * T + y];
    if (both && c == 0u) ok[blockIdx.y] = 0;
    D[base + i] = both ? 1. - (double)same[base + i] / (double)c : 0.;
}

// grid (splits of the printed tree, families): clade C of split s against the present set P of an ok family: A = C & P, B = P & ~C; decisive
// iff both hold two taxa; concordant iff the family's tree holds the one of A and B without P's lowest taxon -- the form its own splits
// have (rows n_present - 3 .. are zeros and match nothing: a side holds two taxa).  Integer atomics: the sums do not depend on the order.
__global__ __launch_bounds__(256) void k_phy_gene_concord(const ull* __restrict__ ref, const ull* __restrict__ splits, u32 S, u32 W, const u8* __restrict__ ok,
                                                          const u32* __restrict__ n_present, const ull* __restrict__ present, u32* __restrict__ decisive,
                                                          u32* __restrict__ concordant) {
    const u32 s = blockIdx.x * 256u + threadIdx.x;
    if (s >= S || !ok[blockIdx.y]) return;
    const u32 n = n_present[blockIdx.y];
    if (n < 4u) return;
    const ull* P = present + (size_t)blockIdx.y * W;
    const ull* C = ref + (size_t)s * W;
    u32 na = 0, nb = 0;
    bool seen = false, a_low = false;
    for (u32 w = 0; w < W; ++w) {
        const ull p = P[w], a = C[w] & p;
        na += (u32)__popcll(a), nb += (u32)__popcll(p & ~C[w]);
        if (!seen && p) seen = true, a_low = (a & (p & (~p + 1ull))) != 0ull;
    }
    if (na < 2u || nb < 2u) return;
    atomicAdd(decisive + s, 1u);
    const ull* fam = splits + (size_t)blockIdx.y * S * W;
    const u32 rows = min(S, n - 3u);
    bool found = false;
    for (u32 x = 0; x < rows && !found; ++x) {
        bool eq = true;
        for (u32 w = 0; w < W && eq; ++w) eq = fam[(size_t)x * W + w] == (a_low ? P[w] & ~C[w] : C[w] & P[w]);
        found = eq;
    }
    if (found) atomicAdd(concordant + s, 1u);
}

// ---- so_phy_subst: the 20 x 20 table of residue pairs per pair of taxa -------------------------------------------------------------------
// grid (columns of the padded row, groups of PHY_BOOT_TAXA taxa, tensors): the residue codes of the kept columns (draw == 0) or of replicate
// b0 + z's drawn columns side by side: the index in ARNDCQEGHILKMFPSTWYV, 0xFF for every other byte and behind the K columns up to Kp (a
// multiple of the k-step: the padding never counts).  keep[] lies inside [0, L) (the host has checked), a draw inside [0, K).
__global__ __launch_bounds__(256) void k_phy_code(const u8* __restrict__ matrix, u32 T, u32 L, u32 K, u32 Kp, const int* __restrict__ keep, ull seed, u32 b0, u32 draw,
                                                  u8* __restrict__ out) {
    __shared__ u8 lut[256];
    lut[threadIdx.x] = 0xFFu;
    __syncthreads();
    if (threadIdx.x < 20u) lut[(u8)"ARNDCQEGHILKMFPSTWYV"[threadIdx.x]] = (u8)threadIdx.x;
    __syncthreads();
    const u32 j = blockIdx.x * 256u + threadIdx.x;
    if (j >= Kp) return;
    const u32 t0 = blockIdx.y * PHY_BOOT_TAXA, t1 = min(T, t0 + PHY_BOOT_TAXA);
    u8* dst = out + (size_t)blockIdx.z * T * Kp + j;
    if (j >= K) {
        for (u32 t = t0; t < t1; ++t) dst[(size_t)t * Kp] = 0xFFu;
        return;
    }
    const u32 c = (u32)keep[draw ? replicate_draw(seed, (ull)b0 + blockIdx.z, j, K) : j];
    for (u32 t = t0; t < t1; ++t) dst[(size_t)t * Kp] = lut[matrix[(size_t)t * L + c]];
}

typedef int phs_v4 __attribute__((ext_vector_type(4)));
typedef int phs_v16 __attribute__((ext_vector_type(16)));

// 0x01 in every byte of w that equals the splat's byte: four entries of a row of E
__device__ __forceinline__ u32 onehot4(u32 w, u32 splat) { return (~nonzero_bytes(w ^ splat) & 0x80808080u) >> 7; }
// the 16 operand bytes of a lane: row 20 i + a of E over 16 columns is (code[i][k] == a); p: the 16 codes of taxon i in the LDS
__device__ __forceinline__ phs_v4 subst_frag(const u8* p, u32 splat) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    phs_v4 f;
    f.x = (int)onehot4(v.x, splat), f.y = (int)onehot4(v.y, splat), f.z = (int)onehot4(v.z, splat), f.w = (int)onehot4(v.w, splat);
    return f;
}

// grid (nt * nt tiles of PHS_TILE x PHS_TILE of N = E E^T, ranges of `cps` columns, tensors); code: T rows of Kp bytes (Kp a multiple of 32,
// cps a multiple of PHS_CHUNK_COLS), 0xFF behind the K columns.  Only tiles I <= J hold a pair i < j.  Wave (wr, wc) of the 2 x 2 owns rows
// I * 128 + wr * 64 .. + 63 against columns J * 128 + wc * 64 .. + 63 as 2 x 2 MFMA tiles.  v_mfma_i32_32x32x32_i8: lane l holds row (A) or
// column (B) l & 31 over the 16 columns 16 (l >> 5) .. + 15 of the k-step -- A and B are built by the same function from the same bytes, so
// the k order inside a lane does not matter --; accumulator register g of lane l is row (g & 3) + 8 (g >> 2) + 4 (l >> 5), column l & 31.
// A row of E beyond 20 T reads a staged row of 0xFF and stays 0; the flush keeps i < j < T only.  out: [pair][20][20], zeroed by the host;
// blockIdx.z: its code rows lie crep bytes, its tensor orep elements behind the last one's.
__global__ __launch_bounds__(256) void k_phy_subst(const u8* __restrict__ code, u32 T, u32 Kp, u32 nt, u32 cps, int* __restrict__ out, size_t crep, size_t orep) {
    code += (size_t)blockIdx.z * crep, out += (size_t)blockIdx.z * orep;
    __shared__ __attribute__((aligned(16))) u8 sA[PHS_TAXA * PHS_CHUNK_COLS];
    __shared__ __attribute__((aligned(16))) u8 sB[PHS_TAXA * PHS_CHUNK_COLS];
    const u32 I = blockIdx.x / nt, J = blockIdx.x % nt;
    if (I > J) return;
    const u32 c_begin = blockIdx.y * cps, c_end = min(Kp, c_begin + cps);   // multiples of 32
    if (c_begin >= c_end) return;   // (the whole workgroup)
    const u32 tA0 = I * PHS_TILE / 20u, tB0 = J * PHS_TILE / 20u;
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, wr = wave >> 1, wc = wave & 1u, r = lane & 31u, h = lane >> 5;
    const bool live = I != J || wr <= wc;   // (wave-uniform) below the diagonal of a diagonal tile no pair has i < j
    u32 aoff[2], asplat[2], boff[2], bsplat[2];
#pragma unroll
    for (u32 m = 0; m < 2u; ++m) {
        const u32 ra = I * PHS_TILE + wr * 64u + m * 32u + r, rb = J * PHS_TILE + wc * 64u + m * 32u + r;   // ra / 20 - tA0 < PHS_TAXA
        aoff[m] = (ra / 20u - tA0) * PHS_CHUNK_COLS + 16u * h, asplat[m] = (ra % 20u) * 0x01010101u;
        boff[m] = (rb / 20u - tB0) * PHS_CHUNK_COLS + 16u * h, bsplat[m] = (rb % 20u) * 0x01010101u;
    }
    phs_v16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[m][n][g] = 0;
    static_assert(PHS_TAXA * (PHS_CHUNK_COLS / 16u) == 256u, "a lane stages 16 bytes of each side per chunk");
    const u32 st = threadIdx.x / (PHS_CHUNK_COLS / 16u), sp = (threadIdx.x % (PHS_CHUNK_COLS / 16u)) * 16u;
    for (u32 c0 = c_begin; c0 < c_end; c0 += PHS_CHUNK_COLS) {
        __syncthreads();   // the last chunk's readers are done
        uint4 va = make_uint4(~0u, ~0u, ~0u, ~0u), vb = va;
        if (c0 + sp < c_end) {   // c0 + sp a multiple of 16 below c_end <= Kp, itself a multiple of 32: the 16 bytes lie inside the row
            if (tA0 + st < T) va = *reinterpret_cast<const uint4*>(code + (size_t)(tA0 + st) * Kp + c0 + sp);
            if (tB0 + st < T) vb = *reinterpret_cast<const uint4*>(code + (size_t)(tB0 + st) * Kp + c0 + sp);
        }
        *reinterpret_cast<uint4*>(sA + st * PHS_CHUNK_COLS + sp) = va;
        *reinterpret_cast<uint4*>(sB + st * PHS_CHUNK_COLS + sp) = vb;
        __syncthreads();
        if (!live) continue;
        const u32 steps = min((u32)PHS_CHUNK_COLS, c_end - c0) / 32u;
        for (u32 kk = 0; kk < steps; ++kk) {
            const phs_v4 a0 = subst_frag(sA + aoff[0] + kk * 32u, asplat[0]), a1 = subst_frag(sA + aoff[1] + kk * 32u, asplat[1]);
            const phs_v4 b0 = subst_frag(sB + boff[0] + kk * 32u, bsplat[0]), b1 = subst_frag(sB + boff[1] + kk * 32u, bsplat[1]);
            acc[0][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    if (!live) return;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const u32 col = J * PHS_TILE + wc * 64u + (u32)n * 32u + r, j = col / 20u, b = col % 20u;
            if (j >= T) continue;
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const u32 row = I * PHS_TILE + wr * 64u + (u32)m * 32u + (u32)(g & 3) + 8u * (u32)(g >> 2) + 4u * h, i = row / 20u, a = row % 20u;
                const int v = acc[m][n][g];
                if (v == 0 || i >= j) continue;   // i < j < T: the pair's number lies below T (T - 1) / 2
                const size_t p = (size_t)(i * (2u * T - i - 1u) / 2u + (j - i - 1u));
                atomicAdd(out + p * 400u + a * 20u + b, v);
            }
        }
}

thread_local std::string g_phy_err;

auto slots(so_phy_subst_result* r) { return result_slots(&r->subst); }
auto slots(so_phy_result* r) { return result_slots(&r->row, &r->matrix, &r->gaps, &r->keep, &r->cmp, &r->same); }
auto slots(so_phy_boot_result* r) { return result_slots(&r->cmp, &r->same, &r->splits, &r->count, &r->ok); }
auto slots(so_phy_gene_result* r) { return result_slots(&r->cmp, &r->same, &r->splits, &r->present, &r->decisive, &r->concordant, &r->n_present, &r->ok); }

// What every call over a matrix and its kept columns checks before anything touches the device -> keep as the 32-bit columns the kernels
// read (want32; the calls over families lay their columns out themselves, gene_layout, and take none).  some_keep: a call that draws needs a kept column.  rest(): the caller's own checks (its replicates or families, the NULL
// pointers), made before keep[] is walked.
template <class Rest>
std::vector<int> matrix_check(const std::string& who, i64 n_taxa, i64 n_cols, i64 n_keep, const i64* keep, bool some_keep, bool want32, Rest rest) {
    if (n_taxa < 2 || n_taxa > PHY_MAX_TAXA) throw SoError(who + ": the taxa number 2 .. " + std::to_string(PHY_MAX_TAXA) + " (n_taxa is " + std::to_string(n_taxa) + ")");
    if (n_cols < 0 || n_cols > 0x7FFFFFFFll) throw SoError(who + ": more than 2^31 - 1 columns are not supported");
    if (some_keep && n_keep <= 0) throw SoError(who + ": no kept column to draw from (n_keep is 0)");
    if (n_keep < 0 || n_keep > 0x7FFFFFFFll - 16) throw SoError(who + ": more than 2^31 - 17 kept columns are not supported");
    rest();
    std::vector<int> k32(want32 ? (size_t)n_keep : 0);
    for (i64 k = 0; k < n_keep; ++k) {
        if (keep[k] < 0 || keep[k] >= n_cols) throw SoError(who + ": keep[" + std::to_string(k) + "] lies outside 0 .. n_cols - 1");
        if (want32) k32[(size_t)k] = (int)keep[k];
    }
    return k32;
}
// ... of the calls that draw columns
std::vector<int> boot_check(const std::string& who, i64 n_taxa, i64 n_cols, const u8* matrix, i64 n_keep, const i64* keep, i64 b0, i64 n_reps) {
    return matrix_check(who, n_taxa, n_cols, n_keep, keep, true, true, [&] {
        if (n_reps < 1) throw SoError(who + ": a replicate at least (n_reps is " + std::to_string(n_reps) + ")");
        if (b0 < 0 || b0 >= (1ll << 31) || n_reps >= (1ll << 31) || b0 + n_reps > (1ll << 31))
            throw SoError(who + ": replicates beyond 2^31 - 1 are not supported");
        if (!matrix || !keep) throw SoError(who + ": matrix or keep is NULL");
    });
}

// one batch: the drawn columns of nb replicates from b0 on side by side, then their pair counts (cmp, same: nb * T * T, zeroed here)
void boot_counts_batch(hipStream_t st, const u8* matrix, u32 T, u32 L, u32 K, const int* keep, const u32* d_K, ull seed, u32 b0, u32 nb, u8* cols, ull* cmp, ull* same) {
    const u32 Kp = (K + 15u) & ~15u, Kpw = Kp / 4u, nt = pair_tiles(T);
    const size_t TT = (size_t)T * T;
    HIP_CHECK(hipMemsetAsync(cmp, 0, (size_t)nb * TT * sizeof(ull), st));
    HIP_CHECK(hipMemsetAsync(same, 0, (size_t)nb * TT * sizeof(ull), st));
    hipLaunchKernelGGL(k_phy_boot_gather, dim3((Kp + 255u) / 256u, (T + PHY_BOOT_TAXA - 1u) / PHY_BOOT_TAXA, nb), dim3(256), 0, st, matrix, T, L, K, Kp, keep, seed, b0, cols);
    const auto [wps, ranges] = pair_grid(nt, Kpw, nb);
    hipLaunchKernelGGL(k_phy_pairs, dim3(nt * nt, ranges, nb), dim3(256), 0, st, reinterpret_cast<const u32*>(cols), T, Kpw, d_K, nt, wps, cmp, same, (size_t)T * Kpw, TT);
}

// the walk of nb matrices, over all taxa (present null: k_phy_nj) or over each one's present taxa (k_phy_nj_subset); clades: the scratch of
// the bit sets (nb * T * W words) or null where they fit the LDS
static_assert(sizeof(so_phy_boot_result) == 120, "nj_tier and its pad word follow the pointers: swiftortho_amd/_lib.py SoPhyBootResult mirrors the layout");
size_t nj_lds_bytes(u32 T, u32 W, bool in_lds) { return (size_t)T * 8u + (in_lds ? (size_t)T * W * 8u : 0u) + (size_t)T * 4u; }
bool nj_clades_fit(u32 T, u32 W) { return nj_lds_bytes(T, W, true) <= PHY_NJ_LDS_BYTES; }
void nj_launch(hipStream_t st, double* D, u32 T, u32 W, u32 nb, const u8* ok, const u32* n_present, const ull* present, ull* splits, ull* clades) {
    const size_t lds = nj_lds_bytes(T, W, clades == nullptr);
    if (present) hipLaunchKernelGGL(k_phy_nj_subset, dim3(nb), dim3(PHY_NJ_THREADS), lds, st, D, T, W, ok, n_present, present, splits, clades);
    else hipLaunchKernelGGL(k_phy_nj, dim3(nb), dim3(PHY_NJ_THREADS), lds, st, D, T, W, ok, splits, clades);
}

// ---- gene concordance ----
static_assert(sizeof(so_phy_gene_result) == 136, "swiftortho_amd/_lib.py SoPhyGeneResult mirrors the layout");
// what the calls over families check before anything touches the device
void gene_check(const std::string& who, i64 n_taxa, i64 n_cols, const u8* matrix, i64 n_keep, const i64* keep, i64 n_fam, const i64* fam_off) {
    matrix_check(who, n_taxa, n_cols, n_keep, keep, false, false, [&] {
        if (n_fam < 1 || n_fam >= (1ll << 31)) throw SoError(who + ": the families number 1 .. 2^31 - 1 (n_fam is " + std::to_string(n_fam) + ")");
        if (!fam_off || (n_keep > 0 && !keep) || ((i64)n_taxa * n_cols > 0 && !matrix)) throw SoError(who + ": matrix, keep or fam_off is NULL");
        if (fam_off[0] != 0) throw SoError(who + ": inconsistent offsets: fam_off does not start at 0");
        for (i64 f = 0; f < n_fam; ++f)
            if (fam_off[f + 1] < fam_off[f]) throw SoError(who + ": inconsistent offsets: fam_off falls at family " + std::to_string(f));
        if (fam_off[n_fam] != n_keep) throw SoError(who + ": inconsistent offsets: fam_off does not end at n_keep");
    });
}
// the gathered row of the families f0 .. f0 + nf - 1: src[j] = the matrix column of byte j, -1 where a family's range is padded to a
// multiple of 16 bytes; woff[z] = the first 32-bit word of family f0 + z (nf + 1 of them, multiples of 4)
void gene_layout(const std::string& who, const i64* keep, const i64* fam_off, i64 f0, i64 nf, std::vector<int>& src, std::vector<u32>& woff) {
    u64 bytes = 0;
    for (i64 f = f0; f < f0 + nf; ++f) bytes += ((u64)(fam_off[f + 1] - fam_off[f]) + 15u) & ~15ull;
    if (bytes > 0x7FFFFFF0ull) throw SoError(who + ": the families' padded columns take more than 2^31 - 16 bytes a row: ask for fewer families per call");
    src.assign((size_t)bytes, -1), woff.assign((size_t)nf + 1, 0u);
    size_t at = 0;
    for (i64 z = 0; z < nf; ++z) {
        const i64 k0 = fam_off[f0 + z], k1 = fam_off[f0 + z + 1];
        for (i64 k = k0; k < k1; ++k) src[at + (size_t)(k - k0)] = (int)keep[k];
        at += ((size_t)(k1 - k0) + 15u) & ~(size_t)15u;
        woff[(size_t)z + 1] = (u32)(at / 4u);
    }
}
// the gathered rows of such a layout (T rows of src.size() bytes) in K
void gene_gather(hipStream_t st, const u8* matrix, u32 T, u32 L, const std::vector<int>& src, DevBuf<int>& d_src, DevBuf<u8>& K) {
    const u32 Lp = (u32)src.size();
    upload(d_src, src.data(), src.size(), st);
    K.ensure((size_t)T * Lp + 16);
    if (Lp) hipLaunchKernelGGL(k_phy_fam_gather, dim3((Lp + 255u) / 256u, T), dim3(256), 0, st, matrix, L, Lp, d_src.p, K.p);
}

// so_phy_nj_splits (R so_phy_boot_result, present null) and so_phy_nj_subsets (R so_phy_gene_result, a row of present words per matrix):
// the walk of n_reps matrices, PHY_BOOT_MAX_BATCH to a launch, one host wait each.  Where the walk reads D -- between two present taxa,
// everywhere without `present` -- it is finite and symmetric bit for bit, or the call is refused.
template <class R>
int nj_call(const std::string& who, int device, i64 n_reps, i64 n_taxa, const double* D, const uint64_t* present, int32_t flags, R* out, void (*free_result)(R*)) {
    constexpr bool subset = std::is_same<R, so_phy_gene_result>::value;
    const std::string among = subset ? " between two present taxa" : "";
    return guarded_call(g_phy_err, out, free_result, [&] {
        if (!out) throw SoError(who + ": result pointer is NULL");
        memset(out, 0, sizeof *out);
        if (flags & ~1) throw SoError(who + ": unknown flag bits (bit 0: the clade bit sets in global scratch)");
        if (n_taxa < 2 || n_taxa > PHY_MAX_TAXA) throw SoError(who + ": the taxa number 2 .. " + std::to_string(PHY_MAX_TAXA) + " (n_taxa is " + std::to_string(n_taxa) + ")");
        if (n_reps < 1 || n_reps >= (1ll << 31)) throw SoError(who + ": the matrices number 1 .. 2^31 - 1 (n_reps is " + std::to_string(n_reps) + ")");
        if (!D || (subset && !present)) throw SoError(who + (subset ? ": D or present is NULL" : ": D is NULL"));
        const u32 T = (u32)n_taxa, W = (T + 63u) / 64u, S = T > 3u ? T - 3u : 0u;
        const size_t TT = (size_t)T * T;
        const u64 last_mask = (T & 63u) ? (1ull << (T & 63u)) - 1ull : ~0ull;
        std::vector<u32> npres(present ? (size_t)n_reps : 0), rows(T);   // rows: the taxa the walk reads -- all of them, or a matrix's present ones
        for (u32 t = 0; t < T; ++t) rows[t] = t;
        for (i64 b = 0; b < n_reps; ++b) {
            const double* M = D + (size_t)b * TT;
            if (present) {
                const uint64_t* P = present + (size_t)b * W;
                if (P[W - 1u] & ~last_mask) throw SoError(who + ": the present words of matrix " + std::to_string(b) + " name a taxon beyond n_taxa - 1");
                rows.clear();
                for (u32 t = 0; t < T; ++t)
                    if ((P[t >> 6] >> (t & 63u)) & 1ull) rows.push_back(t);
                npres[(size_t)b] = (u32)rows.size();
            }
            for (u32 i : rows)
                for (u32 j : rows) {
                    if (!std::isfinite(M[(size_t)i * T + j])) throw SoError(who + ": matrix " + std::to_string(b) + " holds a value that is not finite" + among);
                    if (j < i && memcmp(&M[(size_t)i * T + j], &M[(size_t)j * T + i], sizeof(double)) != 0)
                        throw SoError(who + ": matrix " + std::to_string(b) + " is not symmetric bit for bit" + among);
                }
        }
        out->n_taxa = n_taxa, out->n_splits = S, out->n_words = W;
        if constexpr (subset) out->n_fam = n_reps;
        else out->n_reps = n_reps;
        check_device(who.c_str(), device);
        if (S == 0) {   // two or three taxa: one topology, no split
            fill_empty_slots(slots(out));
            return;
        }
        const bool in_lds = !(flags & 1) && nj_clades_fit(T, W);
        out->nj_tier = in_lds ? 1 : 2;
        DeviceCall call(device);
        hipStream_t st = call.st;
        DevBuf<double> d_D;
        DevBuf<ull> d_splits, clades, d_present;
        DevBuf<u32> d_np;
        const size_t per_call = PHY_BOOT_MAX_BATCH;
        out->splits = host_array<uint64_t>(who.c_str(), (size_t)n_reps * S * W);
        static_assert(sizeof(ull) == sizeof(uint64_t), "the bit sets are copied out as uint64");
        for (size_t b0 = 0; b0 < (size_t)n_reps; b0 += per_call) {
            const u32 nb = (u32)std::min(per_call, (size_t)n_reps - b0);
            upload(d_D, D + b0 * TT, (size_t)nb * TT, st);
            if (present) upload(d_present, reinterpret_cast<const ull*>(present) + b0 * W, (size_t)nb * W, st), upload(d_np, npres.data() + b0, nb, st);
            d_splits.ensure((size_t)nb * S * W + 2);
            if (!in_lds) clades.ensure((size_t)nb * T * W + 2);
            nj_launch(st, d_D.p, T, W, nb, nullptr, d_np.p, present ? d_present.p : nullptr, d_splits.p, in_lds ? nullptr : clades.p);
            HIP_CHECK(hipGetLastError());
            call.fetch(reinterpret_cast<ull*>(out->splits) + b0 * S * W, d_splits.p, (size_t)nb * S * W);
            call.wait();
            ++out->batches;
        }
        out->waits = call.waits;
        fill_empty_slots(slots(out));
    });
}

}  // namespace

extern "C" {

const char* so_phy_last_error(void) { return g_phy_err.c_str(); }

void so_phy_free(so_phy_result* r) {
    if (r) release_slots(r, slots(r));
}

int so_phy_rows(int device, int64_t n, const int32_t* q, const int32_t* s, const double* score, int64_t n_pairs, const int32_t* pair_q, const int32_t* pair_s, int32_t flags,
                so_phy_result* out) {
    const std::string who = "so_phy_rows";
    return guarded_call(g_phy_err, out, so_phy_free, [&] {
        if (!out) throw SoError(who + ": result pointer is NULL");
        memset(out, 0, sizeof *out);
        if (flags != 0) throw SoError(who + ": flags is reserved and must be 0");
        if (n < 0 || n_pairs < 0) throw SoError(who + ": bad arguments");
        if (n >= (1ll << 31)) throw SoError(who + ": 2^31 rows and more are not supported (32-bit row numbers)");
        if (n_pairs >= (1ll << 31)) throw SoError(who + ": 2^31 wanted pairs and more are not supported");
        if (n > 0 && (!q || !s || !score)) throw SoError(who + ": a hit column is NULL");
        if (n_pairs > 0 && (!pair_q || !pair_s)) throw SoError(who + ": a pair column is NULL");
        for (i64 i = 0; i < n; ++i)
            if (score[i] != score[i]) throw SoError(who + ": row " + std::to_string(i) + " has a NaN score");
        std::vector<u64> key((size_t)n_pairs);
        for (i64 p = 0; p < n_pairs; ++p) {
            if (pair_q[p] < 0 || pair_s[p] < 0) throw SoError(who + ": wanted pair " + std::to_string(p) + " holds a negative name code");
            key[(size_t)p] = ((u64)(u32)pair_q[p] << 32) | (u64)(u32)pair_s[p];
        }
        out->n_pairs = n_pairs;
        check_device(who.c_str(), device);
        out->row = host_array<int64_t>(who.c_str(), (size_t)n_pairs);
        for (i64 p = 0; p < n_pairs; ++p) out->row[p] = -1;
        if (n == 0 || n_pairs == 0) {   // nothing to launch
            fill_empty_slots(slots(out));
            return;
        }
        DeviceCall call(device);
        hipStream_t st = call.st;
        const u32 N = (u32)n, P = (u32)n_pairs;
        DevBuf<int> d_q, d_s;
        DevBuf<ull> d_score, d_pkey, d_skey, best;
        DevBuf<u32> slot_of, first, d_row;
        DevBuf<u8> sort_tmp;
        static_assert(sizeof(ull) == sizeof(double) && sizeof(ull) == sizeof(u64), "scores travel as their bits");
        upload(d_q, q, (size_t)n, st), upload(d_s, s, (size_t)n, st), upload(d_score, reinterpret_cast<const ull*>(score), (size_t)n, st);
        upload(d_pkey, reinterpret_cast<const ull*>(key.data()), key.size(), st);
        d_skey.ensure((size_t)P + 2), best.ensure((size_t)P + 2), first.ensure((size_t)P + 2), d_row.ensure((size_t)P + 2), slot_of.ensure((size_t)N + 2);
        const size_t tb = sort_keys_u64_temp_bytes(P, 64);
        sort_tmp.ensure(tb + 16);
        sort_keys_u64(sort_tmp.p, tb, reinterpret_cast<const u64*>(d_pkey.p), reinterpret_cast<u64*>(d_skey.p), P, 0, 64, st);
        HIP_CHECK(hipMemsetAsync(best.p, 0, (size_t)P * sizeof(ull), st));          // below every score's number
        HIP_CHECK(hipMemsetAsync(first.p, 0xFF, (size_t)P * sizeof(u32), st));      // NONE32: no row
        hipLaunchKernelGGL(k_phy_row_max, grid256(N), dim3(256), 0, st, N, d_q.p, d_s.p, d_score.p, d_skey.p, P, slot_of.p, best.p);
        hipLaunchKernelGGL(k_phy_row_first, grid256(N), dim3(256), 0, st, N, d_score.p, slot_of.p, best.p, first.p);
        hipLaunchKernelGGL(k_phy_row_out, grid256(P), dim3(256), 0, st, P, d_pkey.p, d_skey.p, first.p, d_row.p);
        HIP_CHECK(hipGetLastError());
        std::vector<u32> row((size_t)P);
        call.fetch(row.data(), d_row.p, (size_t)P);
        call.wait();
        out->waits = call.waits;
        for (size_t p = 0; p < (size_t)P; ++p) out->row[p] = row[p] == NONE32 ? -1 : (int64_t)row[p];
        fill_empty_slots(slots(out));
    });
}

int so_phy_build(int device, int64_t n_taxa, int64_t n_fam, const int64_t* col_off, int64_t n_tasks, const int32_t* fam, const int32_t* slot, const uint8_t* kind,
                 const int64_t* res_off, const int32_t* res_len, const int32_t* qst, const int32_t* sst, const int64_t* run_off, const uint32_t* runs, int64_t n_runs,
                 const uint8_t* residues, int64_t n_res, double gap_share, int32_t flags, so_phy_result* out) {
    const std::string who = "so_phy_build";
    return guarded_call(g_phy_err, out, so_phy_free, [&] {
        if (!out) throw SoError(who + ": result pointer is NULL");
        memset(out, 0, sizeof *out);
        if (flags & ~1) throw SoError(who + ": unknown flag bits (bit 0: no matrix in the result)");
        if (n_taxa < 0 || n_fam < 0 || n_tasks < 0 || n_runs < 0 || n_res < 0) throw SoError(who + ": bad arguments");
        if (n_taxa == 0) throw SoError(who + ": no taxa (n_taxa is 0)");
        if (n_fam == 0) throw SoError(who + ": no families (n_fam is 0)");
        if (!(gap_share >= 0. && gap_share <= 1.)) throw SoError(who + ": the gap share must lie in [0, 1]");
        if (n_taxa >= 46341) throw SoError(who + ": 46341 taxa and more (2^31 pairs) are not supported");
        if (n_fam >= (1ll << 31) || n_tasks >= (1ll << 31)) throw SoError(who + ": 2^31 families or tasks and more are not supported");
        if (!col_off) throw SoError(who + ": col_off is NULL");
        if (n_tasks > 0 && (!fam || !slot || !kind || !res_off || !res_len || !qst || !sst || !run_off)) throw SoError(who + ": a task column is NULL");
        if ((n_runs > 0 && !runs) || (n_res > 0 && !residues)) throw SoError(who + ": runs or residues is NULL");
        if (col_off[0] != 0) throw SoError(who + ": inconsistent offsets: col_off does not start at 0");
        for (i64 f = 0; f < n_fam; ++f) {
            if (col_off[f + 1] < col_off[f]) throw SoError(who + ": inconsistent offsets: col_off falls at family " + std::to_string(f));
            if (col_off[f + 1] > 0x7FFFFFFFll) throw SoError(who + ": more than 2^31 - 1 columns are not supported");
        }
        const i64 L64 = col_off[n_fam];
        if (n_tasks > 0 && run_off[0] != 0) throw SoError(who + ": inconsistent offsets: run_off does not start at 0");
        {
            std::vector<u64> cell((size_t)n_tasks);
            for (i64 t = 0; t < n_tasks; ++t) {
                const std::string task = "task " + std::to_string(t);
                if (fam[t] < 0 || fam[t] >= n_fam) throw SoError(who + ": " + task + " names a family outside 0 .. n_fam - 1");
                if (slot[t] < 0 || slot[t] >= n_taxa) throw SoError(who + ": " + task + " names a slot outside 0 .. n_taxa - 1");
                if (res_len[t] < 0 || res_off[t] < 0 || res_off[t] > n_res || (i64)res_len[t] > n_res - res_off[t])
                    throw SoError(who + ": inconsistent offsets: the residues of " + task + " lie outside the residue blob");
                if (run_off[t + 1] < run_off[t] || run_off[t + 1] > n_runs) throw SoError(who + ": inconsistent offsets: the runs of " + task + " lie outside the run array");
                cell[(size_t)t] = (u64)fam[t] * (u64)n_taxa + (u64)slot[t];
            }
            if (n_tasks > 0 && run_off[n_tasks] != n_runs) throw SoError(who + ": inconsistent offsets: run_off does not end at n_runs");
            std::sort(cell.begin(), cell.end());
            const auto dup = std::adjacent_find(cell.begin(), cell.end());
            if (dup != cell.end())
                throw SoError(who + ": two tasks fill family " + std::to_string(*dup / (u64)n_taxa) + ", slot " + std::to_string(*dup % (u64)n_taxa));
        }
        const bool want_matrix = !(flags & 1);
        const u32 T = (u32)n_taxa, L = (u32)L64, NT = (u32)n_tasks;
        const size_t cells = (size_t)T * L, TT = (size_t)T * T;
        out->n_taxa = n_taxa, out->n_cols = L64;
        check_device(who.c_str(), device);
        const char* w = who.c_str();
        if (L == 0) {   // families without a column: nothing to launch (a task then has an anchor of length 0: only empty tasks pass)
            for (i64 t = 0; t < n_tasks; ++t)
                if (kind[t] ? res_len[t] != 0 : (run_off[t + 1] != run_off[t] || qst[t] != 1 || sst[t] < 1 || sst[t] - 1 > res_len[t]))
                    throw SoError(who + ": task " + std::to_string(t) + " (family " + std::to_string(fam[t]) + ", slot " + std::to_string(slot[t]) + ") runs past its anchor");
            out->cmp = host_array<int64_t>(w, TT), out->same = host_array<int64_t>(w, TT);
            memset(out->cmp, 0, TT * 8), memset(out->same, 0, TT * 8);
            fill_empty_slots(slots(out));
            return;
        }
        const u32 gmax = (u32)std::floor(gap_share * (double)T);   // (as Python evaluates floor(g * T): one IEEE product)
        DeviceCall call(device);
        hipStream_t st = call.st;
        DevBuf<int> d_fam, d_slot, d_rlen, d_qst, d_sst, d_gaps, d_keep;
        DevBuf<u8> d_kind, d_res, matrix, kept;
        DevBuf<i64> d_roff, d_runoff, d_coloff;
        DevBuf<u32> d_runs, err, flag, pos, scan_tmp;
        DevBuf<ull> d_cmp, d_same;
        upload(d_coloff, col_off, (size_t)n_fam + 1, st);
        if (NT) {
            upload(d_fam, fam, NT, st), upload(d_slot, slot, NT, st), upload(d_kind, kind, NT, st), upload(d_roff, res_off, NT, st), upload(d_rlen, res_len, NT, st);
            upload(d_qst, qst, NT, st), upload(d_sst, sst, NT, st), upload(d_runoff, run_off, (size_t)NT + 1, st);
        }
        upload(d_runs, runs, (size_t)n_runs, st), upload(d_res, residues, (size_t)n_res, st);
        const u32 Lp = (L + 15u) & ~15u, Lpw = Lp / 4u;   // (L <= 2^31 - 1: Lp <= 2^31)
        matrix.ensure(cells + 16), kept.ensure((size_t)T * Lp + 16), d_gaps.ensure((size_t)L + 2), d_keep.ensure((size_t)L + 2), flag.ensure((size_t)L + 2), pos.ensure((size_t)L + 2);
        scan_tmp.ensure(scan_u32_temp_elems(L) + 2), err.ensure(4), d_cmp.ensure(TT + 2), d_same.ensure(TT + 2);
        HIP_CHECK(hipMemsetAsync(matrix.p, (int)PHY_DASH, cells, st));
        HIP_CHECK(hipMemsetAsync(err.p, 0, sizeof(u32), st));
        HIP_CHECK(hipMemsetAsync(err.p + 1, 0xFF, sizeof(u32), st));
        HIP_CHECK(hipMemsetAsync(d_cmp.p, 0, TT * sizeof(ull), st));
        HIP_CHECK(hipMemsetAsync(d_same.p, 0, TT * sizeof(ull), st));
        if (NT) {
            const PhyTasks tk = {d_fam.p, d_slot.p, d_rlen.p, d_qst.p, d_sst.p, d_kind.p, d_roff.p, d_runoff.p};
            hipLaunchKernelGGL(k_phy_project, dim3((NT + 3u) / 4u), dim3(256), 0, st, NT, tk, d_runs.p, d_res.p, d_coloff.p, (u64)L, matrix.p, err.p);
        }
        hipLaunchKernelGGL(k_phy_gaps, grid256(L), dim3(256), 0, st, matrix.p, T, L, gmax, d_gaps.p, flag.p);
        const u32* d_nk = scan_u32(flag.p, pos.p, L, false, scan_tmp.p, st);
        hipLaunchKernelGGL(k_phy_keep, grid256(L), dim3(256), 0, st, flag.p, pos.p, L, d_keep.p);
        hipLaunchKernelGGL(k_phy_gather, dim3((Lp + 255u) / 256u, T), dim3(256), 0, st, matrix.p, L, Lp, d_keep.p, d_nk, kept.p);
        {
            const u32 nt = pair_tiles(T);
            const auto [wps, ranges] = pair_grid(nt, Lpw, 1u);
            hipLaunchKernelGGL(k_phy_pairs, dim3(nt * nt, ranges), dim3(256), 0, st, reinterpret_cast<const u32*>(kept.p), T, Lpw, d_nk, nt, wps, d_cmp.p, d_same.p, (size_t)0,
                               (size_t)0);
        }
        HIP_CHECK(hipGetLastError());
        u32 e[2] = {0, 0}, nk = 0;
        call.fetch(e, err.p, 2), call.fetch(&nk, d_nk);
        if (want_matrix) out->matrix = host_copy(w, matrix.p, cells, st);
        out->gaps = host_copy(w, d_gaps.p, (size_t)L, st);
        out->keep = host_copy(w, d_keep.p, (size_t)L, st);   // (the first n_keep entries are written)
        static_assert(sizeof(ull) == sizeof(int64_t), "the counters are copied out as int64");
        out->cmp = (int64_t*)host_copy(w, d_cmp.p, TT, st);
        out->same = (int64_t*)host_copy(w, d_same.p, TT, st);
        call.wait();
        out->waits = call.waits;
        if (e[0]) {
            const u32 t = e[1];
            const std::string task = "task " + std::to_string(t) + " (family " + std::to_string(fam[t]) + ", slot " + std::to_string(slot[t]) + ")";
            if (kind[t]) throw SoError(who + ": " + task + " is the anchor, and its residues are not as many as the family's columns");
            if (qst[t] < 1 || sst[t] < 1) throw SoError(who + ": " + task + " starts before the first residue (qst or sst < 1)");
            throw SoError(who + ": " + task + " has a run of length 0 or of an unknown operation, or its runs lead past the anchor or past the member");
        }
        out->n_keep = nk;
        fill_empty_slots(slots(out));
    });
}

void so_phy_boot_free(so_phy_boot_result* r) {
    if (r) release_slots(r, slots(r));
}

int so_phy_boot_counts(int device, int64_t n_taxa, int64_t n_cols, const uint8_t* matrix, int64_t n_keep, const int64_t* keep, uint64_t seed, int64_t b0, int64_t n_reps,
                       int32_t flags, so_phy_boot_result* out) {
    const std::string who = "so_phy_boot_counts";
    return guarded_call(g_phy_err, out, so_phy_boot_free, [&] {
        if (!out) throw SoError(who + ": result pointer is NULL");
        memset(out, 0, sizeof *out);
        if (flags != 0) throw SoError(who + ": flags is reserved and must be 0");
        const std::vector<int> k32 = boot_check(who, n_taxa, n_cols, matrix, n_keep, keep, b0, n_reps);
        if (n_reps > PHY_BOOT_MAX_BATCH) throw SoError(who + ": more than " + std::to_string(PHY_BOOT_MAX_BATCH) + " replicates in one call are not supported");
        const u32 T = (u32)n_taxa, L = (u32)n_cols, K = (u32)n_keep, nb = (u32)n_reps, Kp = (K + 15u) & ~15u;
        const size_t TT = (size_t)T * T;
        out->n_taxa = n_taxa, out->n_reps = n_reps;
        check_device(who.c_str(), device);
        DeviceCall call(device);
        hipStream_t st = call.st;
        DevBuf<u8> d_matrix, cols;
        DevBuf<int> d_keep;
        DevBuf<u32> d_K;
        DevBuf<ull> d_cmp, d_same;
        upload(d_matrix, matrix, (size_t)T * L, st), upload(d_keep, k32.data(), k32.size(), st), upload(d_K, &K, 1, st);
        cols.ensure((size_t)nb * T * Kp + 16), d_cmp.ensure((size_t)nb * TT + 2), d_same.ensure((size_t)nb * TT + 2);
        boot_counts_batch(st, d_matrix.p, T, L, K, d_keep.p, d_K.p, (ull)seed, (u32)b0, nb, cols.p, d_cmp.p, d_same.p);
        HIP_CHECK(hipGetLastError());
        out->cmp = (int64_t*)host_copy(who.c_str(), d_cmp.p, (size_t)nb * TT, st);
        out->same = (int64_t*)host_copy(who.c_str(), d_same.p, (size_t)nb * TT, st);
        call.wait();
        out->waits = call.waits, out->batches = 1;
        fill_empty_slots(slots(out));
    });
}

void so_phy_subst_free(so_phy_subst_result* r) {
    if (r) release_slots(r, slots(r));
}

int so_phy_subst(int device, int64_t n_taxa, int64_t n_cols, const uint8_t* matrix, int64_t n_keep, const int64_t* keep, uint64_t seed, int64_t b0, int64_t n_reps,
                 int32_t flags, so_phy_subst_result* out) {
    const std::string who = "so_phy_subst";
    return guarded_call(g_phy_err, out, so_phy_subst_free, [&] {
        if (!out) throw SoError(who + ": result pointer is NULL");
        memset(out, 0, sizeof *out);
        if (flags & ~3) throw SoError(who + ": unknown flag bits (bit 0: no tensor in the result, bit 1: the two passes timed by events)");
        if (n_reps < 0) throw SoError(who + ": n_reps is 0 (the kept columns) or the number of replicates (n_reps is " + std::to_string(n_reps) + ")");
        const bool draw = n_reps > 0;
        const std::vector<int> k32 = boot_check(who, n_taxa, n_cols, matrix, n_keep, keep, draw ? b0 : 0, draw ? n_reps : 1);
        if (n_reps > PHY_BOOT_MAX_BATCH) throw SoError(who + ": more than " + std::to_string(PHY_BOOT_MAX_BATCH) + " replicates in one call are not supported");
        const bool want_tensor = !(flags & 1), timed = flags & 2;
        const u32 T = (u32)n_taxa, L = (u32)n_cols, K = (u32)n_keep, nb = draw ? (u32)n_reps : 1u, Kp = (K + 31u) & ~31u;
        const size_t P = (size_t)T * (T - 1u) / 2u, per = P * 400u, bytes = (size_t)nb * per * sizeof(int);
        out->n_taxa = n_taxa, out->n_pairs = (int64_t)P, out->n_reps = nb, out->bytes = (int64_t)bytes;
        check_device(who.c_str(), device);
        DeviceCall call(device);
        hipStream_t st = call.st;
        refuse_over_half_free(who, "tensor of " + std::to_string(nb) + " x " + std::to_string(P) + " pairs", bytes);
        DevBuf<u8> d_matrix, codes;
        DevBuf<int> d_keep, d_out;
        upload(d_matrix, matrix, (size_t)T * L, st), upload(d_keep, k32.data(), k32.size(), st);
        codes.ensure((size_t)nb * T * Kp + 16), d_out.ensure((size_t)nb * per + 2);
        StageEvents ev(timed);
        HIP_CHECK(hipMemsetAsync(d_out.p, 0, bytes, st));
        ev.mark(0, st);
        hipLaunchKernelGGL(k_phy_code, dim3((Kp + 255u) / 256u, (T + PHY_BOOT_TAXA - 1u) / PHY_BOOT_TAXA, nb), dim3(256), 0, st, d_matrix.p, T, L, K, Kp, d_keep.p, (ull)seed,
                           (u32)(draw ? b0 : 0), draw ? 1u : 0u, codes.p);
        ev.mark(1, st);
        const u32 nt = (20u * T + PHS_TILE - 1u) / PHS_TILE;   // tiles per side; columns per range (whole chunks), ranges
        const auto [cps, ranges] = range_grid(Kp, PHS_CHUNK_COLS, (u64)nt * (nt + 1u) / 2u * nb, PHS_TARGET_WGS);
        hipLaunchKernelGGL(k_phy_subst, dim3(nt * nt, ranges, nb), dim3(256), 0, st, codes.p, T, Kp, nt, cps, d_out.p, (size_t)T * Kp, per);
        ev.mark(2, st);
        HIP_CHECK(hipGetLastError());
        static_assert(sizeof(int) == sizeof(int32_t), "the counts are copied out as int32");
        if (want_tensor) out->subst = host_copy(who.c_str(), d_out.p, (size_t)nb * per, st);
        call.wait();
        out->waits = call.waits;
        out->code_ms = ev.ms(0), out->product_ms = ev.ms(1);
        fill_empty_slots(slots(out));
    });
}

int so_phy_nj_splits(int device, int64_t n_reps, int64_t n_taxa, const double* D, int32_t flags, so_phy_boot_result* out) {
    return nj_call("so_phy_nj_splits", device, n_reps, n_taxa, D, nullptr, flags, out, so_phy_boot_free);
}

int so_phy_boot(int device, int64_t n_taxa, int64_t n_cols, const uint8_t* matrix, int64_t n_keep, const int64_t* keep, uint64_t seed, int64_t n_reps,
                const uint64_t* ref_splits, int32_t flags, so_phy_boot_result* out) {
    const std::string who = "so_phy_boot";
    return guarded_call(g_phy_err, out, so_phy_boot_free, [&] {
        if (!out) throw SoError(who + ": result pointer is NULL");
        memset(out, 0, sizeof *out);
        if (flags & ~3) throw SoError(who + ": unknown flag bits (bit 0: every replicate's splits in the result, bit 1: the stages timed by events)");
        const std::vector<int> k32 = boot_check(who, n_taxa, n_cols, matrix, n_keep, keep, 0, n_reps);
        const u32 T = (u32)n_taxa, L = (u32)n_cols, K = (u32)n_keep, Kp = (K + 15u) & ~15u, W = (T + 63u) / 64u, S = T > 3u ? T - 3u : 0u;
        if (S && !ref_splits) throw SoError(who + ": ref_splits is NULL");
        const bool want_splits = flags & 1, timed = flags & 2;
        const size_t TT = (size_t)T * T, B = (size_t)n_reps, SW = (size_t)S * W;
        out->n_taxa = n_taxa, out->n_reps = n_reps, out->n_splits = S, out->n_words = W;
        check_device(who.c_str(), device);
        const char* w = who.c_str();
        DeviceCall call(device);
        hipStream_t st = call.st;
        DevBuf<u8> d_matrix, cols, d_ok;
        DevBuf<int> d_keep;
        DevBuf<u32> d_K, d_count;
        DevBuf<ull> d_cmp, d_same, d_ref, d_splits, clades;
        DevBuf<double> d_D;
        upload(d_matrix, matrix, (size_t)T * L, st), upload(d_keep, k32.data(), k32.size(), st), upload(d_K, &K, 1, st);
        if (S) upload(d_ref, reinterpret_cast<const ull*>(ref_splits), SW, st);
        d_count.ensure((size_t)S + 2);
        HIP_CHECK(hipMemsetAsync(d_count.p, 0, ((size_t)S + 2) * sizeof(u32), st));
        // a batch: the drawn columns, two counters and a distance per pair, the splits and the bit sets of every replicate
        const bool in_lds = S && nj_clades_fit(T, W);
        out->nj_tier = S ? (in_lds ? 1 : 2) : 0;
        const size_t per_rep = (size_t)T * Kp + 3u * TT * 8u + SW * 8u + (S && !in_lds ? (size_t)T * W * 8u : 0u) + 1u;
        const size_t batch = device_batch(call, call.tn.phy_boot_batch, per_rep, std::min(B, (size_t)PHY_BOOT_MAX_BATCH));
        cols.ensure(batch * T * Kp + 16), d_cmp.ensure(batch * TT + 2), d_same.ensure(batch * TT + 2), d_D.ensure(batch * TT + 2), d_ok.ensure(batch + 2);
        d_splits.ensure(batch * SW + 2);
        if (S && !in_lds) clades.ensure(batch * T * W + 2);
        out->ok = host_array<uint8_t>(w, B);
        if (want_splits) out->splits = host_array<uint64_t>(w, B * SW);
        out->count = host_array<int32_t>(w, S);
        static_assert(sizeof(u32) == sizeof(int32_t) && sizeof(ull) == sizeof(uint64_t), "counts and bit sets are copied out as they are");
        StageEvents ev(timed);
        for (size_t b0 = 0; b0 < B; b0 += batch) {
            const u32 nb = (u32)std::min(batch, B - b0);
            ev.mark(0, st);
            boot_counts_batch(st, d_matrix.p, T, L, K, d_keep.p, d_K.p, (ull)seed, (u32)b0, nb, cols.p, d_cmp.p, d_same.p);
            HIP_CHECK(hipMemsetAsync(d_ok.p, 1, nb, st));
            hipLaunchKernelGGL(k_phy_boot_dist, dim3((unsigned)((TT + 255) / 256), nb), dim3(256), 0, st, d_cmp.p, d_same.p, (u32)TT, d_D.p, d_ok.p);
            ev.mark(1, st);
            if (S) nj_launch(st, d_D.p, T, W, nb, d_ok.p, nullptr, nullptr, d_splits.p, in_lds ? nullptr : clades.p);
            ev.mark(2, st);
            if (S) hipLaunchKernelGGL(k_phy_boot_support, dim3((S + 255u) / 256u, nb), dim3(256), 0, st, d_ref.p, d_splits.p, S, W, d_ok.p, d_count.p);
            ev.mark(3, st);
            HIP_CHECK(hipGetLastError());
            call.fetch(out->ok + b0, d_ok.p, nb);
            if (want_splits && S) call.fetch(reinterpret_cast<ull*>(out->splits) + b0 * SW, d_splits.p, (size_t)nb * SW);
            if (b0 + nb == B && S) call.fetch(reinterpret_cast<u32*>(out->count), d_count.p, S);
            call.wait();   // the one wait of the batch: its buffers are the next batch's
            ++out->batches;
            out->counts_ms += ev.ms(0), out->trees_ms += ev.ms(1), out->support_ms += ev.ms(2);
        }
        out->waits = call.waits;
        for (size_t b = 0; b < B; ++b) out->valid += out->ok[b] ? 1 : 0;
        fill_empty_slots(slots(out));
    });
}

void so_phy_gene_free(so_phy_gene_result* r) {
    if (r) release_slots(r, slots(r));
}

int so_phy_gene_counts(int device, int64_t n_taxa, int64_t n_cols, const uint8_t* matrix, int64_t n_keep, const int64_t* keep, int64_t n_fam, const int64_t* fam_off,
                       int64_t f0, int64_t n, int32_t flags, so_phy_gene_result* out) {
    const std::string who = "so_phy_gene_counts";
    return guarded_call(g_phy_err, out, so_phy_gene_free, [&] {
        if (!out) throw SoError(who + ": result pointer is NULL");
        memset(out, 0, sizeof *out);
        if (flags != 0) throw SoError(who + ": unknown flag bits (flags is reserved and must be 0)");
        gene_check(who, n_taxa, n_cols, matrix, n_keep, keep, n_fam, fam_off);
        if (f0 < 0 || n < 1 || f0 > n_fam || n > n_fam - f0) throw SoError(who + ": the families f0 .. f0 + n - 1 lie outside 0 .. n_fam - 1");
        if (n > PHY_BOOT_MAX_BATCH) throw SoError(who + ": more than " + std::to_string(PHY_BOOT_MAX_BATCH) + " families in one call are not supported");
        std::vector<int> src;
        std::vector<u32> woff;
        gene_layout(who, keep, fam_off, f0, n, src, woff);
        const u32 T = (u32)n_taxa, L = (u32)n_cols, nf = (u32)n, nt = pair_tiles(T);
        const size_t TT = (size_t)T * T;
        out->n_taxa = n_taxa, out->n_fam = n;
        check_device(who.c_str(), device);
        DeviceCall call(device);
        hipStream_t st = call.st;
        DevBuf<u8> d_matrix, K;
        DevBuf<int> d_src;
        DevBuf<u32> d_woff, d_cmp, d_same;
        upload(d_matrix, matrix, (size_t)T * L, st), upload(d_woff, woff.data(), woff.size(), st);
        gene_gather(st, d_matrix.p, T, L, src, d_src, K);
        d_cmp.ensure((size_t)nf * TT + 2), d_same.ensure((size_t)nf * TT + 2);
        hipLaunchKernelGGL(k_phy_fam_pairs, dim3(nt * nt, 1, nf), dim3(256), 0, st, reinterpret_cast<const u32*>(K.p), T, (u32)(src.size() / 4u), d_woff.p, nt, d_cmp.p, d_same.p);
        HIP_CHECK(hipGetLastError());
        std::vector<u32> c32((size_t)nf * TT), s32((size_t)nf * TT);
        call.fetch(c32.data(), d_cmp.p, c32.size()), call.fetch(s32.data(), d_same.p, s32.size());
        call.wait();
        out->cmp = host_array<int64_t>(who.c_str(), c32.size()), out->same = host_array<int64_t>(who.c_str(), s32.size());
        for (size_t i = 0; i < c32.size(); ++i) out->cmp[i] = c32[i], out->same[i] = s32[i];
        out->waits = call.waits, out->batches = 1;
        fill_empty_slots(slots(out));
    });
}

int so_phy_nj_subsets(int device, int64_t n_reps, int64_t n_taxa, const double* D, const uint64_t* present, int32_t flags, so_phy_gene_result* out) {
    return nj_call("so_phy_nj_subsets", device, n_reps, n_taxa, D, present, flags, out, so_phy_gene_free);
}

int so_phy_gene(int device, int64_t n_taxa, int64_t n_cols, const uint8_t* matrix, int64_t n_keep, const int64_t* keep, int64_t n_fam, const int64_t* fam_off,
                const uint64_t* ref_splits, int32_t flags, so_phy_gene_result* out) {
    const std::string who = "so_phy_gene";
    return guarded_call(g_phy_err, out, so_phy_gene_free, [&] {
        if (!out) throw SoError(who + ": result pointer is NULL");
        memset(out, 0, sizeof *out);
        if (flags & ~3) throw SoError(who + ": unknown flag bits (bit 0: every family's present words and splits in the result, bit 1: the stages timed by events)");
        gene_check(who, n_taxa, n_cols, matrix, n_keep, keep, n_fam, fam_off);
        const u32 T = (u32)n_taxa, L = (u32)n_cols, W = (T + 63u) / 64u, S = T > 3u ? T - 3u : 0u, nt = pair_tiles(T);
        if (S && !ref_splits) throw SoError(who + ": ref_splits is NULL");
        std::vector<int> src;
        std::vector<u32> woff;
        gene_layout(who, keep, fam_off, 0, n_fam, src, woff);
        const bool want_all = flags & 1, timed = flags & 2;
        const size_t TT = (size_t)T * T, F = (size_t)n_fam, SW = (size_t)S * W;
        out->n_taxa = n_taxa, out->n_fam = n_fam, out->n_splits = S, out->n_words = W;
        check_device(who.c_str(), device);
        const char* w = who.c_str();
        DeviceCall call(device);
        hipStream_t st = call.st;
        DevBuf<u8> d_matrix, K, d_ok;
        DevBuf<int> d_src;
        DevBuf<u32> d_woff, d_cmp, d_same, d_np, d_dec, d_con;
        DevBuf<ull> d_ref, d_present, d_splits, clades;
        DevBuf<double> d_D;
        upload(d_matrix, matrix, (size_t)T * L, st), upload(d_woff, woff.data(), woff.size(), st);
        if (S) upload(d_ref, reinterpret_cast<const ull*>(ref_splits), SW, st);
        d_dec.ensure((size_t)S + 2), d_con.ensure((size_t)S + 2);
        HIP_CHECK(hipMemsetAsync(d_dec.p, 0, ((size_t)S + 2) * sizeof(u32), st));
        HIP_CHECK(hipMemsetAsync(d_con.p, 0, ((size_t)S + 2) * sizeof(u32), st));
        StageEvents ev(timed);
        ev.mark(0, st);
        gene_gather(st, d_matrix.p, T, L, src, d_src, K);   // (the first batch's counts stage is timed from here)
        // a batch: two 32-bit counters and a distance per pair, the present words, the splits and the bit sets of every family
        const bool in_lds = S && nj_clades_fit(T, W);
        out->nj_tier = S ? (in_lds ? 1 : 2) : 0;
        const size_t per_fam = 2u * TT * 4u + TT * 8u + SW * 8u + (S && !in_lds ? (size_t)T * W * 8u : 0u) + (size_t)W * 8u + 5u;
        const size_t batch = device_batch(call, call.tn.phy_gene_batch, per_fam, std::min(F, (size_t)PHY_BOOT_MAX_BATCH));
        d_cmp.ensure(batch * TT + 2), d_same.ensure(batch * TT + 2), d_D.ensure(batch * TT + 2), d_ok.ensure(batch + 2), d_np.ensure(batch + 2);
        d_present.ensure(batch * W + 2), d_splits.ensure(batch * SW + 2);
        if (S && !in_lds) clades.ensure(batch * T * W + 2);
        out->ok = host_array<uint8_t>(w, F), out->n_present = host_array<int32_t>(w, F);
        if (want_all) out->present = host_array<uint64_t>(w, F * W), out->splits = host_array<uint64_t>(w, F * SW);
        out->decisive = host_array<int32_t>(w, S), out->concordant = host_array<int32_t>(w, S);
        static_assert(sizeof(u32) == sizeof(int32_t) && sizeof(ull) == sizeof(uint64_t), "counts and bit sets are copied out as they are");
        for (size_t f0 = 0; f0 < F; f0 += batch) {
            const u32 nb = (u32)std::min(batch, F - f0);
            if (f0) ev.mark(0, st);
            hipLaunchKernelGGL(k_phy_fam_pairs, dim3(nt * nt, 1, nb), dim3(256), 0, st, reinterpret_cast<const u32*>(K.p), T, (u32)(src.size() / 4u), d_woff.p + f0, nt, d_cmp.p,
                               d_same.p);
            HIP_CHECK(hipMemsetAsync(d_ok.p, 1, nb, st));
            hipLaunchKernelGGL(k_phy_gene_dist, dim3((unsigned)((TT + 255) / 256), nb), dim3(256), 0, st, d_cmp.p, d_same.p, T, W, d_D.p, d_ok.p, d_present.p, d_np.p);
            ev.mark(1, st);
            if (S) nj_launch(st, d_D.p, T, W, nb, d_ok.p, d_np.p, d_present.p, d_splits.p, in_lds ? nullptr : clades.p);
            ev.mark(2, st);
            if (S)
                hipLaunchKernelGGL(k_phy_gene_concord, dim3((S + 255u) / 256u, nb), dim3(256), 0, st, d_ref.p, d_splits.p, S, W, d_ok.p, d_np.p, d_present.p, d_dec.p, d_con.p);
            ev.mark(3, st);
            HIP_CHECK(hipGetLastError());
            call.fetch(out->ok + f0, d_ok.p, nb), call.fetch(reinterpret_cast<u32*>(out->n_present) + f0, d_np.p, nb);
            if (want_all) call.fetch(reinterpret_cast<ull*>(out->present) + f0 * W, d_present.p, (size_t)nb * W);
            if (want_all && S) call.fetch(reinterpret_cast<ull*>(out->splits) + f0 * SW, d_splits.p, (size_t)nb * SW);
            if (f0 + nb == F && S) call.fetch(reinterpret_cast<u32*>(out->decisive), d_dec.p, S), call.fetch(reinterpret_cast<u32*>(out->concordant), d_con.p, S);
            call.wait();   // the one wait of the batch: its buffers are the next batch's
            ++out->batches;
            out->counts_ms += ev.ms(0), out->trees_ms += ev.ms(1), out->concord_ms += ev.ms(2);
        }
        out->waits = call.waits;
        fill_empty_slots(slots(out));
    });
}

}  // extern "C"
