// k_ixsort.hip -- the index build's grouping step (fsearch.py:2240-2266: count per bucket, prefix, fill): the (bucket id, entry) pairs
// of a chunk, emitted in position order, grouped by ascending bucket id.  The members of a bucket may come out in any order (every
// consumer derives the visiting order from the entry itself; tests/test_gpu_parity.py check_index compares buckets as sets), so no
// stable sort is needed -- counting passes over digits of the bucket id do it:
//
//   level 1   the id range [0, NC) is cut into <= 8192 BINS of W = 2^wsh ids, and 2^ssh neighbouring bins make a SUPERBIN (<= 128 of them:
//             115 of 64 bins at the default -M).  IXS_G workgroups each take a contiguous slice of the pairs: k_ixs_count builds the slice's
//             bin histogram in LDS and stores it as column g of a bins x IXS_G matrix, and its sums per superbin as column g of a second,
//             small matrix.  The exclusive scans of the two in (row, g) order are the two plans: P[bin][g], the first slot of slice g's
//             pairs inside bin's region, and Q[superbin][g], the same for the superbins.  The pairs then reach their bin in two hops:
//               k_ixs_hop1  re-reads the slice and writes every pair to its SUPERBIN's region, from the cursors Q[.][g]: a (workgroup,
//                           superbin) run is ~250 pairs;
//               k_ixs_hop2  one workgroup per (superbin S, IXS_K neighbouring slices t): its input is the contiguous piece
//                           [Q[S][tK], Q[S][(t+1)K]) those slices wrote, its cursors for the bins of S start at P[bin][tK] -- the pairs
//                           land in their bin's region [P[bin][0], P[bin+1][0]), runs of K x 3.9 pairs, back in the level-1 INPUT arrays.
//             Both move their pairs through the LDS in tiles of 4096, laid out by destination, so that a wave stores whole lines (ixs_hop).
//             No pass counts twice: hop 2's per-bin counts are sums of columns P already holds.
//             (Until r09 ONE scatter did this, k_ixs_scatter: 512 workgroups x 7 324 bins = runs of 3.9 pairs, ~66 MB of partly written
//             lines open per XCD against 4 MB of L2 -- 0.567 ms per chunk at 0.62 TB/s, the random-access rate of the part.)
//   level 2   one workgroup per bin (~2000 pairs over 16384 ids at the default -M); the bin's pairs land grouped by id.
//               k_ixs_bin_lds  bins of up to IXS_CAP = 4096 pairs and up to 16384 ids: (position, local id) words ordered in the LDS by two
//                              stable 7-bit counting passes -- the cost follows the pairs;
//               k_ixs_bin      the others: LDS counters per id (count, scan, scatter: 16384 counters whatever the bin holds); bins of more
//                              than 16384 ids (-M above 2^27) are first split by the id's upper digit (<= 32 sub-ranges, through hop 1's
//                              output arrays as scratch), then every sub-range is grouped like a bin.
//
// Measured per 50 000-sequence chunk (14.7 M pairs, -M 120000000; profiles/r09_a_ (before) / r09_b_c3only_kernel_stats.csv, one machine):
// count 0.040 + plan scans 0.04 + hop 1 0.086 + hop 2 0.081 (353 MB each way per hop: 4.1-4.4 TB/s) + bins 0.125 + 0.008 = 0.38 ms, where
// the one scatter (0.499; 0.567 on two other machines) and the counters for every bin (0.221) made it 0.80.  Tried and not kept: the hops
// with every pair stored from its own lane (0.238 + 0.239 ms: the lines do fill in the L2, but a wave instruction is still 64 store
// transactions); 8 or 32 slices per hop-2 workgroup (0.096 / 0.090 against 0.082 ms at 16); key and entry as one narrower word through
// the hops (not built: at most a third of 0.17 ms per chunk).
#include "common.h"
#include "kernels.h"
#include "tune.h"

#define IXS_G 512            // level-1 workgroups (= columns of the count matrices)
#define IXS_T1 1024          // their threads
#define IXS_BINS_MAX 8192
#define IXS_SB_MAX 128       // superbins (= destinations of hop 1)
#define IXS_K 16             // slices per hop-2 workgroup (SOHIT_IXS_K: 1 .. IXS_G / 8, a power of two)
#define IXS_TH 512           // hop-2 threads
#define IXS_W 16384          // ids per level-2 counting pass (LDS counters)
#define IXS_T2 512
#define IXS_T3 512           // threads of k_ixs_bin_lds (0.120-0.125 ms per chunk; 256: 0.156, 1024: 0.170)
#define IXS_CAP 4096         // most pairs of a bin that k_ixs_bin_lds orders in the LDS (SOHIT_IXS_CAP lowers it; 0: every bin by k_ixs_bin)

static inline int ixs_wsh(u32 NC) {   // log2 of the bin width: the fewest bits that leave <= IXS_BINS_MAX bins
    int wsh = 0;
    while ((((u64)NC + (1ull << wsh) - 1) >> wsh) > IXS_BINS_MAX) ++wsh;
    return wsh;
}
u32 ixsort_bins(u32 NC) { return (u32)(((u64)NC + (1ull << ixs_wsh(NC)) - 1) >> ixs_wsh(NC)); }
static inline int ixs_ssh(u32 nbins) {   // log2 of the bins per superbin: the fewest bits that leave <= IXS_SB_MAX superbins
    int ssh = 0;
    while (((nbins + (1u << ssh) - 1) >> ssh) > IXS_SB_MAX) ++ssh;
    return ssh;
}
static inline u32 ixs_sbins(u32 nbins) { return (nbins + (1u << ixs_ssh(nbins)) - 1) >> ixs_ssh(nbins); }
// the plan buffer: P = nbins x IXS_G words + 1, then (from a multiple of 4 words) Q = superbins x IXS_G words + 1
static inline size_t ixs_q_at(u32 nbins) { return ((size_t)nbins * IXS_G + 1 + 3) & ~(size_t)3; }
size_t ixsort_plan_elems(u32 NC) { return ixs_q_at(ixsort_bins(NC)) + (size_t)ixs_sbins(ixsort_bins(NC)) * IXS_G + 1; }
static inline u32 ixs_k() {   // slices per hop-2 workgroup: every XCD's eighth of the slices is a whole number of groups
    const long long k = tune().ixs_k;
    return k >= 1 && k <= IXS_G / 8 && (k & (k - 1)) == 0 ? (u32)k : (u32)IXS_K;
}

static inline u32 ixs_cap() {
    const long long cap = tune().ixs_cap;
    return cap >= 0 && cap <= IXS_CAP ? (u32)cap : (u32)IXS_CAP;
}

// Slice (= plan column) of this workgroup.  Workgroups are dealt round-robin to the 8 XCDs, so XCD x takes the x-th contiguous eighth of the
// slices: inside a superbin the runs of neighbouring slices are neighbours too, a line that two of them share is filled by ONE XCD's L2, and
// hop 2 (its groups numbered the same way) reads a piece on the XCD that wrote it.
__device__ __forceinline__ u32 ixs_col() { return (blockIdx.x & 7u) * (IXS_G / 8) + (blockIdx.x >> 3); }
__device__ __forceinline__ void ixs_slice(u32 E, u32& lo, u32& hi) {   // (multiples of 4 pairs but the end)
    const u64 per = (((u64)E + IXS_G - 1) / IXS_G + 3) & ~3ull;
    lo = (u32)min((u64)E, per * ixs_col()), hi = (u32)min((u64)E, per * (ixs_col() + 1));
}

__global__ __launch_bounds__(IXS_T1) void k_ixs_count(const u32* __restrict__ keys, u32 E, int wsh, u32 nbins, int ssh, u32 nsb,
                                                     u32* __restrict__ plan /*[nbins][IXS_G] (+1)*/, u32* __restrict__ qplan /*[nsb][IXS_G] (+1)*/) {
    __shared__ u32 s_cnt[IXS_BINS_MAX];
    for (u32 i = threadIdx.x; i < nbins; i += IXS_T1) s_cnt[i] = 0;
    __syncthreads();
    u32 lo, hi;
    ixs_slice(E, lo, hi);
    for (u32 i = lo + threadIdx.x; i < hi; i += IXS_T1) {
        const u32 k = keys[i];
        if (k != 0xFFFFFFFFu) atomicAdd(&s_cnt[k >> wsh], 1u);   // (~0: the slot of an invalid window, k_index_windows_sparse)
    }
    __syncthreads();
    for (u32 i = threadIdx.x; i < nbins; i += IXS_T1) plan[(size_t)i * IXS_G + ixs_col()] = s_cnt[i];
    for (u32 s = threadIdx.x; s < nsb; s += IXS_T1) {
        u32 c = 0;
        for (u32 b = s << ssh, e = min(nbins, (s + 1) << ssh); b < e; ++b) c += s_cnt[b];
        qplan[(size_t)s * IXS_G + ixs_col()] = c;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) plan[(size_t)nbins * IXS_G] = 0, qplan[(size_t)nsb * IXS_G] = 0;   // (the scans leave E there: the end of the last row)
}

// One hop inside a workgroup of T threads: the pairs [lo, hi) of (keys, vals), holes (key ~0) skipped, to (dk, dv) at the cursors s_cur[digit],
// digit = (key >> sh) - dbase < nd <= 128.  A pair written straight from its lane is a store transaction of its own (64 per wave
// instruction: measured, the two hops then take 0.238 + 0.239 ms per chunk where the one scatter took 0.551), so the pairs go through the LDS
// in TILES of T x IT: rank inside (tile, digit) from an LDS fetch-add, scan of the <= 128 counts, the tile laid out by digit in the LDS,
// and written out with neighbouring lanes on neighbouring slots -- a (tile, digit) run is one or a few whole lines.
// The caller has set s_cur and passed a barrier.
template <int T, int IT>
__device__ __forceinline__ void ixs_hop(const u32* __restrict__ keys, const u64* __restrict__ vals, u32 lo, u32 hi, int sh, u32 dbase, u32 nd, u32* s_cur,
                                        u32* __restrict__ dk, u64* __restrict__ dv) {
    __shared__ u32 s_hist[IXS_SB_MAX], s_off[IXS_SB_MAX], s_tot;
    __shared__ u32 s_k[T * IT];
    __shared__ u64 s_v[T * IT];
    const u32 tid = threadIdx.x;
    for (u32 t0 = lo; t0 < hi; t0 += T * IT) {
        if (tid < IXS_SB_MAX) s_hist[tid] = 0;
        __syncthreads();
        u32 k[IT], r[IT];
        u64 v[IT] = {};
#pragma unroll
        for (int j = 0; j < IT; ++j) {
            const u32 i = t0 + (u32)j * T + tid;
            k[j] = i < hi ? keys[i] : 0xFFFFFFFFu;
            if (k[j] != 0xFFFFFFFFu) v[j] = vals[i];
        }
#pragma unroll
        for (int j = 0; j < IT; ++j)
            if (k[j] != 0xFFFFFFFFu) r[j] = atomicAdd(&s_hist[(k[j] >> sh) - dbase], 1u);
        __syncthreads();
        if (tid < 64) {   // exclusive scan of the counts, two per lane
            const u32 c0 = s_hist[2 * tid], c1 = s_hist[2 * tid + 1];
            u32 inc = c0 + c1;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const u32 x = __shfl_up(inc, o);
                if (tid >= (u32)o) inc += x;
            }
            s_off[2 * tid] = inc - c0 - c1, s_off[2 * tid + 1] = inc - c1;
            if (tid == 63) s_tot = inc;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < IT; ++j)
            if (k[j] != 0xFFFFFFFFu) {
                const u32 p = s_off[(k[j] >> sh) - dbase] + r[j];
                s_k[p] = k[j], s_v[p] = v[j];
            }
        __syncthreads();
        const u32 n = s_tot;
        for (u32 p = tid; p < n; p += T) {
            const u32 kk = s_k[p], d = (kk >> sh) - dbase;
            const u32 at = s_cur[d] + (p - s_off[d]);
            dk[at] = kk, dv[at] = s_v[p];
        }
        __syncthreads();
        if (tid < nd) s_cur[tid] += s_hist[tid];   // (read again behind the next tile's barriers; the same thread zeroes s_hist[tid])
    }
}

// hop 1: slice -> superbin regions.  sh = wsh + ssh; qplan scanned.
__global__ __launch_bounds__(IXS_T1) void k_ixs_hop1(const u32* __restrict__ keys, const u64* __restrict__ vals, u32 E, int sh, u32 nsb,
                                                    const u32* __restrict__ qplan, u32* __restrict__ tk, u64* __restrict__ tv) {
    __shared__ u32 s_cur[IXS_SB_MAX];
    if (threadIdx.x < nsb) s_cur[threadIdx.x] = qplan[(size_t)threadIdx.x * IXS_G + ixs_col()];
    __syncthreads();
    u32 lo, hi;
    ixs_slice(E, lo, hi);
    ixs_hop<IXS_T1, 4>(keys, vals, lo, hi, sh, 0u, nsb, s_cur, tk, tv);
}

// hop 2: the piece that K neighbouring slices wrote for one superbin -> its bins' regions.  Grid: nsb x (IXS_G / K) workgroups; the groups
// of a superbin are dealt to the XCDs as the slices are (XCD x: the x-th eighth), so the runs that meet inside a bin's line come from one XCD.
__global__ __launch_bounds__(IXS_TH) void k_ixs_hop2(const u32* __restrict__ tk, const u64* __restrict__ tv, int wsh, u32 nbins, int ssh, u32 K,
                                                    const u32* __restrict__ plan /*scanned*/, const u32* __restrict__ qplan /*scanned*/,
                                                    u32* __restrict__ ok, u64* __restrict__ ov) {
    __shared__ u32 s_cur[IXS_SB_MAX];
    const u32 per = IXS_G / 8 / K;   // groups per XCD and superbin
    const u32 r = blockIdx.x >> 3;
    const u32 S = r / per, t = (blockIdx.x & 7u) * per + r % per;
    const u32 a = qplan[(size_t)S * IXS_G + (size_t)t * K], b = qplan[(size_t)S * IXS_G + (size_t)(t + 1) * K];   // (the last group's end: the next row's start, or E)
    if (a == b) return;
    const u32 b0 = S << ssh, nb = min(1u << ssh, nbins - b0);
    if (threadIdx.x < nb) s_cur[threadIdx.x] = plan[(size_t)(b0 + threadIdx.x) * IXS_G + (size_t)t * K];
    __syncthreads();
    ixs_hop<IXS_TH, 8>(tk, tv, a, b, wsh, b0, nb, s_cur, ok, ov);
}

// counting pass of one id range inside a workgroup: pairs [a, b) of (sk, sv), ids in [idbase, idbase + IXS_W), to (dk, dv) at the same
// positions, grouped by id
// (sk / sv carry no __restrict__: the split path of k_ixs_bin hands in the scratch pairs the same workgroup has just written)
__device__ __forceinline__ void ixs_group(const u32* sk, const u64* sv, u32 a, u32 b, u32 idbase, u32* __restrict__ dk,
                                          u64* __restrict__ dv, u32* s_cnt, u32* s_ws) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    constexpr int PER = IXS_W / IXS_T2;   // counters per thread in the scan
    for (int i = tid; i < IXS_W; i += IXS_T2) s_cnt[i] = 0;
    __syncthreads();
    for (u32 i = a + (u32)tid; i < b; i += IXS_T2) atomicAdd(&s_cnt[sk[i] - idbase], 1u);
    __syncthreads();
    {   // exclusive scan of the counters (each thread PER consecutive ones), + a
        u32 c[PER], tot = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) c[k] = s_cnt[tid * PER + k], tot += c[k];
        u32 inc = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u32 x = __shfl_up(inc, o);
            if (lane >= o) inc += x;
        }
        if (lane == 63) s_ws[w] = inc;
        __syncthreads();
        u32 run = a + inc - tot;
        for (int k = 0; k < w; ++k) run += s_ws[k];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            s_cnt[tid * PER + k] = run;
            run += c[k];
        }
    }
    __syncthreads();
    for (u32 i = a + (u32)tid; i < b; i += IXS_T2) {
        const u32 k = sk[i];
        const u32 at = atomicAdd(&s_cnt[k - idbase], 1u);
        dk[at] = k, dv[at] = sv[i];
    }
    __syncthreads();
}

// One stable counting pass over a 7-bit digit of n words in the LDS, src -> dst, by the IXS_T3 / 64 waves of the workgroup.  Wave w owns the w-th
// contiguous part of src and a counter column of its own (s_cnt[digit * NW + w]); the counters are scanned in (digit, wave) order, and a wave
// walks its part in order, 64 words at a time, the lanes with one digit ranked by lane number -- so words with equal digits keep their order.
__device__ __forceinline__ void ixs_lds_pass(const u32* src, u32* dst, u32 n, int shift, u32* s_cnt /*[128 * NW]*/, u32* s_ws) {
    constexpr u32 NW = IXS_T3 / 64;
    const u32 tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const u32 per = (n + IXS_T3 - 1) / IXS_T3 * 64u;   // words per wave
    const u32 lo = min(n, per * w), hi = min(n, per * (w + 1));
    s_cnt[2 * tid] = 0, s_cnt[2 * tid + 1] = 0;
    __syncthreads();
    for (u32 i = lo + lane; i < hi; i += 64) atomicAdd(&s_cnt[((src[i] >> shift) & 127u) * NW + w], 1u);
    __syncthreads();
    {
        const u32 c0 = s_cnt[2 * tid], c1 = s_cnt[2 * tid + 1];
        u32 inc = c0 + c1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u32 x = __shfl_up(inc, o);
            if (lane >= (u32)o) inc += x;
        }
        if (lane == 63) s_ws[w] = inc;
        __syncthreads();
        u32 run = inc - c0 - c1;
        for (u32 k = 0; k < w; ++k) run += s_ws[k];
        s_cnt[2 * tid] = run, s_cnt[2 * tid + 1] = run + c0;
    }
    __syncthreads();
    for (u32 i0 = lo; i0 < hi; i0 += 64) {   // (wave-uniform bounds)
        const u32 i = i0 + lane;
        const bool live = i < hi;
        const u32 x = live ? src[i] : 0u, d = (x >> shift) & 127u;
        unsigned long long peers = __ballot(live);
#pragma unroll
        for (int bit = 0; bit < 7; ++bit) {
            const unsigned long long m = __ballot((d >> bit) & 1u);
            peers &= ((d >> bit) & 1u) ? m : ~m;
        }
        if (live) {
            const u32 rank = (u32)__popcll(peers & ((1ull << lane) - 1ull)), cnt = (u32)__popcll(peers);
            const u32 base = s_cnt[d * NW + w];   // (the column is this wave's own: read by all peers, then advanced by the last of them)
            dst[base + rank] = x;
            if (rank + 1 == cnt) s_cnt[d * NW + w] = base + cnt;
        }
    }
    __syncthreads();
}

// level 2 where the work follows the bin's PAIRS, not its ids: a bin of up to cap <= IXS_CAP pairs and up to 16384 ids is ordered in the LDS as
// words (position in the bin << 14 | local id) by two stable 7-bit passes, low digit first, and written out from there, each value fetched
// from its old position (the bin's 16 KB of values are in the L2).  ~2000 pairs go through 2 x 1024 counters where k_ixs_bin zeroes,
// fills and scans 16384.  Bins with more pairs or more ids are left to k_ixs_bin.
__global__ __launch_bounds__(IXS_T3) void k_ixs_bin_lds(const u32* __restrict__ tk, const u64* __restrict__ tv, const u32* __restrict__ plan, int wsh, u32 cap,
                                                        u32* __restrict__ ok, u64* __restrict__ ov) {
    __shared__ u32 s_a[IXS_CAP], s_b[IXS_CAP];
    __shared__ u32 s_cnt[128 * (IXS_T3 / 64)];
    __shared__ u32 s_ws[IXS_T3 / 64];
    const u32 bin = blockIdx.x;
    const u32 a = plan[(size_t)bin * IXS_G], n = plan[(size_t)(bin + 1) * IXS_G] - a;
    if (n == 0 || n > cap || wsh > 14) return;
    const u32 idbase = bin << wsh;
    for (u32 i = threadIdx.x; i < n; i += IXS_T3) s_a[i] = (tk[a + i] - idbase) | (i << 14);
    __syncthreads();
    ixs_lds_pass(s_a, s_b, n, 0, s_cnt, s_ws);
    ixs_lds_pass(s_b, s_a, n, 7, s_cnt, s_ws);
    for (u32 p = threadIdx.x; p < n; p += IXS_T3) {
        const u32 x = s_a[p];
        ok[a + p] = idbase + (x & 16383u), ov[a + p] = tv[a + (x >> 14)];
    }
}

// ... and the bins it leaves: more than cap pairs (one LDS counter per id), or more than 16384 ids (split first)
__global__ __launch_bounds__(IXS_T2) void k_ixs_bin(const u32* __restrict__ tk, const u64* __restrict__ tv, const u32* __restrict__ plan, int wsh, u32 cap,
                                                    u32* ak, u64* av /*scratch (hop 1's output), bins wider than IXS_W only: written, then re-read by this workgroup*/,
                                                    u32* __restrict__ ok, u64* __restrict__ ov) {
    __shared__ u32 s_cnt[IXS_W];
    __shared__ u32 s_ws[IXS_T2 / 64];
    __shared__ u32 s_sub[34];
    const u32 bin = blockIdx.x;
    const u32 a = plan[(size_t)bin * IXS_G], b = plan[(size_t)(bin + 1) * IXS_G];
    if (a == b || (wsh <= 14 && b - a <= cap)) return;
    const u32 idbase = bin << wsh;
    if (wsh <= 14) {
        ixs_group(tk, tv, a, b, idbase, ok, ov, s_cnt, s_ws);
        return;
    }
    // a bin of 2^wsh > 16384 ids: split by the id's digit above bit 14 first (<= 32 sub-ranges: NC < 2^32, <= 8192 bins), then every sub-range
    const u32 nsub = 1u << (wsh - 14);
    const int tid = threadIdx.x;
    if (tid < 34) s_sub[tid] = 0;
    __syncthreads();
    for (u32 i = a + (u32)tid; i < b; i += IXS_T2) atomicAdd(&s_sub[(tk[i] - idbase) >> 14], 1u);
    __syncthreads();
    if (tid == 0) {
        u32 run = a;
        for (u32 j = 0; j <= nsub; ++j) {
            const u32 c = j < nsub ? s_sub[j] : 0u;
            s_sub[j] = run;
            run += c;
        }
    }
    __syncthreads();
    u32 sub_lo[32];   // (kept per thread: the cursors below overwrite the starts)
    for (u32 j = 0; j < nsub; ++j) sub_lo[j] = s_sub[j];
    const u32 sub_end = s_sub[nsub];
    __syncthreads();
    for (u32 i = a + (u32)tid; i < b; i += IXS_T2) {
        const u32 k = tk[i];
        const u32 at = atomicAdd(&s_sub[(k - idbase) >> 14], 1u);
        ak[at] = k, av[at] = tv[i];
    }
    __threadfence();
    __syncthreads();
    for (u32 j = 0; j < nsub; ++j) {
        const u32 sa = sub_lo[j], sb = j + 1 < nsub ? sub_lo[j + 1] : sub_end;
        if (sa < sb) ixs_group(ak, av, sa, sb, idbase + (j << 14), ok, ov, s_cnt, s_ws);   // (wave-uniform condition: barriers inside are safe)
    }
}

// keys in [0, NC), or ~0 = no pair in this slot (n slots in all).  plan: ixsort_plan_elems(NC) u32; (tk, tv), (kout, vout): E pairs, E = the
// number of valid slots = the plan's last word after ixsort_count; (kin, vin) are overwritten (hop 2 writes them, k_ixs_bin reads them).
const u32* ixsort_count(const u32* kin, u32 n, u32 NC, u32* plan, u32* scan_tmp, hipStream_t st) {   // -> device word holding E
    const int wsh = ixs_wsh(NC);
    const u32 nbins = ixsort_bins(NC), nsb = ixs_sbins(nbins);
    u32* qplan = plan + ixs_q_at(nbins);
    hipLaunchKernelGGL(k_ixs_count, dim3(IXS_G), dim3(IXS_T1), 0, st, kin, n, wsh, nbins, ixs_ssh(nbins), nsb, plan, qplan);
    scan_u32(plan, plan, (size_t)nbins * IXS_G + 1, false, scan_tmp, st);
    scan_u32(qplan, qplan, (size_t)nsb * IXS_G + 1, false, scan_tmp, st);
    return plan + (size_t)nbins * IXS_G;
}
void ixsort_finish(u32* kin, u64* vin, u32 n, u32 NC, const u32* plan, u32* tk, u64* tv, u32* kout, u64* vout, hipStream_t st) {
    if (!n) return;
    const int wsh = ixs_wsh(NC);
    const u32 nbins = ixsort_bins(NC), nsb = ixs_sbins(nbins), K = ixs_k();
    const int ssh = ixs_ssh(nbins);
    const u32* qplan = plan + ixs_q_at(nbins);
    hipLaunchKernelGGL(k_ixs_hop1, dim3(IXS_G), dim3(IXS_T1), 0, st, kin, vin, n, wsh + ssh, nsb, qplan, tk, tv);
    hipLaunchKernelGGL(k_ixs_hop2, dim3(nsb * (IXS_G / K)), dim3(IXS_TH), 0, st, tk, tv, wsh, nbins, ssh, K, plan, qplan, kin, vin);
    const u32 cap = ixs_cap();
    if (cap && wsh <= 14) hipLaunchKernelGGL(k_ixs_bin_lds, dim3(nbins), dim3(IXS_T3), 0, st, kin, vin, plan, wsh, cap, kout, vout);
    hipLaunchKernelGGL(k_ixs_bin, dim3(nbins), dim3(IXS_T2), 0, st, kin, vin, plan, wsh, cap, tk, tv, kout, vout);   // (what the first leaves: a workgroup whose bin is done ends at once)
}
void ixsort_pairs(u32* kin, u64* vin, u32 E, u32 NC, u32* plan, u32* scan_tmp, u32* tk, u64* tv, u32* kout, u64* vout, hipStream_t st) {
    if (!E) return;
    (void)ixsort_count(kin, E, NC, plan, scan_tmp, st);
    ixsort_finish(kin, vin, E, NC, plan, tk, tv, kout, vout, st);
}
