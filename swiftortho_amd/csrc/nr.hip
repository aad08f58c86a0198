// nr.hip -- the expansion of a collapsed search on the device: SwiftOrtho's scripts/nr2full.py (14-44) as swiftortho_amd/nr.py
// `expand_records()` restates it on so_hit records.  The collapsed proteome holds one record per distinct sequence; a hit between
// collapsed query c (members m_0 .. m_{k-1}) and a collapsed subject with n members stands for k * n hits of the full file.
//
// Closed form.  A run = a maximal stretch of consecutive records with one qidx.  For the run of collapsed query c with rows j = 0 .. t-1,
// n_j = members of row j's subject, S = sum n_j, P_j = sum_{i<j} n_i: the record of (member a, row j, subject member b) stands at
//     base_c + a * S + P_j + b,        base_c = the expanded records of all earlier runs,
// and equals row j with qidx = m_a and sidx = subject member b.  That is nr2full's order: inside a run the rows are grouped by individual
// query (first-appearance order = member order), inside a group they keep generation order.
//
// Kernels, all on the call's one stream; every position follows from count -> scan -> emit, no atomics, nothing depends on scheduling:
//   k_nr_weigh    per row: k_c * n_j, n_j and [qidx differs from the row before]; a qidx / sidx outside its table raises an error word
//                 (every lane that raises it stores the same value) and weighs nothing
//   k_nr_reduce, k_nr_blocksums, k_nr_apply    one 64-bit exclusive scan of the three columns at once (blockIdx.y picks the column):
//                 W (where a row's weight starts: base_c at the first row of a run), N (P_j + N at the run's first row), R (run number)
//   k_nr_runs     per run r: its first row, W and N there; entry n_runs closes the tables with the totals
//   k_nr_emit     by OUTPUT: a workgroup takes NR_PIECE consecutive output records; each lane finds the run of its record in the runs'
//                 bases, a = rel / S, the row in N, b; builds the record in LDS; the workgroup then writes its piece as consecutive
//                 16-byte stores.  (With a thread per SOURCE row the single row between two collapsed records of 700 members each
//                 would be 490 000 records, 39 MB, written by one thread.)
// Host waits (after the member tables are up): one for the totals (n_out, n_runs, the error words: they size the buffer and are the
// count-only answer), one for the end.
#include "common.h"
#include "device_call.h"
#include "../../include/sohit.h"

#include <cstring>
#include <string>
#include <vector>

namespace {

#define NR_PIECE 256     // output records per workgroup of k_nr_emit (swiftortho_amd/nr.py EXPAND_PIECE)
#define NR_THREADS 256   // rows per workgroup of the row kernels and of the scan
#define NR_REC16 5       // an so_hit record is five 16-byte words; the first holds qidx and sidx
#define NR_WCAP (1ull << 32)

static_assert(sizeof(so_hit) == 16 * NR_REC16, "so_hit is 80 bytes");
static_assert(NR_PIECE == NR_THREADS, "k_nr_emit: one lane per record of the piece");

inline dim3 nr_grid(size_t n, unsigned y = 1) { return dim3((unsigned)((n + NR_THREADS - 1) / NR_THREADS), y); }

__global__ __launch_bounds__(NR_THREADS) void k_nr_weigh(const uint4* __restrict__ hits, u32 n, const i64* __restrict__ qoff, i64 nq, const i64* __restrict__ soff,
                                                          i64 ns, u64* __restrict__ W, u64* __restrict__ N, u64* __restrict__ R, u32* __restrict__ err) {
    const size_t i = (size_t)blockIdx.x * NR_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint4 h = hits[i * NR_REC16];
    const i64 q = (i64)(((u64)h.y << 32) | h.x), s = (i64)(((u64)h.w << 32) | h.z);
    u64 k = 0, m = 0;
    if (q < 0 || q >= nq) err[0] = 1u;
    else if (s < 0 || s >= ns) err[1] = 1u;
    else k = (u64)(qoff[q + 1] - qoff[q]), m = (u64)(soff[s + 1] - soff[s]);
    u64 head = 1;
    if (i) {
        const uint4 p = hits[(i - 1) * NR_REC16];
        head = (p.x != h.x || p.y != h.y) ? 1u : 0u;
    }
    // (a weight is capped at 2^32: 2^31 rows of them still add up in 64 bits, and one capped row alone puts the total past what is served)
    const u64 w = k * m;
    W[i] = w < NR_WCAP ? w : NR_WCAP, N[i] = m, R[i] = head;
}

__device__ __forceinline__ u64 nr_block_excl_scan(u64 v, u64* lds4, u64* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    u64 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up((unsigned long long)inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) lds4[w] = inc;
    __syncthreads();
    u64 base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < NR_THREADS / 64; ++k) {
        const u64 s = lds4[k];
        if (k < w) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// column y = blockIdx.y of v (stride apart); its block sums at bs + y * bstride
__global__ __launch_bounds__(NR_THREADS) void k_nr_reduce(const u64* __restrict__ v, size_t stride, u32 n, u64* __restrict__ bs, size_t bstride) {
    __shared__ u64 lds4[4];
    const size_t i = (size_t)blockIdx.x * NR_THREADS + threadIdx.x;
    u64 tot;
    nr_block_excl_scan(i < n ? v[blockIdx.y * stride + i] : 0ull, lds4, &tot);
    if (threadIdx.x == 0) bs[blockIdx.y * bstride + blockIdx.x] = tot;
}
// one workgroup per column: exclusive scan of its nb block sums in place; the column's total goes to bs[nb] and to v[n]
__global__ __launch_bounds__(NR_THREADS) void k_nr_blocksums(u64* __restrict__ bs, size_t bstride, size_t nb, u64* __restrict__ v, size_t stride, u32 n) {
    __shared__ u64 lds4[4];
    u64* b = bs + blockIdx.y * bstride;
    u64 carry = 0;
    for (size_t b0 = 0; b0 < nb; b0 += NR_THREADS) {
        const size_t i = b0 + threadIdx.x;
        u64 tot;
        const u64 ex = nr_block_excl_scan(i < nb ? b[i] : 0ull, lds4, &tot);
        if (i < nb) b[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) b[nb] = carry, v[blockIdx.y * stride + n] = carry;
}
__global__ __launch_bounds__(NR_THREADS) void k_nr_apply(u64* __restrict__ v, size_t stride, u32 n, const u64* __restrict__ bs, size_t bstride) {
    __shared__ u64 lds4[4];
    const size_t i = (size_t)blockIdx.x * NR_THREADS + threadIdx.x;
    u64* a = v + blockIdx.y * stride;
    u64 tot;
    const u64 ex = nr_block_excl_scan(i < n ? a[i] : 0ull, lds4, &tot);
    if (i < n) a[i] = bs[blockIdx.y * bstride + blockIdx.x] + ex;
}

// row i opens run R[i] when the scan steps there; i == n closes the tables
__global__ __launch_bounds__(NR_THREADS) void k_nr_runs(const u64* __restrict__ W, const u64* __restrict__ N, const u64* __restrict__ R, u32 n,
                                                         u64* __restrict__ rbase, u64* __restrict__ rN, u32* __restrict__ rrow) {
    const size_t i = (size_t)blockIdx.x * NR_THREADS + threadIdx.x;
    if (i > n) return;
    if (i < n && R[i + 1] == R[i]) return;
    const u64 r = R[i];
    rbase[r] = W[i], rN[r] = N[i], rrow[r] = (u32)i;
}

// Work goes by OUTPUT, not by source row: a thread per source row would leave the one row between two collapsed records of 700 members
// each -- 490 000 records, 39 MB -- to a single thread.  Lane t of workgroup g builds output record g * NR_PIECE + t in LDS; the piece then
// leaves as consecutive 16-byte stores.
__global__ __launch_bounds__(NR_THREADS) void k_nr_emit(const uint4* __restrict__ hits, const u64* __restrict__ N, const u64* __restrict__ rbase,
                                                         const u64* __restrict__ rN, const u32* __restrict__ rrow, u32 nruns, const i64* __restrict__ qoff,
                                                         const int* __restrict__ qmem, const i64* __restrict__ soff, const int* __restrict__ smem, u64 n_out,
                                                         uint4* __restrict__ out) {
    __shared__ uint4 piece[NR_PIECE * NR_REC16];
    const u64 o0 = (u64)blockIdx.x * NR_PIECE, o = o0 + threadIdx.x;
    if (o < n_out) {
        // the run: the largest r with rbase[r] <= o (rbase[0] = 0; runs that weigh nothing share their successor's base and are passed over)
        u32 lo = 0, hi = nruns;
        while (hi - lo > 1) {
            const u32 mid = lo + (hi - lo) / 2;
            if (rbase[mid] <= o) lo = mid;
            else hi = mid;
        }
        const u32 r = lo;
        const u64 n0 = rN[r], S = rN[r + 1] - n0, rel = o - rbase[r];
        const u64 a = rel / S, rem = rel - a * S;
        // the row: the largest j of the run with P_j <= rem
        lo = rrow[r], hi = rrow[r + 1];
        while (hi - lo > 1) {
            const u32 mid = lo + (hi - lo) / 2;
            if (N[mid] - n0 <= rem) lo = mid;
            else hi = mid;
        }
        const u64 b = rem - (N[lo] - n0);
        const uint4* src = hits + (size_t)lo * NR_REC16;
        const uint4 h = src[0];
        const i64 q = (i64)(((u64)h.y << 32) | h.x), s = (i64)(((u64)h.w << 32) | h.z);
        const i64 qm = qmem[qoff[q] + (i64)a], sm = smem[soff[s] + (i64)b];
        uint4* dst = piece + threadIdx.x * NR_REC16;
        dst[0] = make_uint4((u32)(u64)qm, (u32)((u64)qm >> 32), (u32)(u64)sm, (u32)((u64)sm >> 32));
#pragma unroll
        for (int k = 1; k < NR_REC16; ++k) dst[k] = src[k];
    }
    __syncthreads();
    const u64 left = n_out - o0;   // (o0 < n_out: the grid covers the output exactly)
    const u32 words = (u32)(left < NR_PIECE ? left : (u64)NR_PIECE) * NR_REC16;
    uint4* dst = out + o0 * NR_REC16;
    for (u32 c = threadIdx.x; c < words; c += NR_THREADS) dst[c] = piece[c];
}

// off[0 .. n] rises from 0 and mem[0 .. off[n]) names every member 0 .. off[n] - 1 exactly once
void nr_check_table(const char* side, const int64_t* off, const int32_t* mem, int64_t n) {
    const std::string who = std::string("so_nr_expand: the ") + side + " member table ";
    if (n >= (1ll << 31)) throw SoError(who + "holds 2^31 distinct sequences or more");
    if (n == 0) return;
    if (!off) throw SoError(who + "has no offsets");
    if (off[0] != 0) throw SoError(who + "does not start at 0");
    for (int64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) throw SoError(who + "does not rise: off[" + std::to_string(i + 1) + "] < off[" + std::to_string(i) + "]");
    const int64_t m = off[n];
    if (m >= (1ll << 31)) throw SoError(who + "holds 2^31 members or more");
    if (m > 0 && !mem) throw SoError(who + "has no members");
    std::vector<u8> seen((size_t)m, 0);
    for (int64_t i = 0; i < m; ++i) {
        if (mem[i] < 0 || mem[i] >= m) throw SoError(who + "names member " + std::to_string(mem[i]) + " outside 0 .. " + std::to_string(m - 1) + " (a member is missing)");
        if (seen[(size_t)mem[i]]) throw SoError(who + "names member " + std::to_string(mem[i]) + " twice");
        seen[(size_t)mem[i]] = 1;
    }
}

thread_local std::string g_nr_err;

}  // namespace

extern "C" {

const char* so_nr_last_error(void) { return g_nr_err.c_str(); }

void so_nr_expand_free(so_nr_expand_result* r) {
    if (!r) return;
    if (r->d_out) (void)hipFree(r->d_out);
    memset(r, 0, sizeof *r);
}

int so_nr_expand(int device, const so_hit* d_hits, int64_t n, const int64_t* qoff, const int32_t* qmem, int64_t n_q, const int64_t* soff, const int32_t* smem,
                 int64_t n_s, int32_t flags, so_nr_expand_result* out) {
    void* d_out = nullptr;   // the output until the result owns it: released with the result when the call is refused
    auto drop = [&](so_nr_expand_result* r) {
        if (d_out) (void)hipFree(d_out);
        memset(r, 0, sizeof *r);
    };
    return guarded_call(g_nr_err, out, drop, [&] {
        if (!out) throw SoError("so_nr_expand: result pointer is NULL");
        memset(out, 0, sizeof *out);
        if (n < 0 || n_q < 0 || n_s < 0) throw SoError("so_nr_expand: a negative count");
        if (n >= (1ll << 31)) throw SoError("so_nr_expand: 2^31 records and more are not served (32-bit row indices)");
        nr_check_table("query", qoff, qmem, n_q);
        nr_check_table("subject", soff, smem, n_s);
        if (n > 0 && !d_hits) throw SoError("so_nr_expand: the record pointer is NULL");
        if ((uintptr_t)d_hits & 15u) throw SoError("so_nr_expand: the records are not 16-byte aligned");
        check_device("so_nr_expand", device);
        out->n_in = n;
        if (n == 0) return;   // nothing to launch (a grid of 0 blocks is an invalid configuration)

        // the records must be complete before this call's own stream reads them: wait for everything queued on the device so far
        // (the ordering rule of so_orth_*_records)
        DeviceCall call(device, true);
        const hipStream_t st = call.st;

        const size_t R = (size_t)n, nb = (R + NR_THREADS - 1) / NR_THREADS;
        const size_t stride = R + 2, bstride = nb + 2;
        const i64 zero = 0;
        const i64 mq = n_q ? qoff[n_q] : 0, ms = n_s ? soff[n_s] : 0;
        DevBuf<i64> d_qoff, d_soff;
        DevBuf<int> d_qmem, d_smem;
        DevBuf<u64> v, bs, rbase, rN;
        DevBuf<u32> rrow, err;
        upload(d_qoff, n_q ? qoff : &zero, (size_t)n_q + 1, st), upload(d_soff, n_s ? soff : &zero, (size_t)n_s + 1, st);
        upload(d_qmem, qmem, (size_t)mq, st), upload(d_smem, smem, (size_t)ms, st);
        v.ensure(3 * stride), bs.ensure(3 * bstride), rbase.ensure(R + 2), rN.ensure(R + 2), rrow.ensure(R + 2), err.ensure(4);
        u64 *W = v.p, *N = v.p + stride, *Rn = v.p + 2 * stride;
        const uint4* hits16 = reinterpret_cast<const uint4*>(d_hits);
        HIP_CHECK(hipMemsetAsync(err.p, 0, 2 * sizeof(u32), st));
        hipLaunchKernelGGL(k_nr_weigh, nr_grid(R), dim3(NR_THREADS), 0, st, hits16, (u32)R, d_qoff.p, (i64)n_q, d_soff.p, (i64)n_s, W, N, Rn, err.p);
        hipLaunchKernelGGL(k_nr_reduce, nr_grid(R, 3), dim3(NR_THREADS), 0, st, v.p, stride, (u32)R, bs.p, bstride);
        hipLaunchKernelGGL(k_nr_blocksums, dim3(1, 3), dim3(NR_THREADS), 0, st, bs.p, bstride, nb, v.p, stride, (u32)R);
        hipLaunchKernelGGL(k_nr_apply, nr_grid(R, 3), dim3(NR_THREADS), 0, st, v.p, stride, (u32)R, bs.p, bstride);
        hipLaunchKernelGGL(k_nr_runs, nr_grid(R + 1), dim3(NR_THREADS), 0, st, W, N, Rn, (u32)R, rbase.p, rN.p, rrow.p);
        HIP_CHECK(hipGetLastError());
        u64 n_out = 0, n_runs = 0;
        u32 herr[2] = {0, 0};
        HIP_CHECK(hipMemcpyAsync(&n_out, W + R, sizeof(u64), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(&n_runs, Rn + R, sizeof(u64), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(herr, err.p, sizeof herr, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));   // wait 1: the totals
        out->waits = 1;
        if (herr[0]) throw SoError("so_nr_expand: a record's qidx lies outside 0 .. n_q - 1 (" + std::to_string(n_q) + " collapsed queries)");
        if (herr[1]) throw SoError("so_nr_expand: a record's sidx lies outside 0 .. n_s - 1 (" + std::to_string(n_s) + " collapsed subjects)");
        if (n_runs < 1 || n_runs > R) throw SoError("so_nr_expand: internal error: " + std::to_string(n_runs) + " runs among " + std::to_string(R) + " records");
        if (n_out >= (1ull << 31)) throw SoError("so_nr_expand: the records expand to " + std::to_string(n_out) + " or more; 2^31 and more are not served (the orthology stage refuses them too)");
        out->n_out = (int64_t)n_out, out->n_runs = (int64_t)n_runs;
        if ((flags & 1) || n_out == 0) return;

        const size_t bytes = (size_t)n_out * sizeof(so_hit);
        {
            const hipError_t e = hipMalloc(&d_out, bytes);
            if (e == hipErrorOutOfMemory) {
                (void)hipGetLastError();
                d_out = nullptr;
                throw DevOom(bytes);
            }
            HIP_CHECK(e);
        }
        if (call.tn.poison >= 0) HIP_CHECK(hipMemsetAsync(d_out, (int)call.tn.poison & 0xFF, bytes, st));
        hipLaunchKernelGGL(k_nr_emit, dim3((unsigned)((n_out + NR_PIECE - 1) / NR_PIECE)), dim3(NR_THREADS), 0, st, hits16, N, rbase.p, rN.p, rrow.p, (u32)n_runs, d_qoff.p,
                           d_qmem.p, d_soff.p, d_smem.p, n_out, reinterpret_cast<uint4*>(d_out));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));   // wait 2: the end
        out->waits = 2;
        out->d_out = (so_hit*)d_out;
    });
}

}  // extern "C"
