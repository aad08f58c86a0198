// apc.hip -- affinity propagation on the edge list of the orthology graph, on the device: the loop of SwiftOrtho's
// bin/find_cluster.py `apclust_blk` (404-513) with its five passes `max_row`, `update_R`, `sum_col`, `update_A`, `get_change`
// (309-401), as `main` runs it for `-a apc` with a batch size above zero.
//
// The reference walks a list of entries (i, k, s, R, A) -- float32 on disk, float64 while a pass works on them -- five times per round,
// 100 rounds, and its labels depend on every rounding and on every tie, so each pass reproduces the reference's ARITHMETIC ORDER:
//   * every operation is one IEEE float64 add, multiply or compare (no contraction: the library is built with -ffp-contract=off, and the
//     products and sums are spelled __dmul_rn / __dadd_rn), R and A are rounded to float32 once per pass when they are stored;
//   * the row maxima (m1, k1, m2) are CARRIED from round to round (the reference never resets them; they start at 0, k1 at gene 0), a
//     displaced maximum is not demoted to second place, and `k2` is never read by any pass, so it is not kept;
//   * `diag5[i]` is the UNROUNDED float64 R of the last entry of row i that lies on the diagonal (the preference entry);
//   * the column sum adds max(0, R) of the float32-rounded R in entry order, sequentially;
//   * Python's min(0, x) / max(0, x) are explicit compares (x only when strictly below / above 0: a NaN gives 0);
//   * `get_change` starts every round from -inf, the first maximum of a row wins, and a row without one keeps its label.
//
// Layout.  The entries are grouped by row once per call (a stable counting sort on the host: entry order survives inside each row), and
// (k, s, R, A) live in that order, so a row is one contiguous range.  A second stable grouping by column gives, per column, the
// positions of its entries in entry order and their rows.  A round is two kernels:
//   k_apc_row : get_change of the round before, max_row and update_R of this one -- all three read R + A of the same row once;
//   k_apc_col : sum_col and update_A -- both walk the same column.
// Rows / columns of up to APC_LANE_MAX entries are walked literally by one lane; longer ones by one wave, 64 entries at a time.  The wave
// form of the row passes rests on the exclusive prefix maximum pm of R + A along the row, seeded with the carried m1: an entry replaces
// the maximum iff ra > pm ("updater"); m1 / k1 come from the last updater; the others are the candidates for m2, which moves only when
// their maximum exceeds the carried m2, to the FIRST candidate reaching it.  get_change is the same scan seeded with -inf.  A NaN or
// -inf never passes either strict compare, so both count as -inf in the scans.  The column sum of a wave is loaded 64 values at a
// time and added one after the other, in entry order, by every lane alike.
// All rounds are queued on one stream; the host waits once, at the end.
//
// so_apc_rows: the same loop from id-coded rows (cx <= cy, float64 weights, a taxon code per id code) -- `find_cluster -a apc -G A`.  The
// layout above is built on the device, without the entry list ever being written (its definition: find_cluster.apc_entry_columns()): genes
// numbered by first appearance, the taxa in use counted for the preference, pointers from the occurrences per gene, the entries in row
// order and the columns' entries in entry order from two stable radix sorts, short / long lists by flag / scan / compact; see "the layout
// from id-coded rows" below.  so_apc (layout prepared on the host) and so_apc_rows (on the device) feed one function, apc_queue_loop, which
// queues the four kernels above.  Only gene codes and labels are downloaded; the host waits three times (number of genes, list lengths, end).
#include "common.h"
#include "device_call.h"
#include "kernels.h"
#include "../../include/sohit.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace {

#define APC_LANE_MAX 32u   // longest row / column one lane walks alone
#define APC_TOO_MANY_GENES ": more than 2^24 genes (the reference keeps gene numbers in float32 and merges genes beyond that; not reproduced)"

struct ApcRowState {   // per gene, carried over all rounds
    double* m1;
    double* m2;
    double* d5;
    int* k1;
    int* lab;
};

// ---- one lane per row: the reference's loops, literally ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_apc_row_lane(const u32* __restrict__ rows, u32 nrows, const u32* __restrict__ rptr, const int* __restrict__ kcol,
                                                      const float* __restrict__ s, float* __restrict__ R, const float* __restrict__ A, ApcRowState g,
                                                      double damp, double beta, int do_change, int do_update) {
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t >= nrows) return;
    const u32 i = rows[t];
    const u32 b = rptr[i], e = rptr[i + 1];
    if (do_change) {
        double ras = -INFINITY;
        int lab = g.lab[i];
        for (u32 p = b; p < e; ++p) {
            const double ra = __dadd_rn((double)R[p], (double)A[p]);
            if (ras < ra) ras = ra, lab = kcol[p];
        }
        g.lab[i] = lab;
    }
    if (!do_update) return;
    double m1 = g.m1[i], m2 = g.m2[i];
    int k1 = g.k1[i];
    for (u32 p = b; p < e; ++p) {
        const double ra = __dadd_rn((double)R[p], (double)A[p]);
        if (m1 < ra) m1 = ra, k1 = kcol[p];
        else if (m2 < ra) m2 = ra;
    }
    g.m1[i] = m1, g.m2[i] = m2, g.k1[i] = k1;
    bool on_diag = false;
    double d5 = 0.;
    for (u32 p = b; p < e; ++p) {
        const int k = kcol[p];
        const double r = __dadd_rn((double)s[p], -(k != k1 ? m1 : m2));
        const double rn = __dadd_rn(__dmul_rn((double)R[p], damp), __dmul_rn(beta, r));
        R[p] = (float)rn;
        if ((u32)k == i) on_diag = true, d5 = rn;
    }
    if (on_diag) g.d5[i] = d5;
}

__device__ __forceinline__ double apc_max(double a, double b) { return a < b ? b : a; }   // b only when strictly above; never a NaN b

// inclusive prefix maximum over the lanes of a wave
__device__ __forceinline__ double apc_scan_max(double v, u32 lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const double u = __shfl_up(v, o);
        if (lane >= (u32)o) v = apc_max(u, v);
    }
    return v;
}

// ---- one wave per row ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_apc_row_wave(const u32* __restrict__ rows, u32 nrows, const u32* __restrict__ rptr, const int* __restrict__ kcol,
                                                     const float* __restrict__ s, float* __restrict__ R, const float* __restrict__ A, ApcRowState g,
                                                     double damp, double beta, int do_change, int do_update) {
    if (blockIdx.x >= nrows) return;
    const u32 i = rows[blockIdx.x];
    const u32 lane = threadIdx.x;
    const u32 b = rptr[i], e = rptr[i + 1];
    double ras = -INFINITY, m1 = 0., m2 = 0.;
    int lab = 0, k1 = 0;
    if (do_change) lab = g.lab[i];
    if (do_update) m1 = g.m1[i], m2 = g.m2[i], k1 = g.k1[i];
    for (u32 c = b; c < e; c += 64) {   // (wave-uniform bounds)
        const u32 p = c + lane;
        const bool have = p < e;
        double ra = -INFINITY;
        int k = 0;
        if (have) {
            ra = __dadd_rn((double)R[p], (double)A[p]);
            k = kcol[p];
            if (ra != ra) ra = -INFINITY;
        }
        const double inc = apc_scan_max(ra, lane);
        double before = __shfl_up(inc, 1);   // maximum of the lanes before this one
        if (lane == 0) before = -INFINITY;
        if (do_change) {
            const unsigned long long up = __ballot(have && ra > apc_max(ras, before));
            if (up) {
                const int last = 63 - __builtin_clzll(up);
                ras = __shfl(ra, last), lab = __shfl(k, last);
            }
        }
        if (do_update) {
            const bool updater = have && ra > apc_max(m1, before);
            const unsigned long long up = __ballot(updater);
            if (up) {
                const int last = 63 - __builtin_clzll(up);
                m1 = __shfl(ra, last), k1 = __shfl(k, last);
            }
            double cm = (have && !updater) ? ra : -INFINITY;   // the candidates for second place
            const double mine = cm;
            for (int o = 32; o > 0; o >>= 1) cm = apc_max(cm, __shfl_xor(cm, o));
            if (m2 < cm) {   // (the same on every lane: a maximum of the same 64 values, equal whatever the order -- +0 and -0 compare equal)
                const unsigned long long at = __ballot(have && !updater && mine == cm);
                m2 = __shfl(mine, __builtin_ctzll(at));   // the value of the FIRST candidate reaching the maximum, sign of zero included
            }
        }
    }
    if (do_change && lane == 0) g.lab[i] = lab;
    if (!do_update) return;
    if (lane == 0) g.m1[i] = m1, g.m2[i] = m2, g.k1[i] = k1;
    bool on_diag = false;
    double d5 = 0.;
    for (u32 c = b; c < e; c += 64) {
        const u32 p = c + lane;
        const bool have = p < e;
        int k = -1;
        double rn = 0.;
        if (have) {
            k = kcol[p];
            const double r = __dadd_rn((double)s[p], -(k != k1 ? m1 : m2));
            rn = __dadd_rn(__dmul_rn((double)R[p], damp), __dmul_rn(beta, r));
            R[p] = (float)rn;
        }
        const unsigned long long dg = __ballot(have && (u32)k == i);
        if (dg) on_diag = true, d5 = __shfl(rn, 63 - __builtin_clzll(dg));
    }
    if (on_diag && lane == 0) g.d5[i] = d5;
}

// update_A of one entry: column sum d4, the diagonal's unrounded R d5
__device__ __forceinline__ float apc_new_a(float a, float r32, bool off_diag, double d4, double d5, double damp, double beta) {
    const double an = __dmul_rn((double)a, damp);
    double add;
    if (off_diag) {
        const double r = (double)r32;
        const double x = __dadd_rn(__dadd_rn(d5, d4), -(r > 0. ? r : 0.));
        add = x < 0. ? x : 0.;
    } else {
        add = d4;
    }
    return (float)__dadd_rn(an, __dmul_rn(beta, add));
}

// ---- one lane per column ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_apc_col_lane(const u32* __restrict__ cols, u32 ncols, const u32* __restrict__ cptr, const u32* __restrict__ cpos,
                                                      const int* __restrict__ crow, const float* __restrict__ R, float* __restrict__ A,
                                                      const double* __restrict__ d5, double damp, double beta) {
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t >= ncols) return;
    const u32 k = cols[t];
    const u32 b = cptr[k], e = cptr[k + 1];
    double d4 = 0.;
    for (u32 q = b; q < e; ++q) {
        const double r = (double)R[cpos[q]];
        if ((u32)crow[q] != k && r > 0.) d4 = __dadd_rn(d4, r);   // (adding the 0 of max(0, r) leaves a sum that is never -0 as it is)
    }
    const double dk = d5[k];
    for (u32 q = b; q < e; ++q) {
        const u32 p = cpos[q];
        A[p] = apc_new_a(A[p], R[p], (u32)crow[q] != k, d4, dk, damp, beta);
    }
}

// ---- one wave per column ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_apc_col_wave(const u32* __restrict__ cols, u32 ncols, const u32* __restrict__ cptr, const u32* __restrict__ cpos,
                                                     const int* __restrict__ crow, const float* __restrict__ R, float* __restrict__ A,
                                                     const double* __restrict__ d5, double damp, double beta) {
    if (blockIdx.x >= ncols) return;
    const u32 k = cols[blockIdx.x];
    const u32 lane = threadIdx.x;
    const u32 b = cptr[k], e = cptr[k + 1];
    double d4 = 0.;
    for (u32 c = b; c < e; c += 64) {
        const u32 q = c + lane;
        double v = 0.;
        if (q < e) {
            const double r = (double)R[cpos[q]];
            if ((u32)crow[q] != k && r > 0.) v = r;
        }
        const u32 cnt = min(64u, e - c);
        for (u32 t = 0; t < cnt; ++t) d4 = __dadd_rn(d4, __shfl(v, (int)t));   // in entry order, the same on every lane
    }
    const double dk = d5[k];
    for (u32 q = b + lane; q < e; q += 64) {
        const u32 p = cpos[q];
        A[p] = apc_new_a(A[p], R[p], (u32)crow[q] != k, d4, dk, damp, beta);
    }
}

__global__ __launch_bounds__(256) void k_apc_iota(int* __restrict__ lab, u32 n) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) lab[i] = (int)i;
}

// the row / column layout of one call, on the device: what the host prepares in so_apc and the device in so_apc_rows
struct ApcLayout {
    const u32 *rptr, *cptr, *cpos, *rshort, *rlong, *cshort, *clong;
    const int *kcol, *crow;
    const float* s;
    u32 nrs, nrl, ncs, ncl;   // lengths of the four lists
};
struct ApcLoop {   // R, A (row order) and the per-gene state of the loop
    DevBuf<int> k1, lab;
    DevBuf<float> R, A;
    DevBuf<double> m1, m2, d5;
};

// all rounds of the loop over a prepared layout of D genes and N entries, queued on `st` (no host wait)
void apc_queue_loop(const ApcLayout& l, size_t D, size_t N, ApcLoop& b, double damp, int rounds, hipStream_t st) {
    b.R.ensure(N + 2), b.A.ensure(N + 2), b.m1.ensure(D + 2), b.m2.ensure(D + 2), b.d5.ensure(D + 2), b.k1.ensure(D + 2), b.lab.ensure(D + 2);
    HIP_CHECK(hipMemsetAsync(b.R.p, 0, (N + 2) * sizeof(float), st));
    HIP_CHECK(hipMemsetAsync(b.A.p, 0, (N + 2) * sizeof(float), st));
    HIP_CHECK(hipMemsetAsync(b.m1.p, 0, (D + 2) * sizeof(double), st));
    HIP_CHECK(hipMemsetAsync(b.m2.p, 0, (D + 2) * sizeof(double), st));
    HIP_CHECK(hipMemsetAsync(b.d5.p, 0, (D + 2) * sizeof(double), st));
    HIP_CHECK(hipMemsetAsync(b.k1.p, 0, (D + 2) * sizeof(int), st));
    if (D) hipLaunchKernelGGL(k_apc_iota, dim3((u32)((D + 255) / 256)), dim3(256), 0, st, b.lab.p, (u32)D);

    const ApcRowState g{b.m1.p, b.m2.p, b.d5.p, b.k1.p, b.lab.p};
    const double beta = 1. - damp;
    auto row_pass = [&](int do_change, int do_update) {
        if (l.nrs)
            hipLaunchKernelGGL(k_apc_row_lane, dim3((l.nrs + 255) / 256), dim3(256), 0, st, l.rshort, l.nrs, l.rptr, l.kcol, l.s, b.R.p, b.A.p, g, damp, beta, do_change,
                               do_update);
        if (l.nrl)
            hipLaunchKernelGGL(k_apc_row_wave, dim3(l.nrl), dim3(64), 0, st, l.rlong, l.nrl, l.rptr, l.kcol, l.s, b.R.p, b.A.p, g, damp, beta, do_change, do_update);
    };
    for (int it = 0; it < rounds; ++it) {
        row_pass(it > 0, 1);
        if (l.ncs) hipLaunchKernelGGL(k_apc_col_lane, dim3((l.ncs + 255) / 256), dim3(256), 0, st, l.cshort, l.ncs, l.cptr, l.cpos, l.crow, b.R.p, b.A.p, b.d5.p, damp, beta);
        if (l.ncl) hipLaunchKernelGGL(k_apc_col_wave, dim3(l.ncl), dim3(64), 0, st, l.clong, l.ncl, l.cptr, l.cpos, l.crow, b.R.p, b.A.p, b.d5.p, damp, beta);
    }
    if (rounds > 0) row_pass(1, 0);   // get_change of the last round
    HIP_CHECK(hipGetLastError());
}

// stable grouping of the entries by `key`: ptr[g] .. ptr[g + 1] = the entries of group g in entry order
void group_stable(const int32_t* key, size_t n, size_t groups, std::vector<u32>& ptr, std::vector<u32>& order) {
    ptr.assign(groups + 1, 0);
    for (size_t e = 0; e < n; ++e) ++ptr[(size_t)key[e] + 1];
    for (size_t g = 0; g < groups; ++g) ptr[g + 1] += ptr[g];
    order.resize(n);
    std::vector<u32> at(ptr.begin(), ptr.end() - 1);
    for (size_t e = 0; e < n; ++e) order[at[(size_t)key[e]]++] = (u32)e;
}

// the groups of at most / more than APC_LANE_MAX entries (empty ones: none)
void split_by_length(const std::vector<u32>& ptr, std::vector<u32>& shorts, std::vector<u32>& longs) {
    for (size_t g = 0; g + 1 < ptr.size(); ++g) {
        const u32 len = ptr[g + 1] - ptr[g];
        if (!len) continue;
        (len <= APC_LANE_MAX ? shorts : longs).push_back((u32)g);
    }
}

// ---- the layout from id-coded rows, on the device (so_apc_rows) ----------------------------------------------------------------------
// Rows come as id CODES (cx <= cy).  Genes are numbered by first appearance in cx0, cy0, cx1, ... as cnc.hip's plan numbers them
// (number_by_first_appearance, k_util.hip); the taxa of the first positions are flagged and counted for the preference.  The entry
// list is never written: entry e is
// (X_r, Y_r) for e = 2r, (Y_r, X_r) for e = 2r + 1 and (g, g) for e = 2 * rows + g, and every kernel below derives it from e.  A row of
// the layout holds one entry per occurrence of its gene in the rows and its preference entry, and so does its column: ONE array of
// pointers serves as rptr and cptr, one pair of lists as the short / long rows and columns.  A stable radix sort of (row of e, e) gives
// the entries in row order, a second one of (column of e, e) the columns' entries in entry order.  Integer atomics only.

// after the numbering (flag[p]: position p is its code's first): the taxon of such a code is in use; cnt[g] = the occurrences of gene g
__global__ __launch_bounds__(256) void k_apcr_count(const int* __restrict__ cx, const int* __restrict__ cy, u32 nr, const u32* __restrict__ flag,
                                                    const int* __restrict__ taxon_of_code, const int* __restrict__ X, const int* __restrict__ Y,
                                                    u32* __restrict__ taxflag, u32* __restrict__ cnt) {
    const size_t i = tid256();
    if (i >= nr) return;
    if (flag[2 * i]) atomicOr(&taxflag[taxon_of_code[cx[i]]], 1u);
    if (flag[2 * i + 1]) atomicOr(&taxflag[taxon_of_code[cy[i]]], 1u);
    atomicAdd(&cnt[X[i]], 1u);
    atomicAdd(&cnt[Y[i]], 1u);
}
// len[g] = cnt[g] + 1 (the preference entry), len[D] = 0 for the scan that ends the pointers; which list gene g goes to
__global__ __launch_bounds__(256) void k_apcr_len(const u32* __restrict__ cnt, u32 D, u32* __restrict__ len, u32* __restrict__ sflag, u32* __restrict__ lflag) {
    const size_t g = tid256();
    if (g > D) return;
    if (g == D) {
        len[g] = 0;
        return;
    }
    const u32 l = cnt[g] + 1u;
    len[g] = l, sflag[g] = l <= APC_LANE_MAX ? 1u : 0u, lflag[g] = l <= APC_LANE_MAX ? 0u : 1u;
}
__global__ __launch_bounds__(256) void k_apcr_lists(const u32* __restrict__ sflag, const u32* __restrict__ spos, const u32* __restrict__ lflag,
                                                    const u32* __restrict__ lpos, u32 D, u32* __restrict__ shorts, u32* __restrict__ longs) {
    const size_t g = tid256();
    if (g >= D) return;
    if (sflag[g]) shorts[spos[g]] = (u32)g;
    if (lflag[g]) longs[lpos[g]] = (u32)g;
}
// entry e of the list that is never written: its row and its column
__device__ __forceinline__ void apcr_entry(u32 e, u32 nr2, const int* __restrict__ X, const int* __restrict__ Y, int& row, int& col) {
    if (e < nr2) {
        const int x = X[e >> 1], y = Y[e >> 1];
        row = (e & 1) ? y : x, col = (e & 1) ? x : y;
    } else {
        row = col = (int)(e - nr2);
    }
}
template <bool BYCOL>
__global__ __launch_bounds__(256) void k_apcr_keys(const int* __restrict__ X, const int* __restrict__ Y, u32 nr2, u32 N, u64* __restrict__ key, u32* __restrict__ val) {
    const size_t e = tid256();
    if (e >= N) return;
    int row, col;
    apcr_entry((u32)e, nr2, X, Y, row, col);
    key[e] = (u64)(u32)(BYCOL ? col : row), val[e] = (u32)e;
}
// position p of the row order holds entry rorder[p]: its column, its score (one rounding of the float64 weight), and where the entry went
__global__ __launch_bounds__(256) void k_apcr_place(const int* __restrict__ X, const int* __restrict__ Y, const double* __restrict__ z, u32 nr2, u32 N,
                                                    const u32* __restrict__ rorder, float pref, u32* __restrict__ place, int* __restrict__ kcol,
                                                    float* __restrict__ s) {
    const size_t p = tid256();
    if (p >= N) return;
    const u32 e = rorder[p];
    int row, col;
    apcr_entry(e, nr2, X, Y, row, col);
    place[e] = (u32)p, kcol[p] = col, s[p] = e < nr2 ? (float)z[e >> 1] : pref;
}
__global__ __launch_bounds__(256) void k_apcr_cols(const int* __restrict__ X, const int* __restrict__ Y, u32 nr2, u32 N, const u32* __restrict__ corder,
                                                   const u32* __restrict__ place, u32* __restrict__ cpos, int* __restrict__ crow) {
    const size_t q = tid256();
    if (q >= N) return;
    const u32 e = corder[q];
    int row, col;
    apcr_entry(e, nr2, X, Y, row, col);
    cpos[q] = place[e], crow[q] = row;
}
// the tests' view: the entry list and the stores of the loop in ENTRY order
__global__ __launch_bounds__(256) void k_apcr_entries(const int* __restrict__ X, const int* __restrict__ Y, u32 nr2, u32 N, const u32* __restrict__ place,
                                                      const float* __restrict__ s, const float* __restrict__ R, const float* __restrict__ A, int* __restrict__ orow,
                                                      int* __restrict__ ocol, float* __restrict__ os, float* __restrict__ o_r, float* __restrict__ o_a) {
    const size_t e = tid256();
    if (e >= N) return;
    int row, col;
    apcr_entry((u32)e, nr2, X, Y, row, col);
    const u32 p = place[e];
    orow[e] = row, ocol[e] = col, os[e] = s[p], o_r[e] = R[p], o_a[e] = A[p];
}

thread_local std::string g_apc_err;

auto slots(so_apc_result* r) { return result_slots(&r->labels, &r->r, &r->a); }
auto slots(so_apc_rows_result* r) { return result_slots(&r->gene_code, &r->labels, &r->row, &r->col, &r->score, &r->r, &r->a); }

}  // namespace

extern "C" {

const char* so_apc_last_error(void) { return g_apc_err.c_str(); }

void so_apc_free(so_apc_result* r) {
    if (r) release_slots(r, slots(r));
}

int so_apc(int device, int64_t n_genes, int64_t n_entries, const int32_t* row, const int32_t* col, const float* score, double damp, int32_t rounds,
           so_apc_result* out) {
    return guarded_call(g_apc_err, out, so_apc_free, [&] {
        if (!out) throw SoError("so_apc: result pointer is NULL");
        memset(out, 0, sizeof *out);
        if (n_genes < 0 || n_entries < 0 || rounds < 0 || (n_entries > 0 && (!row || !col || !score))) throw SoError("so_apc: bad arguments");
        if (n_genes > (1ll << 24))
            throw SoError("so_apc" APC_TOO_MANY_GENES);
        if (n_entries > 0x7FFFFFF0ll) throw SoError("so_apc: edge list too large for 32-bit positions");
        const size_t D = (size_t)n_genes, N = (size_t)n_entries;
        for (size_t e = 0; e < N; ++e)
            if (row[e] < 0 || row[e] >= n_genes || col[e] < 0 || col[e] >= n_genes) throw SoError("so_apc: entry " + std::to_string(e) + " names a gene outside 0 .. n_genes - 1");
        check_device("so_apc", device);

        // rows: the entries in row order; columns: positions (in row order) and rows of each column's entries, in entry order
        std::vector<u32> rptr, rorder, cptr, corder;
        group_stable(row, N, D, rptr, rorder);
        group_stable(col, N, D, cptr, corder);
        std::vector<u32> place(N), cpos(N);
        std::vector<int> kcol(N), crow(N);
        std::vector<float> sc(N);
        for (size_t p = 0; p < N; ++p) place[rorder[p]] = (u32)p, kcol[p] = col[rorder[p]], sc[p] = score[rorder[p]];
        for (size_t q = 0; q < N; ++q) cpos[q] = place[corder[q]], crow[q] = row[corder[q]];
        std::vector<u32> rshort, rlong, cshort, clong;
        split_by_length(rptr, rshort, rlong);
        split_by_length(cptr, cshort, clong);

        DeviceCall call(device);
        const hipStream_t st = call.st;
        DevBuf<u32> d_rptr, d_cptr, d_cpos, d_rshort, d_rlong, d_cshort, d_clong;
        DevBuf<int> d_kcol, d_crow;
        DevBuf<float> d_s;
        auto up = [&](auto& d, const auto& h) { upload(d, h.data(), h.size(), st); };
        up(d_rptr, rptr), up(d_cptr, cptr), up(d_cpos, cpos), up(d_kcol, kcol), up(d_crow, crow), up(d_s, sc);
        up(d_rshort, rshort), up(d_rlong, rlong), up(d_cshort, cshort), up(d_clong, clong);
        const ApcLayout lay{d_rptr.p, d_cptr.p, d_cpos.p, d_rshort.p, d_rlong.p, d_cshort.p, d_clong.p, d_kcol.p, d_crow.p, d_s.p,
                            (u32)rshort.size(), (u32)rlong.size(), (u32)cshort.size(), (u32)clong.size()};
        ApcLoop lp;
        apc_queue_loop(lay, D, N, lp, damp, rounds, st);
        HIP_CHECK(hipStreamSynchronize(st));

        std::vector<int> lab(D);
        std::vector<float> hr(N), ha(N);
        if (D) HIP_CHECK(hipMemcpy(lab.data(), lp.lab.p, D * sizeof(int), hipMemcpyDeviceToHost));
        if (N) {
            HIP_CHECK(hipMemcpy(hr.data(), lp.R.p, N * sizeof(float), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(ha.data(), lp.A.p, N * sizeof(float), hipMemcpyDeviceToHost));
        }
        out->n_genes = n_genes, out->n_entries = n_entries, out->rounds = rounds;
        out->labels = host_array<int64_t>("so_apc", D), out->r = host_array<float>("so_apc", N), out->a = host_array<float>("so_apc", N);
        for (size_t i = 0; i < D; ++i) out->labels[i] = lab[i];
        for (size_t e = 0; e < N; ++e) out->r[e] = hr[place[e]], out->a[e] = ha[place[e]];   // back to entry order
    });
}

void so_apc_rows_free(so_apc_rows_result* r) {
    if (r) release_slots(r, slots(r));
}

int so_apc_rows(int device, int64_t n_codes, int64_t n_rows, const int32_t* cx, const int32_t* cy, const double* z, const int32_t* taxon_of_code,
                int64_t n_taxa, double damp, int32_t rounds, int32_t flags, so_apc_rows_result* out) {
    return guarded_call(g_apc_err, out, so_apc_rows_free, [&] {
        if (!out) throw SoError("so_apc_rows: result pointer is NULL");
        memset(out, 0, sizeof *out);
        if (n_codes < 0 || n_rows < 0 || n_taxa < 0 || rounds < 0 || (n_rows > 0 && (!cx || !cy || !z)) || (n_codes > 0 && !taxon_of_code))
            throw SoError("so_apc_rows: bad arguments");
        if (n_codes >= (1ll << 31) || n_rows >= (1ll << 31) || n_taxa >= (1ll << 31))
            throw SoError("so_apc_rows: 2^31 codes, rows or taxa and more are not served (32-bit codes and row indices)");
        if (2 * n_rows + n_codes > 0x7FFFFFF0ll) throw SoError("so_apc_rows: edge list too large for 32-bit positions");
        const size_t N1 = (size_t)n_rows, C = (size_t)n_codes;
        for (size_t c = 0; c < C; ++c)
            if (taxon_of_code[c] < 0 || taxon_of_code[c] >= n_taxa) throw SoError("so_apc_rows: code " + std::to_string(c) + " names a taxon outside 0 .. n_taxa - 1");
        for (size_t i = 0; i < N1; ++i) {
            if (cx[i] < 0 || cx[i] >= n_codes || cy[i] < 0 || cy[i] >= n_codes)
                throw SoError("so_apc_rows: row " + std::to_string(i) + " names a code outside 0 .. n_codes - 1");
            if (cx[i] > cy[i]) throw SoError("so_apc_rows: row " + std::to_string(i) + " has cx > cy (fc2mat drops such rows before anything is numbered)");
        }
        const char* const who = "so_apc_rows";
        check_device(who, device);
        out->n_codes = n_codes, out->n_rows = n_rows, out->rounds = rounds;
        const bool want_entries = (flags & 1) != 0;
        if (!N1) {   // no row: no gene, no entry, nothing to launch
            out->gene_code = host_array<int32_t>(who, 0), out->labels = host_array<int64_t>(who, 0);
            if (want_entries)
                out->row = host_array<int32_t>(who, 0), out->col = host_array<int32_t>(who, 0), out->score = host_array<float>(who, 0), out->r = host_array<float>(who, 0),
                out->a = host_array<float>(who, 0);
            return;
        }

        DeviceCall call(device);
        const hipStream_t st = call.st;
        const u32 nr = (u32)N1, nr2 = 2 * nr;
        const size_t N2 = 2 * N1, T = (size_t)n_taxa, Dmax = std::min(C, N2);

        // genes numbered by first appearance, the taxa in use, the occurrences of every gene
        DevBuf<int> d_cx, d_cy, d_tax, d_x, d_y, d_gene;
        DevBuf<double> d_z;
        DevBuf<u32> d_first, d_flag, d_rank, d_taxflag, d_taxpos, d_cnt, d_tmp_a, d_tmp_b, d_tmp_c;
        d_cx.ensure(N1 + 2), d_cy.ensure(N1 + 2), d_z.ensure(N1 + 2), d_tax.ensure(C + 2), d_x.ensure(N1 + 2), d_y.ensure(N1 + 2), d_first.ensure(C + 2);
        d_flag.ensure(N2 + 2), d_rank.ensure(N2 + 2), d_taxflag.ensure(T + 2), d_taxpos.ensure(T + 2), d_gene.ensure(Dmax + 2), d_cnt.ensure(Dmax + 2);
        const size_t tmp_elems = scan_u32_temp_elems(std::max(N2, T) + 1) + 8;
        d_tmp_a.ensure(tmp_elems), d_tmp_b.ensure(tmp_elems), d_tmp_c.ensure(tmp_elems);
        HIP_CHECK(hipMemcpyAsync(d_cx.p, cx, N1 * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d_cy.p, cy, N1 * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d_z.p, z, N1 * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d_tax.p, taxon_of_code, C * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemsetAsync(d_taxflag.p, 0, T * sizeof(u32), st));
        HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, (Dmax + 2) * sizeof(u32), st));
        const u32* d_ngenes = number_by_first_appearance(d_cx.p, d_cy.p, nr, (u32)C, d_first.p, d_flag.p, d_rank.p, d_tmp_a.p, d_x.p, d_y.p, d_gene.p, st);
        hipLaunchKernelGGL(k_apcr_count, grid256(N1), dim3(256), 0, st, d_cx.p, d_cy.p, nr, d_flag.p, d_tax.p, d_x.p, d_y.p, d_taxflag.p, d_cnt.p);
        const u32* d_ntaxa = scan_u32(d_taxflag.p, d_taxpos.p, T, false, d_tmp_b.p, st);
        HIP_CHECK(hipGetLastError());
        u32 n = 0, ntax = 0;
        call.read(d_ngenes, n, d_ntaxa, ntax);
        if (n < 1 || n > Dmax || ntax < 1 || ntax > T || ntax > n)
            throw SoError("so_apc_rows: internal error: " + std::to_string(n) + " genes of " + std::to_string(ntax) + " taxa in " + std::to_string(nr) + " rows");
        if (n > (1u << 24)) throw SoError("so_apc_rows" APC_TOO_MANY_GENES);
        const size_t D = n, N = N2 + D;
        const u32 ne = (u32)N;
        const float pref = (float)(-20.0 * (double)ntax);

        // pointers (rows and columns alike) and the short / long lists
        DevBuf<u32> d_len, d_ptr, d_sflag, d_lflag, d_spos, d_lpos, d_short, d_long;
        d_len.ensure(D + 3), d_ptr.ensure(D + 3), d_sflag.ensure(D + 2), d_lflag.ensure(D + 2), d_spos.ensure(D + 2), d_lpos.ensure(D + 2), d_short.ensure(D + 2),
            d_long.ensure(D + 2);
        hipLaunchKernelGGL(k_apcr_len, grid256(D + 1), dim3(256), 0, st, d_cnt.p, n, d_len.p, d_sflag.p, d_lflag.p);
        scan_u32(d_len.p, d_ptr.p, D + 1, false, d_tmp_a.p, st);
        const u32* d_nshort = scan_u32(d_sflag.p, d_spos.p, D, false, d_tmp_b.p, st);
        const u32* d_nlong = scan_u32(d_lflag.p, d_lpos.p, D, false, d_tmp_c.p, st);
        hipLaunchKernelGGL(k_apcr_lists, grid256(D), dim3(256), 0, st, d_sflag.p, d_spos.p, d_lflag.p, d_lpos.p, n, d_short.p, d_long.p);

        // the entries in row order, the columns' entries in entry order
        const int bits = ceil_log2((u64)D);
        DevBuf<u64> d_key, d_skey;
        DevBuf<u32> d_val, d_order, d_place, d_cpos;
        DevBuf<int> d_kcol, d_crow;
        DevBuf<float> d_s;
        DevBuf<u8> d_sort_tmp;
        d_key.ensure(N + 2), d_skey.ensure(N + 2), d_val.ensure(N + 2), d_order.ensure(N + 2), d_place.ensure(N + 2), d_cpos.ensure(N + 2), d_kcol.ensure(N + 2);
        d_crow.ensure(N + 2), d_s.ensure(N + 2), d_sort_tmp.ensure(sort_pairs_u64_u32_temp_bytes(N, bits) + 256);
        hipLaunchKernelGGL(k_apcr_keys<false>, grid256(N), dim3(256), 0, st, d_x.p, d_y.p, nr2, ne, d_key.p, d_val.p);
        sort_pairs_u64_u32(d_sort_tmp.p, d_sort_tmp.cap, d_key.p, d_skey.p, d_val.p, d_order.p, N, bits, st);   // stable: entry order inside a row
        hipLaunchKernelGGL(k_apcr_place, grid256(N), dim3(256), 0, st, d_x.p, d_y.p, d_z.p, nr2, ne, d_order.p, pref, d_place.p, d_kcol.p, d_s.p);
        hipLaunchKernelGGL(k_apcr_keys<true>, grid256(N), dim3(256), 0, st, d_x.p, d_y.p, nr2, ne, d_key.p, d_val.p);
        sort_pairs_u64_u32(d_sort_tmp.p, d_sort_tmp.cap, d_key.p, d_skey.p, d_val.p, d_order.p, N, bits, st);   // stable: entry order inside a column
        hipLaunchKernelGGL(k_apcr_cols, grid256(N), dim3(256), 0, st, d_x.p, d_y.p, nr2, ne, d_order.p, d_place.p, d_cpos.p, d_crow.p);
        HIP_CHECK(hipGetLastError());
        u32 nshort = 0, nlong = 0;
        call.read(d_nshort, nshort, d_nlong, nlong);
        if ((size_t)nshort + nlong != D) throw SoError("so_apc_rows: internal error: " + std::to_string(nshort) + " short and " + std::to_string(nlong) + " long rows of " + std::to_string(n));

        const ApcLayout lay{d_ptr.p, d_ptr.p, d_cpos.p, d_short.p, d_long.p, d_short.p, d_long.p, d_kcol.p, d_crow.p, d_s.p, nshort, nlong, nshort, nlong};
        ApcLoop lp;
        apc_queue_loop(lay, D, N, lp, damp, rounds, st);

        out->n_genes = n, out->n_entries = (int64_t)N, out->n_taxa_used = ntax;
        out->gene_code = host_array<int32_t>(who, D), out->labels = host_array<int64_t>(who, D);
        std::vector<int> lab(D);
        HIP_CHECK(hipMemcpyAsync(out->gene_code, d_gene.p, D * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(lab.data(), lp.lab.p, D * sizeof(int), hipMemcpyDeviceToHost, st));
        DevBuf<int> d_orow, d_ocol;
        DevBuf<float> d_os, d_or, d_oa;
        if (want_entries) {
            out->row = host_array<int32_t>(who, N), out->col = host_array<int32_t>(who, N), out->score = host_array<float>(who, N), out->r = host_array<float>(who, N), out->a = host_array<float>(who, N);
            d_orow.ensure(N + 2), d_ocol.ensure(N + 2), d_os.ensure(N + 2), d_or.ensure(N + 2), d_oa.ensure(N + 2);
            hipLaunchKernelGGL(k_apcr_entries, grid256(N), dim3(256), 0, st, d_x.p, d_y.p, nr2, ne, d_place.p, d_s.p, lp.R.p, lp.A.p, d_orow.p, d_ocol.p, d_os.p, d_or.p,
                               d_oa.p);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(out->row, d_orow.p, N * sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(out->col, d_ocol.p, N * sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(out->score, d_os.p, N * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(out->r, d_or.p, N * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(out->a, d_oa.p, N * sizeof(float), hipMemcpyDeviceToHost, st));
        }
        call.wait();
        for (size_t i = 0; i < D; ++i) out->labels[i] = lab[i];
        out->waits = call.waits;
    });
}

}  // extern "C"
