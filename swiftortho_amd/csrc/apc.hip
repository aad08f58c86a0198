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
#include "common.h"
#include "../../include/sohit.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace {

#define APC_LANE_MAX 32u   // longest row / column one lane walks alone

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

template <class T>
void upload(DevBuf<T>& d, const std::vector<T>& h) {
    d.ensure(h.size() + 2);
    if (!h.empty()) HIP_CHECK(hipMemcpy(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
}

thread_local std::string g_apc_err;

}  // namespace

extern "C" {

const char* so_apc_last_error(void) { return g_apc_err.c_str(); }

void so_apc_free(so_apc_result* r) {
    if (!r) return;
    free(r->labels), free(r->r), free(r->a);
    memset(r, 0, sizeof *r);
}

int so_apc(int device, int64_t n_genes, int64_t n_entries, const int32_t* row, const int32_t* col, const float* score, double damp, int32_t rounds,
           so_apc_result* out) {
    try {
        if (!out) throw SoError("so_apc: result pointer is NULL");
        memset(out, 0, sizeof *out);
        if (n_genes < 0 || n_entries < 0 || rounds < 0 || (n_entries > 0 && (!row || !col || !score))) throw SoError("so_apc: bad arguments");
        if (n_genes > (1ll << 24))
            throw SoError("so_apc: more than 2^24 genes (the reference keeps gene numbers in float32 and merges genes beyond that; not reproduced)");
        if (n_entries > 0x7FFFFFF0ll) throw SoError("so_apc: edge list too large for 32-bit positions");
        const size_t D = (size_t)n_genes, N = (size_t)n_entries;
        for (size_t e = 0; e < N; ++e)
            if (row[e] < 0 || row[e] >= n_genes || col[e] < 0 || col[e] >= n_genes) throw SoError("so_apc: entry " + std::to_string(e) + " names a gene outside 0 .. n_genes - 1");
        int nd = 0;
        if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) throw SoError("so_apc: no HIP device available (libsohit has no CPU fallback)");
        if (device < 0 || device >= nd) throw SoError("so_apc: device index out of range");
        HIP_CHECK(hipSetDevice(device));
        Tune tn;   // no context: the switches are read per call
        tn.read();
        const PoisonScope poison((int)tn.poison);

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

        hipStream_t st = nullptr;
        HIP_CHECK(hipStreamCreate(&st));
        struct Guard {
            hipStream_t s;
            ~Guard() { (void)hipStreamSynchronize(s), (void)hipStreamDestroy(s); }
        } guard{st};
        DevBuf<u32> d_rptr, d_cptr, d_cpos, d_rshort, d_rlong, d_cshort, d_clong;
        DevBuf<int> d_kcol, d_crow, d_k1, d_lab;
        DevBuf<float> d_s, d_R, d_A;
        DevBuf<double> d_m1, d_m2, d_d5;
        upload(d_rptr, rptr), upload(d_cptr, cptr), upload(d_cpos, cpos), upload(d_kcol, kcol), upload(d_crow, crow), upload(d_s, sc);
        upload(d_rshort, rshort), upload(d_rlong, rlong), upload(d_cshort, cshort), upload(d_clong, clong);
        d_R.ensure(N + 2), d_A.ensure(N + 2), d_m1.ensure(D + 2), d_m2.ensure(D + 2), d_d5.ensure(D + 2), d_k1.ensure(D + 2), d_lab.ensure(D + 2);
        HIP_CHECK(hipMemsetAsync(d_R.p, 0, (N + 2) * sizeof(float), st));
        HIP_CHECK(hipMemsetAsync(d_A.p, 0, (N + 2) * sizeof(float), st));
        HIP_CHECK(hipMemsetAsync(d_m1.p, 0, (D + 2) * sizeof(double), st));
        HIP_CHECK(hipMemsetAsync(d_m2.p, 0, (D + 2) * sizeof(double), st));
        HIP_CHECK(hipMemsetAsync(d_d5.p, 0, (D + 2) * sizeof(double), st));
        HIP_CHECK(hipMemsetAsync(d_k1.p, 0, (D + 2) * sizeof(int), st));
        if (D) hipLaunchKernelGGL(k_apc_iota, dim3((u32)((D + 255) / 256)), dim3(256), 0, st, d_lab.p, (u32)D);

        const ApcRowState g{d_m1.p, d_m2.p, d_d5.p, d_k1.p, d_lab.p};
        const double beta = 1. - damp;
        const u32 nrs = (u32)rshort.size(), nrl = (u32)rlong.size(), ncs = (u32)cshort.size(), ncl = (u32)clong.size();
        auto row_pass = [&](int do_change, int do_update) {
            if (nrs)
                hipLaunchKernelGGL(k_apc_row_lane, dim3((nrs + 255) / 256), dim3(256), 0, st, d_rshort.p, nrs, d_rptr.p, d_kcol.p, d_s.p, d_R.p, d_A.p, g, damp, beta,
                                   do_change, do_update);
            if (nrl)
                hipLaunchKernelGGL(k_apc_row_wave, dim3(nrl), dim3(64), 0, st, d_rlong.p, nrl, d_rptr.p, d_kcol.p, d_s.p, d_R.p, d_A.p, g, damp, beta, do_change,
                                   do_update);
        };
        for (int it = 0; it < rounds; ++it) {
            row_pass(it > 0, 1);
            if (ncs) hipLaunchKernelGGL(k_apc_col_lane, dim3((ncs + 255) / 256), dim3(256), 0, st, d_cshort.p, ncs, d_cptr.p, d_cpos.p, d_crow.p, d_R.p, d_A.p, d_d5.p, damp, beta);
            if (ncl) hipLaunchKernelGGL(k_apc_col_wave, dim3(ncl), dim3(64), 0, st, d_clong.p, ncl, d_cptr.p, d_cpos.p, d_crow.p, d_R.p, d_A.p, d_d5.p, damp, beta);
        }
        if (rounds > 0) row_pass(1, 0);   // get_change of the last round
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));

        std::vector<int> lab(D);
        std::vector<float> hr(N), ha(N);
        if (D) HIP_CHECK(hipMemcpy(lab.data(), d_lab.p, D * sizeof(int), hipMemcpyDeviceToHost));
        if (N) {
            HIP_CHECK(hipMemcpy(hr.data(), d_R.p, N * sizeof(float), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(ha.data(), d_A.p, N * sizeof(float), hipMemcpyDeviceToHost));
        }
        out->n_genes = n_genes, out->n_entries = n_entries, out->rounds = rounds;
        out->labels = (int64_t*)malloc((D ? D : 1) * sizeof(int64_t));
        out->r = (float*)malloc((N ? N : 1) * sizeof(float));
        out->a = (float*)malloc((N ? N : 1) * sizeof(float));
        if (!out->labels || !out->r || !out->a) {
            so_apc_free(out);
            throw SoError("so_apc: out of host memory");
        }
        for (size_t i = 0; i < D; ++i) out->labels[i] = lab[i];
        for (size_t e = 0; e < N; ++e) out->r[e] = hr[place[e]], out->a[e] = ha[place[e]];   // back to entry order
        g_apc_err.clear();
        return 0;
    } catch (const std::exception& e) {
        g_apc_err = e.what();
        return 1;
    }
}

}  // extern "C"
