// cnc.hip -- the component stage of `find_cluster -a mcl` on the device: the first half of SwiftOrtho's bin/find_cluster.py `cnc`
// (1470-1590) as swiftortho_amd/find_cluster.py `group_numbers()` restates it.  Every gene is linked to its best-scoring neighbours,
// the connected components of those links are numbered (level 1), components joined by any row whose two component numbers are
// non-zero are merged and numbered (level 2), and a row is kept when both ends carry the same level-2 number and that number is not 0.
//
// The reference's orders look sequential -- `popitem()`, networkx insertion order, components numbered by their first node -- and
// reduce to a closed form without an ordered traversal (genes are numbered 0 .. n-1 by first appearance):
//   best[g]   the largest weight over the rows that touch g; a row is a TIE ROW when its weight equals best[x] or best[y];
//   level 1   the connected components of the tie rows.  The tie pairs are inserted for the genes in descending order, so a component
//             is first reached at its largest gene: comp1[g] = number of components whose largest gene exceeds that of g's component
//             (component 0 holds gene n-1);
//   level 2   the rows with comp1[x] != 0 and comp1[y] != 0 join their two components (a row inside one component makes it a node);
//             a level-2 component's number is the rank, in file order, of the first such row that touches it; the genes of component 0
//             and of components no such row touches get -1;
//   keep[i]   grp[x] == grp[y] and that value is not 0 (the -1 pool is kept, level-2 group 0 is dropped).
//
// Kernels.  All results are integers and every atomic is an integer max or min, so each fixed point is unique and nothing depends on
// the order in which lanes arrive; every dependency is a launch boundary on the call's one stream, no kernel waits for another
// workgroup.
//   k_cnc_best   atomicMax of an order-preserving 64-bit image of the weight at both ends (-0.0 counts as +0.0, as numpy's == does;
//                +-inf are ordinary values; a NaN is refused on the host before anything is launched)
//   k_cnc_tie    the tie flag of every row
//   k_cnc_hook<1> + k_cnc_jump, per sweep: a node's label is a node of its own component that is not smaller than itself.  A row raises
//                the labels of its two ends, and of the smaller of their two labels, to the larger label (max-label hooking); then every
//                node follows its label's labels up to CNC_JUMP steps (pointer jumping; the labels rise strictly along the way, so the
//                walk ends whatever other lanes store meanwhile).  Either kernel raises one `changed` word when it moved a label; the
//                host reads that word per sweep and stops at the first sweep that leaves it 0: then both ends of every row agree and
//                every label is its own label, i.e. the largest node of the component.  A sweep carries the largest label at least one
//                row further, so n + 2 sweeps always suffice; passing that cap is reported as an error.
//   k_cnc_roots, scan_u32, k_cnc_number   roots = the genes that are their own label; comp1[g] = roots - 1 - (roots below lab[g])
//   k_cnc_hook<2> + k_cnc_jump   the same sweeps over the comp1 numbers, for the rows whose two numbers are non-zero
//   k_cnc_first  atomicMin of the row index at the final root of every such row;  k_cnc_firstflag  the rows that are a root's first row;
//   scan_u32 over the rows;  k_cnc_grp  grp of a gene = the scan value at the first row of its component's root, or -1;  k_cnc_keep.
// Labels are read with plain loads while other lanes raise them, and a load may return a value another lane (or another XCD's L2) has
// already replaced: any value a label ever held is a node of the same component that is not smaller than its owner, so a stale one only
// makes a sweep do less, and whoever replaced it has raised `changed`, so the host runs another sweep.  The confirming sweep stores
// nothing and therefore reads nothing stale.  How many sweeps a level takes can differ between two runs of the same input; the arrays
// cannot.
#include "common.h"
#include "kernels.h"
#include "../../include/sohit.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace {

#define CNC_JUMP 32          // label steps one lane follows per sweep
#define CNC_NONE 0xFFFFFFFFu   // no row yet (row indices stay below 2^31)

// doubles (no NaN) -> u64 that order the same way; -0.0 and +0.0 share one image
__device__ __forceinline__ u64 cnc_image(double z) {
    if (z == 0.) z = 0.;
    const u64 b = (u64)__double_as_longlong(z);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ __launch_bounds__(256) void k_cnc_best(const int* __restrict__ x, const int* __restrict__ y, const double* __restrict__ z, u32 nr,
                                                  unsigned long long* __restrict__ best) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nr) return;
    const u64 w = cnc_image(z[i]);
    atomicMax(&best[x[i]], (unsigned long long)w);
    atomicMax(&best[y[i]], (unsigned long long)w);
}

__global__ __launch_bounds__(256) void k_cnc_tie(const int* __restrict__ x, const int* __restrict__ y, const double* __restrict__ z, u32 nr,
                                                 const unsigned long long* __restrict__ best, u8* __restrict__ tie) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nr) return;
    const u64 w = cnc_image(z[i]);
    tie[i] = (w == best[x[i]] || w == best[y[i]]) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_cnc_iota(u32* __restrict__ lab, u32 n) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) lab[i] = i;
}

// LEVEL 1: nodes = genes, rows = the tie rows;  LEVEL 2: nodes = comp1 numbers, rows = those whose two numbers are non-zero
template <int LEVEL>
__device__ __forceinline__ bool cnc_row_nodes(const int* __restrict__ x, const int* __restrict__ y, const u8* __restrict__ tie, const u32* __restrict__ comp1,
                                              u32 i, u32& u, u32& v) {
    if (LEVEL == 1) {
        if (!tie[i]) return false;
        u = (u32)x[i], v = (u32)y[i];
        return true;
    }
    u = comp1[x[i]], v = comp1[y[i]];
    return u != 0 && v != 0;
}

template <int LEVEL>
__global__ __launch_bounds__(256) void k_cnc_hook(const int* __restrict__ x, const int* __restrict__ y, u32 nr, const u8* __restrict__ tie,
                                                  const u32* __restrict__ comp1, u32* __restrict__ lab, u32* __restrict__ changed) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nr) return;
    u32 u, v;
    if (!cnc_row_nodes<LEVEL>(x, y, tie, comp1, i, u, v)) return;
    const u32 lu = lab[u], lv = lab[v];
    if (lu == lv) return;
    const u32 hi = lu > lv ? lu : lv, lo = lu > lv ? lv : lu;
    bool moved = atomicMax(&lab[u], hi) < hi;
    moved |= atomicMax(&lab[v], hi) < hi;
    moved |= atomicMax(&lab[lo], hi) < hi;
    if (moved) *changed = 1u;
}

__global__ __launch_bounds__(256) void k_cnc_jump(u32* __restrict__ lab, u32 n, u32* __restrict__ changed) {
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n) return;
    const u32 l0 = lab[g];
    u32 l = l0;
    for (int s = 0; s < CNC_JUMP; ++s) {
        const u32 nl = lab[l];
        if (nl == l) break;
        l = nl;
    }
    if (l != l0) lab[g] = l, *changed = 1u;   // (only this lane stores lab[g] in this kernel)
}

__global__ __launch_bounds__(256) void k_cnc_roots(const u32* __restrict__ lab, u32 n, u32* __restrict__ root) {
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    if (g < n) root[g] = lab[g] == g ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_cnc_number(const u32* __restrict__ lab, const u32* __restrict__ below, const u32* __restrict__ roots, u32 n,
                                                    u32* __restrict__ comp1) {
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    if (g < n) comp1[g] = *roots - 1u - below[lab[g]];
}

__global__ __launch_bounds__(256) void k_cnc_first(const int* __restrict__ x, const int* __restrict__ y, u32 nr, const u32* __restrict__ comp1,
                                                   const u32* __restrict__ lab2, u32* __restrict__ first) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nr) return;
    u32 u, v;
    if (!cnc_row_nodes<2>(x, y, nullptr, comp1, i, u, v)) return;
    atomicMin(&first[lab2[u]], i);
}

__global__ __launch_bounds__(256) void k_cnc_firstflag(const int* __restrict__ x, const int* __restrict__ y, u32 nr, const u32* __restrict__ comp1,
                                                       const u32* __restrict__ lab2, const u32* __restrict__ first, u32* __restrict__ flag) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nr) return;
    u32 u, v;
    flag[i] = (cnc_row_nodes<2>(x, y, nullptr, comp1, i, u, v) && first[lab2[u]] == i) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_cnc_grp(const u32* __restrict__ comp1, const u32* __restrict__ lab2, const u32* __restrict__ first,
                                                 const u32* __restrict__ rank, u32 n, int* __restrict__ grp) {
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n) return;
    const u32 c = comp1[g];
    int r = -1;
    if (c != 0) {
        const u32 f = first[lab2[c]];
        if (f != CNC_NONE) r = (int)rank[f];
    }
    grp[g] = r;
}

__global__ __launch_bounds__(256) void k_cnc_keep(const int* __restrict__ x, const int* __restrict__ y, u32 nr, const int* __restrict__ grp, u8* __restrict__ keep) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nr) return;
    const int a = grp[x[i]], b = grp[y[i]];
    keep[i] = (a == b && a != 0) ? 1 : 0;
}

inline dim3 cnc_grid(u32 n) { return dim3((n + 255u) / 256u); }

// hook + jump until a sweep moves no label; -> sweeps run, the confirming one included
template <int LEVEL>
int cnc_sweeps(const int* x, const int* y, u32 nr, const u8* tie, const u32* comp1, u32* lab, u32 nodes, u32* changed, hipStream_t st) {
    const u64 cap = (u64)nodes + 2;
    for (u64 s = 1; s <= cap; ++s) {
        HIP_CHECK(hipMemsetAsync(changed, 0, sizeof(u32), st));
        hipLaunchKernelGGL(k_cnc_hook<LEVEL>, cnc_grid(nr), dim3(256), 0, st, x, y, nr, tie, comp1, lab, changed);
        hipLaunchKernelGGL(k_cnc_jump, cnc_grid(nodes), dim3(256), 0, st, lab, nodes, changed);
        u32 moved = 0;
        HIP_CHECK(hipMemcpyAsync(&moved, changed, sizeof(u32), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (!moved) return (int)s;
    }
    throw SoError("so_cnc_groups: the level-" + std::to_string(LEVEL) + " labels still moved after " + std::to_string(cap) + " sweeps (nodes + 2): no result");
}

thread_local std::string g_cnc_err;

}  // namespace

extern "C" {

const char* so_cnc_last_error(void) { return g_cnc_err.c_str(); }

void so_cnc_free(so_cnc_result* r) {
    if (!r) return;
    free(r->comp1), free(r->grp), free(r->keep);
    memset(r, 0, sizeof *r);
}

int so_cnc_groups(int device, int64_t n_genes, int64_t n_rows, const int32_t* x, const int32_t* y, const double* z, so_cnc_result* out) {
    try {
        if (!out) throw SoError("so_cnc_groups: result pointer is NULL");
        memset(out, 0, sizeof *out);
        if (n_genes < 0 || n_rows < 0 || (n_rows > 0 && (!x || !y || !z))) throw SoError("so_cnc_groups: bad arguments");
        if (n_genes >= (1ll << 31) || n_rows >= (1ll << 31)) throw SoError("so_cnc_groups: 2^31 genes or rows and more are not served (32-bit labels and row indices)");
        const size_t D = (size_t)n_genes, N = (size_t)n_rows;
        {
            std::vector<u8> seen(N ? D : 0, 0);
            for (size_t i = 0; i < N; ++i) {
                if (x[i] < 0 || x[i] >= n_genes || y[i] < 0 || y[i] >= n_genes)
                    throw SoError("so_cnc_groups: row " + std::to_string(i) + " names a gene outside 0 .. n_genes - 1");
                if (z[i] != z[i]) throw SoError("so_cnc_groups: row " + std::to_string(i) + " has a NaN weight (numpy's answer to it has no integer order; not served)");
                seen[(size_t)x[i]] = seen[(size_t)y[i]] = 1;
            }
            for (size_t g = 0; g < seen.size(); ++g)
                if (!seen[g]) throw SoError("so_cnc_groups: gene " + std::to_string(g) + " occurs in no row (genes are numbered by first appearance)");
        }
        int nd = 0;
        if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) throw SoError("so_cnc_groups: no HIP device available (libsohit has no CPU fallback)");
        if (device < 0 || device >= nd) throw SoError("so_cnc_groups: device index out of range");

        out->comp1 = (int64_t*)malloc((D ? D : 1) * sizeof(int64_t));
        out->grp = (int64_t*)malloc((D ? D : 1) * sizeof(int64_t));
        out->keep = (uint8_t*)malloc(N ? N : 1);
        if (!out->comp1 || !out->grp || !out->keep) throw SoError("so_cnc_groups: out of host memory");
        out->n_genes = n_genes, out->n_rows = n_rows;
        // no gene or no row: nothing to launch (a grid of 0 blocks is an invalid configuration).  Without a row no gene is linked:
        // group_numbers() leaves every comp1 at 0 and every grp at -1
        // one level-1 component: it is component 0, which never merges -- every gene in the -1 pool, every row kept, no level-2 launch
        auto one_pool = [&]() {
            for (size_t g = 0; g < D; ++g) out->comp1[g] = 0, out->grp[g] = -1;
            memset(out->keep, 1, N ? N : 1);
            out->n_grp = 0, out->n_keep = n_rows;
        };
        if (!D || !N) {
            one_pool();
            out->n_comp1 = D ? 1 : 0;
            g_cnc_err.clear();
            return 0;
        }

        HIP_CHECK(hipSetDevice(device));
        Tune tn;   // no context: the switches are read per call
        tn.read();
        const PoisonScope poison((int)tn.poison);
        hipStream_t st = nullptr;
        HIP_CHECK(hipStreamCreate(&st));
        struct Guard {
            hipStream_t s;
            ~Guard() { (void)hipStreamSynchronize(s), (void)hipStreamDestroy(s); }
        } guard{st};
        const u32 n = (u32)D, nr = (u32)N;
        DevBuf<int> d_x, d_y, d_grp;
        DevBuf<double> d_z;
        DevBuf<unsigned long long> d_best;
        DevBuf<u8> d_tie, d_keep;
        DevBuf<u32> d_lab, d_root, d_below, d_comp1, d_changed, d_tmp, d_lab2, d_first, d_flag, d_rank;
        d_x.ensure(N + 2), d_y.ensure(N + 2), d_z.ensure(N + 2), d_best.ensure(D + 2), d_tie.ensure(N + 2), d_lab.ensure(D + 2), d_changed.ensure(4);
        HIP_CHECK(hipMemcpyAsync(d_x.p, x, N * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d_y.p, y, N * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d_z.p, z, N * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemsetAsync(d_best.p, 0, D * sizeof(unsigned long long), st));   // below every weight's image
        hipLaunchKernelGGL(k_cnc_best, cnc_grid(nr), dim3(256), 0, st, d_x.p, d_y.p, d_z.p, nr, d_best.p);
        hipLaunchKernelGGL(k_cnc_tie, cnc_grid(nr), dim3(256), 0, st, d_x.p, d_y.p, d_z.p, nr, d_best.p, d_tie.p);
        hipLaunchKernelGGL(k_cnc_iota, cnc_grid(n), dim3(256), 0, st, d_lab.p, n);
        out->sweeps1 = cnc_sweeps<1>(d_x.p, d_y.p, nr, d_tie.p, nullptr, d_lab.p, n, d_changed.p, st);

        d_root.ensure(D + 2), d_below.ensure(D + 2), d_comp1.ensure(D + 2), d_tmp.ensure(scan_u32_temp_elems(std::max(D, N)) + 8);
        hipLaunchKernelGGL(k_cnc_roots, cnc_grid(n), dim3(256), 0, st, d_lab.p, n, d_root.p);
        const u32* d_roots = scan_u32(d_root.p, d_below.p, D, false, d_tmp.p, st);
        hipLaunchKernelGGL(k_cnc_number, cnc_grid(n), dim3(256), 0, st, d_lab.p, d_below.p, d_roots, n, d_comp1.p);
        u32 roots = 0;
        HIP_CHECK(hipMemcpyAsync(&roots, d_roots, sizeof(u32), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (roots < 1 || roots > n) throw SoError("so_cnc_groups: internal error: " + std::to_string(roots) + " level-1 roots among " + std::to_string(n) + " genes");
        out->n_comp1 = roots;
        if (roots == 1) {
            HIP_CHECK(hipGetLastError());
            one_pool();
            g_cnc_err.clear();
            return 0;
        }

        d_lab2.ensure((size_t)roots + 2), d_first.ensure((size_t)roots + 2), d_flag.ensure(N + 2), d_rank.ensure(N + 2), d_grp.ensure(D + 2), d_keep.ensure(N + 2);
        hipLaunchKernelGGL(k_cnc_iota, cnc_grid(roots), dim3(256), 0, st, d_lab2.p, roots);
        out->sweeps2 = cnc_sweeps<2>(d_x.p, d_y.p, nr, nullptr, d_comp1.p, d_lab2.p, roots, d_changed.p, st);
        HIP_CHECK(hipMemsetAsync(d_first.p, 0xFF, (size_t)roots * sizeof(u32), st));   // CNC_NONE
        hipLaunchKernelGGL(k_cnc_first, cnc_grid(nr), dim3(256), 0, st, d_x.p, d_y.p, nr, d_comp1.p, d_lab2.p, d_first.p);
        hipLaunchKernelGGL(k_cnc_firstflag, cnc_grid(nr), dim3(256), 0, st, d_x.p, d_y.p, nr, d_comp1.p, d_lab2.p, d_first.p, d_flag.p);
        const u32* d_ngrp = scan_u32(d_flag.p, d_rank.p, N, false, d_tmp.p, st);
        hipLaunchKernelGGL(k_cnc_grp, cnc_grid(n), dim3(256), 0, st, d_comp1.p, d_lab2.p, d_first.p, d_rank.p, n, d_grp.p);
        hipLaunchKernelGGL(k_cnc_keep, cnc_grid(nr), dim3(256), 0, st, d_x.p, d_y.p, nr, d_grp.p, d_keep.p);
        HIP_CHECK(hipGetLastError());
        u32 ngrp = 0;
        std::vector<u32> hc(D);
        std::vector<int> hg(D);
        HIP_CHECK(hipMemcpyAsync(&ngrp, d_ngrp, sizeof(u32), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(hc.data(), d_comp1.p, D * sizeof(u32), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(hg.data(), d_grp.p, D * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(out->keep, d_keep.p, N, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        int64_t nk = 0;
        for (size_t g = 0; g < D; ++g) out->comp1[g] = hc[g], out->grp[g] = hg[g];
        for (size_t i = 0; i < N; ++i) nk += out->keep[i];
        out->n_grp = ngrp, out->n_keep = nk;
        g_cnc_err.clear();
        return 0;
    } catch (const std::exception& e) {
        if (out) so_cnc_free(out);
        g_cnc_err = e.what();
        return 1;
    }
}

}  // extern "C"
