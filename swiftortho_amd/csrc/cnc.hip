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
//
// so_cnc_plan (the k_plan_* kernels further down) wraps the same stage into the whole plan cnc needs in front of its batches: from
// id codes to gene numbers, through the component stage where the arrays lie, to the kept rows in `sort -n` order with their cuts.
#include "common.h"
#include "device_call.h"
#include "kernels.h"
#include "../../include/sohit.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace {

#define CNC_JUMP 32   // label steps one lane follows per sweep

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
        if (f != NONE32) r = (int)rank[f];
    }
    grp[g] = r;
}

// (T = u8: the flags so_cnc_groups hands out;  T = u32: the flags so_cnc_plan scans)
template <typename T>
__global__ __launch_bounds__(256) void k_cnc_keep(const int* __restrict__ x, const int* __restrict__ y, u32 nr, const int* __restrict__ grp, T* __restrict__ keep) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nr) return;
    const int a = grp[x[i]], b = grp[y[i]];
    keep[i] = (a == b && a != 0) ? 1 : 0;
}

// hook + jump until a sweep moves no label; -> sweeps run, the confirming one included
template <int LEVEL>
int cnc_sweeps(const int* x, const int* y, u32 nr, const u8* tie, const u32* comp1, u32* lab, u32 nodes, u32* changed, hipStream_t st, const std::string& who) {
    const u64 cap = (u64)nodes + 2;
    for (u64 s = 1; s <= cap; ++s) {
        HIP_CHECK(hipMemsetAsync(changed, 0, sizeof(u32), st));
        hipLaunchKernelGGL(k_cnc_hook<LEVEL>, grid256(nr), dim3(256), 0, st, x, y, nr, tie, comp1, lab, changed);
        hipLaunchKernelGGL(k_cnc_jump, grid256(nodes), dim3(256), 0, st, lab, nodes, changed);
        u32 moved = 0;
        HIP_CHECK(hipMemcpyAsync(&moved, changed, sizeof(u32), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (!moved) return (int)s;
    }
    throw SoError(who + ": the level-" + std::to_string(LEVEL) + " labels still moved after " + std::to_string(cap) + " sweeps (nodes + 2): no result");
}

// what the component stage leaves on the device, and its scratch
struct CncDev {
    DevBuf<unsigned long long> best;
    DevBuf<u8> tie;
    DevBuf<u32> lab, root, below, comp1, changed, tmp, lab2, first, flag, rank;
    DevBuf<int> grp;
    const u32* d_ngrp = nullptr;   // device word: level-2 groups (inside tmp: valid until tmp is scanned with again)
    u32 roots = 0;
    int sweeps1 = 0, sweeps2 = 0, waits = 0;
};

// The component stage on rows that are on the device (n genes numbered by first appearance, nr rows, both above 0), queued on st:
// comp1[n] and, when there is more than one level-1 component, grp[n] and *d_ngrp.  -> false when there is one level-1 component: it
// is component 0, which never merges -- every gene in the -1 pool, every row kept, nothing of level 2 launched, grp not written.
// Both entry points run this body (`who` names the one in an error).
bool cnc_component_stage(const int* d_x, const int* d_y, const double* d_z, u32 n, u32 nr, CncDev& c, hipStream_t st, const std::string& who) {
    const size_t D = n, N = nr;
    c.best.ensure(D + 2), c.tie.ensure(N + 2), c.lab.ensure(D + 2), c.changed.ensure(4);
    HIP_CHECK(hipMemsetAsync(c.best.p, 0, D * sizeof(unsigned long long), st));   // below every weight's image
    hipLaunchKernelGGL(k_cnc_best, grid256(nr), dim3(256), 0, st, d_x, d_y, d_z, nr, c.best.p);
    hipLaunchKernelGGL(k_cnc_tie, grid256(nr), dim3(256), 0, st, d_x, d_y, d_z, nr, c.best.p, c.tie.p);
    hipLaunchKernelGGL(k_cnc_iota, grid256(n), dim3(256), 0, st, c.lab.p, n);
    c.sweeps1 = cnc_sweeps<1>(d_x, d_y, nr, c.tie.p, nullptr, c.lab.p, n, c.changed.p, st, who);

    c.root.ensure(D + 2), c.below.ensure(D + 2), c.comp1.ensure(D + 2), c.tmp.ensure(scan_u32_temp_elems(std::max(D, N)) + 8);
    hipLaunchKernelGGL(k_cnc_roots, grid256(n), dim3(256), 0, st, c.lab.p, n, c.root.p);
    const u32* d_roots = scan_u32(c.root.p, c.below.p, D, false, c.tmp.p, st);
    hipLaunchKernelGGL(k_cnc_number, grid256(n), dim3(256), 0, st, c.lab.p, c.below.p, d_roots, n, c.comp1.p);
    u32 roots = 0;
    HIP_CHECK(hipMemcpyAsync(&roots, d_roots, sizeof(u32), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (roots < 1 || roots > n) throw SoError(who + ": internal error: " + std::to_string(roots) + " level-1 roots among " + std::to_string(n) + " genes");
    c.roots = roots, c.waits = c.sweeps1 + 1;
    if (roots == 1) {
        HIP_CHECK(hipGetLastError());
        return false;
    }

    c.lab2.ensure((size_t)roots + 2), c.first.ensure((size_t)roots + 2), c.flag.ensure(N + 2), c.rank.ensure(N + 2), c.grp.ensure(D + 2);
    hipLaunchKernelGGL(k_cnc_iota, grid256(roots), dim3(256), 0, st, c.lab2.p, roots);
    c.sweeps2 = cnc_sweeps<2>(d_x, d_y, nr, nullptr, c.comp1.p, c.lab2.p, roots, c.changed.p, st, who);
    c.waits += c.sweeps2;
    HIP_CHECK(hipMemsetAsync(c.first.p, 0xFF, (size_t)roots * sizeof(u32), st));   // NONE32
    hipLaunchKernelGGL(k_cnc_first, grid256(nr), dim3(256), 0, st, d_x, d_y, nr, c.comp1.p, c.lab2.p, c.first.p);
    hipLaunchKernelGGL(k_cnc_firstflag, grid256(nr), dim3(256), 0, st, d_x, d_y, nr, c.comp1.p, c.lab2.p, c.first.p, c.flag.p);
    c.d_ngrp = scan_u32(c.flag.p, c.rank.p, N, false, c.tmp.p, st);
    hipLaunchKernelGGL(k_cnc_grp, grid256(n), dim3(256), 0, st, c.comp1.p, c.lab2.p, c.first.p, c.rank.p, n, c.grp.p);
    return true;
}

// ---- the row plan (so_cnc_plan): what cnc does between the id codes and the batches -------------------------------------------------
// Rows come as id CODES (cx <= cy, code order = the ids' byte order).  Genes are numbered by first appearance in cx0, cy0, cx1, ...
// (number_by_first_appearance, k_util.hip); the component stage runs on those numbers; the kept rows are flagged, scanned and compacted
// into (key, row) pairs; a stable radix sort puts them into (grp as a signed number, cx, cy) order -- grp + 1 is the unsigned image: the
// pool -1 becomes 0, group 0 is never kept -- and rows with an equal triple stay in file order; the positions where grp changes (`cut`)
// and where the whole triple repeats (`tied`) are a neighbour comparison, a scan and a compaction each.  Integer atomics only.

// kept row i -> slot pos[i]: its row index and its key.  ONE: grp + 1, cx, cy in one word (cb bits per code);  else cx << 32 | cy
template <bool ONE>
__global__ __launch_bounds__(256) void k_plan_keys(const int* __restrict__ cx, const int* __restrict__ cy, const int* __restrict__ X, const int* __restrict__ grp,
                                                   u32 nr, const u32* __restrict__ flag, const u32* __restrict__ pos, int cb, u64* __restrict__ key,
                                                   u32* __restrict__ row) {
    const size_t i = tid256();
    if (i >= nr || !flag[i]) return;
    const u32 p = pos[i];
    row[p] = (u32)i;
    if (ONE) key[p] = ((u64)(u32)(grp[X[i]] + 1) << (2 * cb)) | ((u64)(u32)cx[i] << cb) | (u64)(u32)cy[i];
    else key[p] = ((u64)(u32)cx[i] << 32) | (u64)(u32)cy[i];
}
// the second pass's key of the rows in (cx, cy) order
__global__ __launch_bounds__(256) void k_plan_grpkey(const int* __restrict__ X, const int* __restrict__ grp, const u32* __restrict__ row, u32 nk,
                                                     u64* __restrict__ key) {
    const size_t p = tid256();
    if (p < nk) key[p] = (u64)(u32)(grp[X[row[p]]] + 1);
}
// position p >= 1 of the sorted rows against p - 1 (position 0 carries no flag)
__global__ __launch_bounds__(256) void k_plan_edges(const int* __restrict__ cx, const int* __restrict__ cy, const int* __restrict__ X, const int* __restrict__ grp,
                                                    const u32* __restrict__ order, u32 nk, u32* __restrict__ cutflag, u32* __restrict__ tiedflag) {
    const size_t p = tid256();
    if (p >= nk) return;
    u32 c = 0, t = 0;
    if (p) {
        const u32 r = order[p], q = order[p - 1];
        const bool same_grp = grp[X[r]] == grp[X[q]];
        c = same_grp ? 0u : 1u;
        t = (same_grp && cx[r] == cx[q] && cy[r] == cy[q]) ? 1u : 0u;
    }
    cutflag[p] = c, tiedflag[p] = t;
}
__global__ __launch_bounds__(256) void k_plan_compact(const u32* __restrict__ cutflag, const u32* __restrict__ cutpos, const u32* __restrict__ tiedflag,
                                                      const u32* __restrict__ tiedpos, u32 nk, int* __restrict__ cut, int* __restrict__ tied) {
    const size_t p = tid256();
    if (p >= nk) return;
    if (cutflag[p]) cut[cutpos[p]] = (int)p;
    if (tiedflag[p]) tied[tiedpos[p]] = (int)p;
}

thread_local std::string g_cnc_err;

auto slots(so_cnc_result* r) { return result_slots(&r->comp1, &r->grp, &r->keep); }
auto slots(so_cnc_plan_result* r) { return result_slots(&r->gene_code, &r->x, &r->y, &r->comp1, &r->grp, &r->order, &r->cut, &r->tied); }

}  // namespace

extern "C" {

const char* so_cnc_last_error(void) { return g_cnc_err.c_str(); }

void so_cnc_free(so_cnc_result* r) {
    if (r) release_slots(r, slots(r));
}

int so_cnc_groups(int device, int64_t n_genes, int64_t n_rows, const int32_t* x, const int32_t* y, const double* z, so_cnc_result* out) {
    return guarded_call(g_cnc_err, out, so_cnc_free, [&] {
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
        check_device("so_cnc_groups", device);

        out->comp1 = host_array<int64_t>("so_cnc_groups", D), out->grp = host_array<int64_t>("so_cnc_groups", D), out->keep = host_array<uint8_t>("so_cnc_groups", N);
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
            return;
        }

        DeviceCall call(device);
        const hipStream_t st = call.st;
        const u32 n = (u32)D, nr = (u32)N;
        DevBuf<int> d_x, d_y;
        DevBuf<double> d_z;
        DevBuf<u8> d_keep;
        CncDev c;
        d_x.ensure(N + 2), d_y.ensure(N + 2), d_z.ensure(N + 2);
        HIP_CHECK(hipMemcpyAsync(d_x.p, x, N * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d_y.p, y, N * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d_z.p, z, N * sizeof(double), hipMemcpyHostToDevice, st));
        const bool level2 = cnc_component_stage(d_x.p, d_y.p, d_z.p, n, nr, c, st, "so_cnc_groups");
        out->sweeps1 = c.sweeps1, out->sweeps2 = c.sweeps2, out->n_comp1 = c.roots;
        if (!level2) {
            one_pool();
            return;
        }
        d_keep.ensure(N + 2);
        hipLaunchKernelGGL(k_cnc_keep<u8>, grid256(nr), dim3(256), 0, st, d_x.p, d_y.p, nr, c.grp.p, d_keep.p);
        HIP_CHECK(hipGetLastError());
        u32 ngrp = 0;
        std::vector<u32> hc(D);
        std::vector<int> hg(D);
        HIP_CHECK(hipMemcpyAsync(&ngrp, c.d_ngrp, sizeof(u32), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(hc.data(), c.comp1.p, D * sizeof(u32), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(hg.data(), c.grp.p, D * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(out->keep, d_keep.p, N, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        int64_t nk = 0;
        for (size_t g = 0; g < D; ++g) out->comp1[g] = hc[g], out->grp[g] = hg[g];
        for (size_t i = 0; i < N; ++i) nk += out->keep[i];
        out->n_grp = ngrp, out->n_keep = nk;
    });
}

void so_cnc_plan_free(so_cnc_plan_result* r) {
    if (r) release_slots(r, slots(r));
}

int so_cnc_plan(int device, int64_t n_codes, int64_t n_rows, const int32_t* cx, const int32_t* cy, const double* z, int32_t flags, so_cnc_plan_result* out) {
    return guarded_call(g_cnc_err, out, so_cnc_plan_free, [&] {
        if (!out) throw SoError("so_cnc_plan: result pointer is NULL");
        memset(out, 0, sizeof *out);
        if (n_codes < 0 || n_rows < 0 || (n_rows > 0 && (!cx || !cy || !z))) throw SoError("so_cnc_plan: bad arguments");
        if (n_codes >= (1ll << 31) || n_rows >= (1ll << 31)) throw SoError("so_cnc_plan: 2^31 codes or rows and more are not served (32-bit codes and row indices)");
        const size_t N = (size_t)n_rows;
        for (size_t i = 0; i < N; ++i) {
            if (cx[i] < 0 || cx[i] >= n_codes || cy[i] < 0 || cy[i] >= n_codes)
                throw SoError("so_cnc_plan: row " + std::to_string(i) + " names a code outside 0 .. n_codes - 1");
            if (cx[i] > cy[i]) throw SoError("so_cnc_plan: row " + std::to_string(i) + " has cx > cy (cnc drops such rows before anything is numbered)");
            if (z[i] != z[i]) throw SoError("so_cnc_plan: row " + std::to_string(i) + " has a NaN weight (numpy's answer to it has no integer order; not served)");
        }
        check_device("so_cnc_plan", device);
        out->n_codes = n_codes, out->n_rows = n_rows;
        auto alloc = [](size_t n) { return host_array<int32_t>("so_cnc_plan", n); };
        if (!N) {   // no row: no gene, nothing kept, nothing to launch
            out->gene_code = alloc(0), out->x = alloc(0), out->y = alloc(0), out->comp1 = alloc(0);
            out->grp = alloc(0), out->order = alloc(0), out->cut = alloc(0), out->tied = alloc(0);
            return;
        }

        DeviceCall call(device);
        const hipStream_t st = call.st;
        const u32 nr = (u32)N;
        const size_t C = (size_t)n_codes, N2 = 2 * N;

        // genes numbered by first appearance
        DevBuf<int> d_cx, d_cy, d_x, d_y, d_gene;
        DevBuf<double> d_z;
        DevBuf<u32> d_first, d_flag, d_rank, d_tmp_a, d_tmp_b;
        d_cx.ensure(N + 2), d_cy.ensure(N + 2), d_z.ensure(N + 2), d_x.ensure(N + 2), d_y.ensure(N + 2), d_first.ensure(C + 2);
        d_flag.ensure(N2 + 2), d_rank.ensure(N2 + 2), d_tmp_a.ensure(scan_u32_temp_elems(N2) + 8), d_tmp_b.ensure(scan_u32_temp_elems(N2) + 8);
        d_gene.ensure(std::min(C, N2) + 2);
        HIP_CHECK(hipMemcpyAsync(d_cx.p, cx, N * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d_cy.p, cy, N * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d_z.p, z, N * sizeof(double), hipMemcpyHostToDevice, st));
        const u32 n = call.read(number_by_first_appearance(d_cx.p, d_cy.p, nr, (u32)C, d_first.p, d_flag.p, d_rank.p, d_tmp_a.p, d_x.p, d_y.p, d_gene.p, st));
        if (n < 1 || n > C || n > N2) throw SoError("so_cnc_plan: internal error: " + std::to_string(n) + " genes in " + std::to_string(nr) + " rows");
        const size_t D = n;

        // the component stage, on the rows where they are
        CncDev c;
        const bool level2 = cnc_component_stage(d_x.p, d_y.p, d_z.p, n, nr, c, st, "so_cnc_plan");
        call.waits += c.waits;
        if (!level2) {   // one level-1 component: comp1 0 and grp -1 for every gene
            c.grp.ensure(D + 2);
            HIP_CHECK(hipMemsetAsync(c.comp1.p, 0, D * sizeof(u32), st));
            HIP_CHECK(hipMemsetAsync(c.grp.p, 0xFF, D * sizeof(int), st));
        }

        // kept rows: flag, scan, compact
        DevBuf<u32> d_keep, d_pos;
        d_keep.ensure(N + 2), d_pos.ensure(N + 2);
        hipLaunchKernelGGL(k_cnc_keep<u32>, grid256(nr), dim3(256), 0, st, d_x.p, d_y.p, nr, c.grp.p, d_keep.p);
        const u32* d_nkeep = scan_u32(d_keep.p, d_pos.p, N, false, d_tmp_a.p, st);
        u32 nk = 0, ngrp = 0;
        call.read(d_nkeep, nk, level2 ? c.d_ngrp : nullptr, ngrp);
        if (nk > nr || ngrp > n) throw SoError("so_cnc_plan: internal error: " + std::to_string(nk) + " rows kept, " + std::to_string(ngrp) + " groups");
        HIP_CHECK(hipGetLastError());

        out->gene_code = alloc(D), out->x = alloc(N), out->y = alloc(N), out->comp1 = alloc(D);
        out->grp = alloc(D), out->order = alloc(nk);
        HIP_CHECK(hipMemcpyAsync(out->gene_code, d_gene.p, D * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(out->x, d_x.p, N * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(out->y, d_y.p, N * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(out->comp1, c.comp1.p, D * sizeof(u32), hipMemcpyDeviceToHost, st));   // (numbers below 2^31)
        HIP_CHECK(hipMemcpyAsync(out->grp, c.grp.p, D * sizeof(int), hipMemcpyDeviceToHost, st));

        u32 ncut = 0, ntied = 0;
        int passes = 0;
        DevBuf<u64> d_key, d_skey;
        DevBuf<u32> d_row, d_order, d_cutflag, d_tiedflag, d_cutpos, d_tiedpos;
        DevBuf<int> d_cut, d_tied;
        DevBuf<u8> d_sort_tmp;
        if (nk) {
            const size_t K = nk;
            const int cb = ceil_log2((u64)n_codes), gb = ceil_log2((u64)ngrp + 1);
            const bool one = !(flags & 1) && gb + 2 * cb <= 64;
            passes = one ? 1 : 2;
            d_key.ensure(K + 2), d_skey.ensure(K + 2), d_row.ensure(K + 2), d_order.ensure(K + 2);
            if (one) {
                hipLaunchKernelGGL(k_plan_keys<true>, grid256(N), dim3(256), 0, st, d_cx.p, d_cy.p, d_x.p, c.grp.p, nr, d_keep.p, d_pos.p, cb, d_key.p, d_row.p);
                d_sort_tmp.ensure(sort_pairs_u64_u32_temp_bytes(K, gb + 2 * cb) + 256);
                sort_pairs_u64_u32(d_sort_tmp.p, d_sort_tmp.cap, d_key.p, d_skey.p, d_row.p, d_order.p, K, gb + 2 * cb, st);   // stable: file order inside a triple
            } else {
                hipLaunchKernelGGL(k_plan_keys<false>, grid256(N), dim3(256), 0, st, d_cx.p, d_cy.p, d_x.p, c.grp.p, nr, d_keep.p, d_pos.p, cb, d_key.p, d_row.p);
                d_sort_tmp.ensure(std::max(sort_pairs_u64_u32_temp_bytes(K, 32 + cb), sort_pairs_u64_u32_temp_bytes(K, gb)) + 256);
                sort_pairs_u64_u32(d_sort_tmp.p, d_sort_tmp.cap, d_key.p, d_skey.p, d_row.p, d_order.p, K, 32 + cb, st);          // (cx, cy), stable
                hipLaunchKernelGGL(k_plan_grpkey, grid256(K), dim3(256), 0, st, d_x.p, c.grp.p, d_order.p, nk, d_key.p);
                sort_pairs_u64_u32(d_sort_tmp.p, d_sort_tmp.cap, d_key.p, d_skey.p, d_order.p, d_row.p, K, gb, st);                // then grp + 1, stable
                std::swap(d_order.p, d_row.p), std::swap(d_order.cap, d_row.cap);
            }
            HIP_CHECK(hipMemcpyAsync(out->order, d_order.p, K * sizeof(u32), hipMemcpyDeviceToHost, st));
            // cut and tied: neighbour comparison, scan, compact
            d_cutflag.ensure(K + 2), d_tiedflag.ensure(K + 2), d_cutpos.ensure(K + 2), d_tiedpos.ensure(K + 2), d_cut.ensure(K + 2), d_tied.ensure(K + 2);
            hipLaunchKernelGGL(k_plan_edges, grid256(K), dim3(256), 0, st, d_cx.p, d_cy.p, d_x.p, c.grp.p, d_order.p, nk, d_cutflag.p, d_tiedflag.p);
            const u32* d_ncut = scan_u32(d_cutflag.p, d_cutpos.p, K, false, d_tmp_a.p, st);
            const u32* d_ntied = scan_u32(d_tiedflag.p, d_tiedpos.p, K, false, d_tmp_b.p, st);
            hipLaunchKernelGGL(k_plan_compact, grid256(K), dim3(256), 0, st, d_cutflag.p, d_cutpos.p, d_tiedflag.p, d_tiedpos.p, nk, d_cut.p, d_tied.p);
            HIP_CHECK(hipGetLastError());
            call.read(d_ncut, ncut, d_ntied, ntied);   // (the arrays queued above arrive with this wait)
            if (ncut >= nk || ntied >= nk || ncut > ngrp) throw SoError("so_cnc_plan: internal error: " + std::to_string(ncut) + " cuts and " + std::to_string(ntied) + " ties among " + std::to_string(nk) + " rows");
        }
        out->cut = alloc(ncut), out->tied = alloc(ntied);
        if (ncut) HIP_CHECK(hipMemcpyAsync(out->cut, d_cut.p, (size_t)ncut * sizeof(int), hipMemcpyDeviceToHost, st));
        if (ntied) HIP_CHECK(hipMemcpyAsync(out->tied, d_tied.p, (size_t)ntied * sizeof(int), hipMemcpyDeviceToHost, st));
        if (ncut || ntied || !nk) {
            call.wait();
        }
        out->n_genes = n, out->n_comp1 = c.roots, out->n_grp = ngrp, out->n_keep = nk, out->n_cut = ncut, out->n_tied = ntied;
        out->sweeps1 = c.sweeps1, out->sweeps2 = c.sweeps2, out->sort_passes = passes, out->waits = call.waits;
    });
}

}  // extern "C"
