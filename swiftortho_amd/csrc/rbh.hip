// rbh.hip -- reciprocal best hits and the core-gene table on the device: from the hit rows of a search (columns uploaded from the host,
// or the so_hit records so_search_device left in HBM) to what swiftortho_amd/rbh.py `reciprocal_best_hits()` and `core_table()` define --
// the pairs scripts/get_rbh.py prints, in its order, and the forward / reciprocal table scripts/rbh2phy.py builds in its two passes.
//
// The numpy functions are the definition:
//   * a run = consecutive rows of one query code; per (run, subject taxon other than the query's) the WINNER is the first row holding
//     the largest score (doubles compared with > and ==: +0 and -0 tie and the earlier row wins; a NaN is refused before anything is
//     compared); the winner list is ordered by the first row of each (run, taxon) group;
//   * pairs: winner p proposes the key min(q, s) * M + max(q, s); the j-th proposal of a key (from 1) lists the pair iff j is even, at
//     position p of the stream;
//   * core, pass 1 (winners whose query has taxon R): genes are numbered by their first such winner; fwd[gene][taxon of s] = s of the
//     LAST such winner; pass 2 (winners whose query has another taxon and whose subject has taxon R): rec[gene s][taxon of q] = 1 when
//     fwd[gene s][taxon of q] == q.
// Nothing in the output depends on scheduling: positions come from flag -> scan -> compact, the sorts are stable, and the three atomics
// are integer minima / maxima of stream positions (first winner per gene, last winner per cell) -- exact whatever the order.
//
// Kernels.  k_rbh_unpack (records -> columns; hit_codes, hit_table.h), k_rbh_check, key_runs -> run_starts (k_util.hip: k_run_heads ->
// scan -> k_run_starts, the run bounds).  Every host wait goes through the call's DeviceCall (device_call.h) and is counted.  The host
// reads the run bounds and lists the runs the wave tier cannot hold (tune.h RBH_WAVE_ROWS; SOHIT_RBH_TIER=long sends every run there):
//   k_rbh_run_wave   a run of up to 64 rows per wave, a row per lane: every lane walks the run's lanes with shuffles and keeps the first
//                    maximum of its own subject taxon; the first lane of a taxon stands for the group;
//   k_rbh_long_keys -> SortedGroups (device_call.h: stable radix sort of (long run, taxon) with the row as payload, segments) ->
//                    k_rbh_seg_max: one wave per (run, taxon) segment, rows ascending inside it, first maximum by a strided walk and
//                    a butterfly.
// Both write flag[first row of the group] = 1 and wrow[first row] = winner row; scan, k_rbh_winners compacts (q, s) of the winners.
// Pairs: k_rbh_pair_keys -> SortedGroups -> k_rbh_even (occurrence = index - segment start) -> scan -> k_rbh_pair_emit.
// Core: k_rbh_first (atomicMin) -> k_rbh_gene_flag -> scan -> k_rbh_gene_emit -> k_rbh_last (atomicMax) -> k_rbh_fwd -> k_rbh_rec.
#include "common.h"
#include "hit_table.h"

#include <cstring>
#include <string>
#include <vector>

namespace {

static_assert(RBH_WAVE_ROWS == 64, "k_rbh_run_wave holds a run a row per lane of one wave");

// ---- rows ----------------------------------------------------------------------------------------------------------------------------
// so_hit records -> the columns columns_from_records() builds; err |= 1 / 2: a qidx / sidx outside its map
__global__ __launch_bounds__(256) void k_rbh_unpack(const so_hit* __restrict__ h, u32 n, const int* __restrict__ qmap, i64 nq, const int* __restrict__ smap, i64 ns,
                                                    int* __restrict__ q, int* __restrict__ s, double* __restrict__ score, u32* __restrict__ err) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    int qc, sc;
    hit_codes(h[i], qmap, nq, smap, ns, qc, sc, err);
    q[i] = qc, s[i] = sc, score[i] = (double)h[i].bit;
}

// err |= 4: a name code outside [0, n_names); err |= 16: a NaN score
__global__ __launch_bounds__(256) void k_rbh_check(u32 n, const int* __restrict__ q, const int* __restrict__ s, const double* __restrict__ score, i64 n_names,
                                                   u32* __restrict__ err) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (q[i] < 0 || q[i] >= n_names || s[i] < 0 || s[i] >= n_names) atomicOr(err, 4u);
    if (score[i] != score[i]) atomicOr(err, 16u);
}

// ---- winners -------------------------------------------------------------------------------------------------------------------------
// a run of up to 64 rows per wave, a row per lane.  Runs the wave cannot hold (or all, when the sorted tier is forced) are left alone:
// their flags stay 0 until k_rbh_seg_max sets them.
__global__ __launch_bounds__(256) void k_rbh_run_wave(const u32* __restrict__ rstart, u32 nruns, int all_long, const int* __restrict__ q, const int* __restrict__ s,
                                                      const double* __restrict__ score, const int* __restrict__ tax, u32* __restrict__ flag, u32* __restrict__ wrow) {
    const u32 w = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (w >= nruns) return;   // (a whole wave)
    const u32 lane = threadIdx.x & 63u;
    const u32 b = rstart[w], len = rstart[w + 1] - b;
    if (all_long || len > RBH_WAVE_ROWS) return;   // (a whole wave)
    const bool have = lane < len;
    const int qtx = tax[q[b]];
    int t = -1;          // no lane below len holds -1: idle lanes match nobody
    double v = 0.;
    if (have) t = tax[s[b + lane]], v = score[b + lane];
    bool first = have && t != qtx;
    int bj = -1;
    double bv = 0.;
    for (u32 j = 0; j < len; ++j) {   // ascending lanes: a later equal score never replaces the earlier one
        const int tj = __shfl(t, (int)j);
        const double vj = __shfl(v, (int)j);
        if (tj == t) {
            if (j < lane) first = false;
            if (bj < 0 || vj > bv) bj = (int)j, bv = vj;
        }
    }
    if (have) {
        flag[b + lane] = first ? 1u : 0u;
        if (first) wrow[b + lane] = b + (u32)bj;
    }
}

// the rows of long run lrun[k] stand at loff[k] .. of the list: key = k * T + subject taxon, val = row
__global__ __launch_bounds__(256) void k_rbh_long_keys(const u32* __restrict__ lrun, const u32* __restrict__ loff, const u32* __restrict__ rstart, const int* __restrict__ s,
                                                       const int* __restrict__ tax, u32 T, u64* __restrict__ key, u32* __restrict__ val) {
    const u32 k = blockIdx.x;
    const u32 r = lrun[k];
    const u32 b = rstart[r], len = rstart[r + 1] - b, o = loff[k];
    for (u32 i = threadIdx.x; i < len; i += 256u) key[o + i] = (u64)k * T + (u64)tax[s[b + i]], val[o + i] = b + i;
}

// one wave per (long run, taxon) segment of the sorted list; the rows of a segment ascend (stable sort)
__global__ __launch_bounds__(256) void k_rbh_seg_max(const u32* __restrict__ start, u32 nseg, const u64* __restrict__ skey, const u32* __restrict__ srow,
                                                     const u32* __restrict__ lrun, const u32* __restrict__ rstart, const int* __restrict__ q,
                                                     const double* __restrict__ score, const int* __restrict__ tax, u32 T, u32* __restrict__ flag, u32* __restrict__ wrow) {
    const u32 w = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (w >= nseg) return;   // (a whole wave)
    const u32 lane = threadIdx.x & 63u;
    const u32 lo = (u32)__builtin_amdgcn_readfirstlane((int)start[w]), hi = (u32)__builtin_amdgcn_readfirstlane((int)start[w + 1]);
    const u64 key = skey[lo];
    const int t = (int)(key % T);
    if (t == tax[q[rstart[lrun[key / T]]]]) return;   // the query's own taxon: no winner (a whole wave)
    u32 br = NONE32;
    double bv = 0.;
    for (u32 i = lo + lane; i < hi; i += 64u) {   // this lane's rows ascend
        const u32 r = srow[i];
        const double v = score[r];
        if (br == NONE32 || v > bv) br = r, bv = v;
    }
    for (int o = 32; o > 0; o >>= 1) {   // (larger score, then lower row): a total order, so every lane ends with the same winner
        const u32 orow = (u32)__shfl_xor((int)br, o);
        const double ov = __shfl_xor(bv, o);
        if (orow != NONE32 && (br == NONE32 || ov > bv || (ov == bv && orow < br))) br = orow, bv = ov;
    }
    if (lane == 0) {
        const u32 f = srow[lo];
        flag[f] = 1u, wrow[f] = br;
    }
}

// the winner list: (q, s) of the winner of every flagged group, in the order of the groups' first rows
__global__ __launch_bounds__(256) void k_rbh_winners(u32 n, const u32* __restrict__ flag, const u32* __restrict__ pos, const u32* __restrict__ wrow,
                                                     const int* __restrict__ q, const int* __restrict__ s, int* __restrict__ wq, int* __restrict__ ws) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const u32 p = pos[i];
    wq[p] = q[i], ws[p] = s[wrow[i]];
}

// ---- pairs ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rbh_pair_keys(u32 nw, const int* __restrict__ wq, const int* __restrict__ ws, u64 M, u64* __restrict__ key, u32* __restrict__ idx) {
    const u32 p = blockIdx.x * 256u + threadIdx.x;
    if (p >= nw) return;
    const u64 a = (u64)min(wq[p], ws[p]), b = (u64)max(wq[p], ws[p]);
    key[p] = a * M + b, idx[p] = p;
}
// sorted by key, the proposals of a key in stream order: the 2nd, 4th, ... list the pair at their own place in the stream
__global__ __launch_bounds__(256) void k_rbh_even(u32 nw, const u32* __restrict__ sidx, const u32* __restrict__ rid, const u32* __restrict__ start, u32* __restrict__ even) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i < nw) even[sidx[i]] = (i - start[rid[i] - 1u]) & 1u;
}
__global__ __launch_bounds__(256) void k_rbh_pair_emit(u32 nw, const u32* __restrict__ even, const u32* __restrict__ pos, const int* __restrict__ wq, const int* __restrict__ ws,
                                                       int* __restrict__ oa, int* __restrict__ ob) {
    const u32 p = blockIdx.x * 256u + threadIdx.x;
    if (p >= nw || !even[p]) return;
    oa[pos[p]] = min(wq[p], ws[p]), ob[pos[p]] = max(wq[p], ws[p]);
}

// ---- core table ----------------------------------------------------------------------------------------------------------------------
// first[gene] = its first pass-1 winner (winners whose query has the reference taxon R)
__global__ __launch_bounds__(256) void k_rbh_first(u32 nw, const int* __restrict__ wq, const int* __restrict__ tax, int R, u32* __restrict__ first) {
    const u32 p = blockIdx.x * 256u + threadIdx.x;
    if (p < nw && tax[wq[p]] == R) atomicMin(first + wq[p], p);
}
__global__ __launch_bounds__(256) void k_rbh_gene_flag(u32 nw, const int* __restrict__ wq, const int* __restrict__ tax, int R, const u32* __restrict__ first, u32* __restrict__ gflag) {
    const u32 p = blockIdx.x * 256u + threadIdx.x;
    if (p < nw) gflag[p] = (tax[wq[p]] == R && first[wq[p]] == p) ? 1u : 0u;
}
// genes in table order; gidx[name code] = its row of the table (first is reused: the position becomes the row)
__global__ __launch_bounds__(256) void k_rbh_gene_emit(u32 nw, const u32* __restrict__ gflag, const u32* __restrict__ gpos, const int* __restrict__ wq, int* __restrict__ gene,
                                                       u32* __restrict__ gidx) {
    const u32 p = blockIdx.x * 256u + threadIdx.x;
    if (p >= nw || !gflag[p]) return;
    gene[gpos[p]] = wq[p], gidx[wq[p]] = gpos[p];
}
// last[gene row * T + taxon of s] = 1 + the last pass-1 winner of the cell (0: none)
__global__ __launch_bounds__(256) void k_rbh_last(u32 nw, const int* __restrict__ wq, const int* __restrict__ ws, const int* __restrict__ tax, int R, u32 T,
                                                  const u32* __restrict__ gidx, u32* __restrict__ last) {
    const u32 p = blockIdx.x * 256u + threadIdx.x;
    if (p < nw && tax[wq[p]] == R) atomicMax(last + (size_t)gidx[wq[p]] * T + (u32)tax[ws[p]], p + 1u);
}
__global__ __launch_bounds__(256) void k_rbh_fwd(u32 cells, const u32* __restrict__ last, const int* __restrict__ ws, int* __restrict__ fwd) {
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c < cells) fwd[c] = last[c] ? ws[last[c] - 1u] : -1;
}
// pass 2: a winner of another taxon's query among the subjects of R confirms the cell whose forward hit it is
__global__ __launch_bounds__(256) void k_rbh_rec(u32 nw, const int* __restrict__ wq, const int* __restrict__ ws, const int* __restrict__ tax, int R, u32 T,
                                                 const u32* __restrict__ gidx, const int* __restrict__ fwd, u8* __restrict__ rec) {
    const u32 p = blockIdx.x * 256u + threadIdx.x;
    if (p >= nw) return;
    const int qq = wq[p], g = ws[p];
    if (tax[qq] == R || tax[g] != R) return;
    const u32 row = gidx[g];
    if (row == NONE32) return;   // the gene has no forward hit at all
    const size_t c = (size_t)row * T + (u32)tax[qq];
    if (fwd[c] == qq) rec[c] = 1;
}

thread_local std::string g_rbh_err;

// the stage on device columns of n > 0 rows; d_err: what the unpack kernel may have set already
void rbh_run(DeviceCall& call, u32 n, const int* q, const int* s, const double* score, i64 n_names, const int32_t* tax, i64 n_taxa, int R, u32* d_err, const char* who,
             so_rbh_result* out) {
    hipStream_t st = call.st;
    const u64 M = (u64)(n_names > 0 ? n_names : 1);
    const u32 T = (u32)(n_taxa > 0 ? n_taxa : 1);
    DevBuf<int> d_tax, wq, ws;
    DevBuf<u32> head, rid, rstart, tmp, flag, wrow, pos;
    upload(d_tax, tax, (size_t)n_names, st);
    head.ensure(n + 2), rid.ensure(n + 2), rstart.ensure((size_t)n + 3), tmp.ensure(scan_u32_temp_elems(n) + 2);
    hipLaunchKernelGGL(k_rbh_check, grid256(n), dim3(256), 0, st, n, q, s, score, n_names, d_err);
    const u32* d_nruns = key_runs(q, n, head.p, rid.p, tmp.p, st);
    run_starts(head.p, rid.p, n, d_nruns, rstart.p, st);
    HIP_CHECK(hipGetLastError());
    u32 nruns = 0, err = 0;
    call.read(d_nruns, nruns, d_err, err);
    hit_table_errors(who, err);
    if (err & 16u) throw SoError(std::string(who) + ": a NaN score (the order of such rows is not defined here)");
    out->n_runs = nruns;

    // the runs the wave tier cannot hold, their rows laid out one run behind the other
    std::vector<u32> rs((size_t)nruns + 1), lrun, loff;
    call.fetch(rs.data(), rstart.p, rs.size());
    call.wait();
    const bool all_long = call.tn.rbh_tier >= 2;   // (forcing the wave tier changes nothing: it already takes every run it can hold)
    u64 nlong = 0;
    for (u32 r = 0; r < nruns; ++r) {
        const u32 len = rs[r + 1] - rs[r];
        if (all_long || len > RBH_WAVE_ROWS) lrun.push_back(r), loff.push_back((u32)nlong), nlong += len;
    }
    out->n_runs_long = (i64)lrun.size(), out->n_rows_long = (i64)nlong;

    flag.ensure(n + 2), wrow.ensure(n + 2), pos.ensure(n + 2);
    HIP_CHECK(hipMemsetAsync(flag.p, 0, (size_t)n * sizeof(u32), st));
    hipLaunchKernelGGL(k_rbh_run_wave, dim3((nruns + 3u) / 4u), dim3(256), 0, st, rstart.p, nruns, all_long ? 1 : 0, q, s, score, d_tax.p, flag.p, wrow.p);
    DevBuf<u32> d_lrun, d_loff, lval;
    DevBuf<u64> lkey;
    SortedGroups lg;
    if (!lrun.empty()) {
        const u32 NL = (u32)nlong;   // <= n < 2^31
        upload(d_lrun, lrun.data(), lrun.size(), st), upload(d_loff, loff.data(), loff.size(), st);
        lkey.ensure((size_t)NL + 2), lval.ensure((size_t)NL + 2);
        hipLaunchKernelGGL(k_rbh_long_keys, dim3((u32)lrun.size()), dim3(256), 0, st, d_lrun.p, d_loff.p, rstart.p, s, d_tax.p, T, lkey.p, lval.p);
        lg.sort(call, lkey.p, lval.p, NL, ceil_log2((u64)lrun.size() * T));
        lg.segments(call, NL);
        hipLaunchKernelGGL(k_rbh_seg_max, dim3((lg.nseg + 3u) / 4u), dim3(256), 0, st, lg.start.p, lg.nseg, lg.skey.p, lg.sidx.p, d_lrun.p, rstart.p, q, score, d_tax.p, T,
                           flag.p, wrow.p);
    }
    const u32* d_nw = scan_u32(flag.p, pos.p, n, false, tmp.p, st);
    HIP_CHECK(hipGetLastError());
    const u32 nw = call.read(d_nw);
    out->n_winners = nw;
    if (!nw) return;
    wq.ensure(nw + 2), ws.ensure(nw + 2);
    hipLaunchKernelGGL(k_rbh_winners, grid256(n), dim3(256), 0, st, n, flag.p, pos.p, wrow.p, q, s, wq.p, ws.p);

    // ---- pairs
    {
        DevBuf<u64> key;
        DevBuf<u32> idx, even, epos, etmp;
        DevBuf<int> oa, ob;
        SortedGroups g;
        key.ensure(nw + 2), idx.ensure(nw + 2), even.ensure(nw + 2), epos.ensure(nw + 2), etmp.ensure(scan_u32_temp_elems(nw) + 2);
        hipLaunchKernelGGL(k_rbh_pair_keys, grid256(nw), dim3(256), 0, st, nw, wq.p, ws.p, M, key.p, idx.p);
        g.sort(call, key.p, idx.p, nw, ceil_log2(M * M));
        g.segments(call, nw);
        hipLaunchKernelGGL(k_rbh_even, grid256(nw), dim3(256), 0, st, nw, g.sidx.p, g.rid.p, g.start.p, even.p);
        const u32* d_ne = scan_u32(even.p, epos.p, nw, false, etmp.p, st);
        HIP_CHECK(hipGetLastError());
        const u32 ne = call.read(d_ne);
        oa.ensure(ne + 2), ob.ensure(ne + 2);
        hipLaunchKernelGGL(k_rbh_pair_emit, grid256(nw), dim3(256), 0, st, nw, even.p, epos.p, wq.p, ws.p, oa.p, ob.p);
        HIP_CHECK(hipGetLastError());
        out->rbh_a = host_copy(who, oa.p, ne, st), out->rbh_b = host_copy(who, ob.p, ne, st);
        call.wait();   // (the buffers of this block go away here)
        out->n_rbh = ne;
    }
    if (R < 0) return;

    // ---- core table
    DevBuf<u32> first, gflag, gpos, last;
    DevBuf<int> gene, fwd;
    DevBuf<u8> rec;
    first.ensure((size_t)M + 2), gflag.ensure(nw + 2), gpos.ensure(nw + 2);
    HIP_CHECK(hipMemsetAsync(first.p, 0xFF, (size_t)M * sizeof(u32), st));
    hipLaunchKernelGGL(k_rbh_first, grid256(nw), dim3(256), 0, st, nw, wq.p, d_tax.p, R, first.p);
    hipLaunchKernelGGL(k_rbh_gene_flag, grid256(nw), dim3(256), 0, st, nw, wq.p, d_tax.p, R, first.p, gflag.p);
    const u32* d_nc = scan_u32(gflag.p, gpos.p, nw, false, tmp.p, st);   // (tmp: sized for n >= nw)
    HIP_CHECK(hipGetLastError());
    const u32 nc = call.read(d_nc);
    if (!nc) return;
    if ((u64)nc * T >= (1ull << 31)) throw SoError(std::string(who) + ": a core table of 2^31 cells and more (genes x taxa) is not supported");
    const u32 cells = nc * T;
    gene.ensure(nc + 2), last.ensure((size_t)cells + 2), fwd.ensure((size_t)cells + 2), rec.ensure((size_t)cells + 2);
    // (gflag was computed from first: only now may the genes' rows overwrite their first positions; every other word becomes "no row")
    HIP_CHECK(hipMemsetAsync(first.p, 0xFF, (size_t)M * sizeof(u32), st));
    HIP_CHECK(hipMemsetAsync(last.p, 0, (size_t)cells * sizeof(u32), st));
    HIP_CHECK(hipMemsetAsync(rec.p, 0, (size_t)cells, st));
    hipLaunchKernelGGL(k_rbh_gene_emit, grid256(nw), dim3(256), 0, st, nw, gflag.p, gpos.p, wq.p, gene.p, first.p);
    hipLaunchKernelGGL(k_rbh_last, grid256(nw), dim3(256), 0, st, nw, wq.p, ws.p, d_tax.p, R, T, first.p, last.p);
    hipLaunchKernelGGL(k_rbh_fwd, grid256(cells), dim3(256), 0, st, cells, last.p, ws.p, fwd.p);
    hipLaunchKernelGGL(k_rbh_rec, grid256(nw), dim3(256), 0, st, nw, wq.p, ws.p, d_tax.p, R, T, first.p, fwd.p, rec.p);
    HIP_CHECK(hipGetLastError());
    out->core_gene = host_copy(who, gene.p, nc, st), out->core_fwd = host_copy(who, fwd.p, cells, st), out->core_rec = host_copy(who, rec.p, cells, st);
    call.wait();
    out->n_core = nc;
}

auto slots(so_rbh_result* r) { return result_slots(&r->rbh_a, &r->rbh_b, &r->core_gene, &r->core_fwd, &r->core_rec); }

// what both entry points check before anything touches the device
void rbh_check(const char* who, int device, i64 n, i64 n_names, const int32_t* tax, i64 n_taxa, int ref_taxon, int flags, so_rbh_result* out) {
    if (!out) throw SoError(std::string(who) + ": result pointer is NULL");
    memset(out, 0, sizeof *out);
    hit_table_check(who, n, n_names, tax, n_taxa, [&] {
        if (flags != 0) throw SoError(std::string(who) + ": flags is reserved and must be 0");
        if (n_names >= (1ll << 31) || n_taxa >= (1ll << 31)) throw SoError(std::string(who) + ": 2^31 names or taxa and more are not supported (32-bit codes)");
        if (ref_taxon < -1 || ref_taxon >= n_taxa) throw SoError(std::string(who) + ": ref_taxon lies outside -1 .. n_taxa - 1");
    });
    out->n_taxa = n_taxa;
    check_device(who, device);
}

struct RbhCols {   // the device columns of a call, and the maps they were unpacked through
    DevBuf<int> q, s, qmap, smap;
    DevBuf<double> score;
    DevBuf<u32> err;
};

// what both entry points end with: columns(call, c) brings the n rows to the device, by upload or from the records -- those must be
// complete before this call's own stream reads them: everything queued on the device so far is waited for
template <class Columns>
void rbh_tail(const char* who, int device, bool records, i64 n, i64 n_names, const int32_t* tax, i64 n_taxa, int ref_taxon, so_rbh_result* out, Columns columns) {
    if (n > 0) {
        DeviceCall call(device, records);
        RbhCols c;
        c.err.ensure(4);
        HIP_CHECK(hipMemsetAsync(c.err.p, 0, sizeof(u32), call.st));
        columns(call, c);
        rbh_run(call, (u32)n, c.q.p, c.s.p, c.score.p, n_names, tax, n_taxa, ref_taxon, c.err.p, who, out);
        out->waits = call.waits;
    }
    fill_empty_slots(slots(out));
}

}  // namespace

extern "C" {

const char* so_rbh_last_error(void) { return g_rbh_err.c_str(); }

void so_rbh_free(so_rbh_result* r) {
    if (r) release_slots(r, slots(r));
}

int so_rbh_cols(int device, int64_t n, const int32_t* q, const int32_t* s, const double* score, int64_t n_names, const int32_t* tax, int64_t n_taxa, int32_t ref_taxon,
                int32_t flags, so_rbh_result* out) {
    const char* who = "so_rbh_cols";
    return guarded_call(g_rbh_err, out, so_rbh_free, [&] {
        rbh_check(who, device, n, n_names, tax, n_taxa, ref_taxon, flags, out);
        if (n > 0 && (!q || !s || !score)) throw SoError(std::string(who) + ": a column is NULL");
        rbh_tail(who, device, false, n, n_names, tax, n_taxa, ref_taxon, out, [&](DeviceCall& call, RbhCols& c) {
            const size_t N = (size_t)n;
            upload(c.q, q, N, call.st), upload(c.s, s, N, call.st), upload(c.score, score, N, call.st);
        });
    });
}

int so_rbh_records(int device, const so_hit* d_hits, int64_t n, const int32_t* qmap, int64_t n_q, const int32_t* smap, int64_t n_s, int64_t n_names, const int32_t* tax,
                   int64_t n_taxa, int32_t ref_taxon, int32_t flags, so_rbh_result* out) {
    const char* who = "so_rbh_records";
    return guarded_call(g_rbh_err, out, so_rbh_free, [&] {
        rbh_check(who, device, n, n_names, tax, n_taxa, ref_taxon, flags, out);
        if (n_q < 0 || n_s < 0 || (n_q > 0 && !qmap) || (n_s > 0 && !smap)) throw SoError(std::string(who) + ": bad arguments");
        if (n > 0 && !d_hits) throw SoError(std::string(who) + ": the record pointer is NULL");
        rbh_tail(who, device, true, n, n_names, tax, n_taxa, ref_taxon, out, [&](DeviceCall& call, RbhCols& c) {
            const size_t N = (size_t)n;
            upload(c.qmap, qmap, (size_t)n_q, call.st), upload(c.smap, smap, (size_t)n_s, call.st);
            c.q.ensure(N + 2), c.s.ensure(N + 2), c.score.ensure(N + 2);
            hipLaunchKernelGGL(k_rbh_unpack, grid256(N), dim3(256), 0, call.st, d_hits, (u32)N, c.qmap.p, (i64)n_q, c.smap.p, (i64)n_s, c.q.p, c.s.p, c.score.p, c.err.p);
        });
    });
}

}  // extern "C"
