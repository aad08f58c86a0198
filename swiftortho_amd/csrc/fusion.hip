// fusion.hip -- gene-fusion links on the device (the "Rosetta stone" method, Marcotte et al. 1999, Enright et al. 1999): two proteins that
// are not homologous to each other but align side by side, without overlap, on one composite protein -- what swiftortho_amd/fusion.py
// `fusion_links()` defines, integer for integer.  From the hit rows of a search (columns uploaded from the host, or the so_hit records
// so_search_device left in HBM):
//   * a run = consecutive rows of one query code; a row is ELIGIBLE iff s != q, (sed - sst + 1) * den >= num * slen (64-bit products,
//     equality passes) and, with same_taxon, tax[s] != tax[q];
//   * the REPRESENTATIVE of (run, subject) is the first eligible row of that subject in the run;
//   * x and y are HOMOLOGOUS iff any row of the table holds (q, s) == (x, y) or (y, x);
//   * a LINK is a pair of representatives ra < rb of one run whose query intervals overlap by max_overlap residues at most, whose
//     subjects a, b are of one taxon (same_taxon) and are not homologous; the links as (ra, rb), ascending.
// Integers only; nothing in the output depends on scheduling but the order inside the emit pass, which the sort on the (unique) keys
// row_a << 32 | row_b removes.
//
// Kernels.  k_fu_unpack (records -> columns; hit_codes, hit_table.h).  k_fu_rows: the row checks (a name code outside the table, a bad
// interval: the error word) and the eligibility flag -- tax[] is never indexed with a code that was not checked --, with every row's
// key q << 32 | s.  key_runs -> run_starts (k_util.hip) give the run bounds.  k_fu_reps: a row per lane walks the rows of its run before
// it: a representative is an eligible row that no earlier eligible row of the same subject precedes (the lanes of a run read the same
// earlier row at the same step: a broadcast).  The walks of a run of L ROWS are L^2 / 2 steps at most, whatever its representatives: bounded
// by the rows a search reports per query (-v, 1000 in the wrapper: 0.7 ms for all row stages of 1.6 M rows, profiles/fusion_cost.txt),
// not by the pairs -- a run of 65 537 rows is 2 * 10^9 steps.  scan_u32 over the flags, k_fu_compact packs
// (row, s, qst, qed) of the representatives, 16 bytes each, in row order -- those of a run stand together.  k_fu_runs: per run its first
// slot and m (m - 1) / 2; k_fu_scan64: the exclusive 64-bit scan of those, one workgroup walking the runs with a carry (the run count
// is on the device only).  sort_keys_u64 orders all rows' keys once.
// k_fu_pairs<EMIT>: a fixed grid (what the device holds at a time) strides over the 64-bit pair space.  A lane finds its run by binary
// search in the scan (the last run whose offset is <= t: runs without a pair are passed over), decodes k = t - offset as k = j (j - 1) / 2
// + i, i < j < m -- consecutive lanes hold consecutive i of one j: slot j is a broadcast, the slots i one coalesced read -- applies the
// interval and the taxon test and only then searches the sorted keys for (a, b) and (b, a).  It runs twice: the count pass adds the
// waves' disjoint pairs and links to two 64-bit totals (two adds per wave's whole walk), from which the host applies the refusals and sizes
// the output exactly; the emit pass reserves a workgroup's slots with one add to a cursor per trip and writes row_a << 32 | row_b.  One sort_keys_u64 orders them; k_fu_unpack_links
// splits the keys and gathers what a line of the text needs.
// Two host waits (DeviceCall, device_call.h): the counters, then the result (one when there is no link, none for n = 0).
#include "hit_table.h"
#include "scan64.h"
#include "tree_stage.h"

#include <cstring>
#include <string>

namespace {

constexpr int FU_SCAN_THREADS = 1024;

struct FuRows {   // the device columns of a call
    const int *q, *s, *qst, *qed, *sst, *sed, *slen, *qlen;
};

// so_hit records -> the columns; err |= 1 / 2: a qidx / sidx outside its map
__global__ __launch_bounds__(256) void k_fu_unpack(const so_hit* __restrict__ h, u32 n, const int* __restrict__ qmap, i64 nq, const int* __restrict__ smap, i64 ns,
                                                   int* __restrict__ q, int* __restrict__ s, int* __restrict__ qst, int* __restrict__ qed, int* __restrict__ sst,
                                                   int* __restrict__ sed, int* __restrict__ slen, int* __restrict__ qlen, u32* __restrict__ err) {
    const size_t i = tid256();
    if (i >= n) return;
    int qc, sc;
    hit_codes(h[i], qmap, nq, smap, ns, qc, sc, err);
    q[i] = qc, s[i] = sc, qst[i] = h[i].qst, qed[i] = h[i].qed, sst[i] = h[i].sst, sed[i] = h[i].sed, slen[i] = h[i].slen, qlen[i] = h[i].qlen;
}

// err |= 4: a name code outside [0, n_names); err |= 8: qst < 1, qed < qst, sst < 1, sed < sst or slen < 0.  elig[i], key[i] = q << 32 | s
// (a row with a code outside the table is not eligible and its taxon is never read); cnt[0] += the eligible rows
__global__ __launch_bounds__(256) void k_fu_rows(u32 n, FuRows c, i64 n_names, const int* __restrict__ tax, i64 num, i64 den, int same_taxon, u32* __restrict__ elig,
                                                 u64* __restrict__ key, u32* __restrict__ err, ull* __restrict__ cnt) {
    const size_t i = tid256();
    bool ok = false;
    if (i < n) {
        const int q = c.q[i], s = c.s[i];
        const i64 sst = c.sst[i], sed = c.sed[i], slen = c.slen[i];
        key[i] = ((u64)(u32)q << 32) | (u64)(u32)s;
        if (c.qst[i] < 1 || c.qed[i] < c.qst[i] || sst < 1 || sed < sst || slen < 0) atomicOr(err, 8u);
        if (q < 0 || q >= n_names || s < 0 || s >= n_names) atomicOr(err, 4u);
        else ok = s != q && (sed - sst + 1) * den >= num * slen && (!same_taxon || tax[s] != tax[q]);
        elig[i] = ok ? 1u : 0u;
    }
    const ull ne = (ull)__popcll(__ballot(ok));   // (every lane of the wave is here)
    if ((threadIdx.x & 63u) == 0 && ne) atomicAdd(cnt, ne);
}

// rep[i] = 1: row i is eligible and no eligible row of its subject stands before it in its run (rid: the run of every row, from 1).
// An eligible lane walks up to every earlier row of its run: quadratic in the run's ROWS, bounded by the search's rows per query
__global__ __launch_bounds__(256) void k_fu_reps(u32 n, const u32* __restrict__ rid, const u32* __restrict__ rstart, const int* __restrict__ s,
                                                 const u32* __restrict__ elig, u32* __restrict__ rep) {
    const size_t i = tid256();
    if (i >= n) return;
    u32 first = elig[i];
    if (first) {
        const int si = s[i];
        for (u32 j = rstart[rid[i] - 1u]; j < (u32)i; ++j)
            if (s[j] == si && elig[j]) {
                first = 0u;
                break;
            }
    }
    rep[i] = first;
}

// representative i -> slot pos[i] (the exclusive scan of rep: row order, a run's slots together)
__global__ __launch_bounds__(256) void k_fu_compact(u32 n, const u32* __restrict__ rep, const u32* __restrict__ pos, const int* __restrict__ s, const int* __restrict__ qst,
                                                    const int* __restrict__ qed, int4* __restrict__ slot) {
    const size_t i = tid256();
    if (i < n && rep[i]) slot[pos[i]] = make_int4((int)i, s[i], qst[i], qed[i]);
}

// run r: its first slot and the pairs of its m representatives
__global__ __launch_bounds__(256) void k_fu_runs(u32 n, const u32* __restrict__ d_nruns, const u32* __restrict__ rstart, const u32* __restrict__ pos,
                                                 const u32* __restrict__ d_nreps, u32* __restrict__ first, u64* __restrict__ npair) {
    const size_t r = tid256();
    if (r >= *d_nruns) return;
    const u32 b = rstart[r], e = rstart[r + 1];   // b < e <= n
    const u32 lo = pos[b], hi = e < n ? pos[e] : *d_nreps;
    const u64 m = hi - lo;
    first[r] = lo, npair[r] = m * (m - (m ? 1u : 0u)) / 2u;
}

// off[r] = the pairs of the runs before r, off[*d_nruns] = *total = all pairs: one workgroup walks the runs with a carry, as
// k_scan_blocksums64 (k_util.hip) walks block sums, on the workgroup scan they share (scan64.h) -- here the count is a device word (no
// wait has told the host how many runs there are) and the offsets go to an array of their own, with the closing one
__global__ __launch_bounds__(FU_SCAN_THREADS) void k_fu_scan64(const u32* __restrict__ d_nruns, const u64* __restrict__ v, u64* __restrict__ off, ull* __restrict__ total) {
    __shared__ u64 s_w[FU_SCAN_THREADS / 64];
    const u32 nr = *d_nruns;
    u64 carry = 0;
    for (u32 i0 = 0; i0 < nr; i0 += FU_SCAN_THREADS) {   // (the same trips for every lane: all of them meet the barriers)
        const u32 i = i0 + threadIdx.x;
        u64 tot;
        const u64 ex = block_excl_scan_u64<FU_SCAN_THREADS>(i < nr ? v[i] : 0ull, s_w, &tot);
        if (i < nr) off[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) off[nr] = carry, *total = carry;
}

// is `k` among the n ascending keys?
__device__ __forceinline__ bool fu_has_key(const u64* __restrict__ skey, u32 n, u64 k) {
    u32 a = 0, b = n;
    while (a < b) {
        const u32 m = a + (b - a) / 2u;
        if (skey[m] < k)
            a = m + 1u;
        else
            b = m;
    }
    return a < n && skey[a] == k;
}

// k < m (m - 1) / 2 -> the j with j (j - 1) / 2 <= k < (j + 1) j / 2: the root in floating point, then made exact in integers
__device__ __forceinline__ u64 fu_tri_row(u64 k) {
    u64 j = k < (1ull << 22) ? (u64)((1.f + sqrtf((float)(8ull * k + 1ull))) * .5f) : (u64)((1. + sqrt((double)(8ull * k + 1ull))) * .5);
    if (j < 1) j = 1;
    while (j * (j - 1u) / 2u > k) --j;
    while ((j + 1u) * j / 2u <= k) ++j;
    return j;
}

// tot[0]: the pairs that pass the interval and the taxon test, tot[1]: the links (count pass); tot[2]: the emit pass's cursor; cap: the
// slots of `out` (the count pass's links: no store lands beyond it).  Every lane of a workgroup makes the same trips, so a wave's
// lanes meet at every ballot and a workgroup's at every barrier.  Both passes were bound by their adds to ONE address -- a wave's two
// adds per trip in the count pass took twice the emit pass's one (9.6 ms against 4.8 ms for the same walk of 9.3 * 10^7 pairs; the count
// pass run twice took the same time twice, so it was not a matter of coming first) --, hence the sums kept per wave and the slots
// reserved per workgroup.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_fu_pairs(const u32* __restrict__ d_nruns, const u64* __restrict__ off, const u32* __restrict__ first,
                                                  const int4* __restrict__ slot, const int* __restrict__ tax, const u64* __restrict__ skey, u32 n, i64 max_overlap,
                                                  int same_taxon, ull* __restrict__ tot, u64* __restrict__ out, u32 cap) {
    const u32 nr = *d_nruns;
    const u64 P = off[nr], step = (u64)gridDim.x * 256u;
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    __shared__ u32 s_cnt[2][4];
    __shared__ ull s_base[2];
    ull nd = 0, nl = 0;
    u32 trip = 0;
    for (u64 t0 = (u64)blockIdx.x * 256u; t0 < P; t0 += step, ++trip) {
        const u64 t = t0 + threadIdx.x;
        bool disjoint = false, link = false;
        u64 rows = 0;
        if (t < P) {
            u32 a = 0, b = nr;   // the last run with off[r] <= t (off[0] = 0)
            while (b - a > 1u) {
                const u32 m = a + (b - a) / 2u;
                if (off[m] <= t)
                    a = m;
                else
                    b = m;
            }
            const u64 k = t - off[a];
            const u64 j = fu_tri_row(k), i = k - j * (j - 1u) / 2u;   // i < j < m
            const int4 x = slot[first[a] + (u32)i], y = slot[first[a] + (u32)j];   // (row, s, qst, qed); x.x < y.x
            const i64 overlap = (i64)min(x.w, y.w) - (i64)max(x.z, y.z) + 1;
            disjoint = overlap <= max_overlap && (!same_taxon || tax[x.y] == tax[y.y]);
            if (disjoint) {
                const u64 ka = (u64)(u32)x.y, kb = (u64)(u32)y.y;
                link = !fu_has_key(skey, n, (ka << 32) | kb) && !fu_has_key(skey, n, (kb << 32) | ka);
                rows = ((u64)(u32)x.x << 32) | (u64)(u32)y.x;
            }
        }
        const ull ml = __ballot(link);
        if (!EMIT) {   // a wave keeps its two sums over its whole walk: two adds per wave, not per trip
            nd += (ull)__popcll(__ballot(disjoint)), nl += (ull)__popcll(ml);
        } else {       // the workgroup's four waves reserve their slots with ONE add per trip; the LDS words alternate between trips
            const u32 par = trip & 1u;
            if (lane == 0) s_cnt[par][w] = (u32)__popcll(ml);
            __syncthreads();
            const u32 c0 = s_cnt[par][0], c1 = s_cnt[par][1], c2 = s_cnt[par][2], c3 = s_cnt[par][3];
            if (threadIdx.x == 0 && c0 + c1 + c2 + c3) s_base[par] = atomicAdd(tot + 2, (ull)(c0 + c1 + c2 + c3));
            __syncthreads();   // (a wave two trips ahead would write these words again: it cannot pass the next trip's first barrier before all have read)
            const ull p = s_base[par] + (w > 0 ? c0 : 0u) + (w > 1 ? c1 : 0u) + (w > 2 ? c2 : 0u) + (ull)__popcll(ml & ((1ull << lane) - 1ull));
            if (link && p < cap) out[p] = rows;
        }
    }
    if (!EMIT && lane == 0) {
        if (nd) atomicAdd(tot, nd);
        if (nl) atomicAdd(tot + 1, nl);
    }
}

// sorted keys -> row_a, row_b and the eight numbers of a line: q, a, b, qst_a, qed_a, qst_b, qed_b, qlen
__global__ __launch_bounds__(256) void k_fu_unpack_links(u32 nl, const u64* __restrict__ skey, FuRows c, int* __restrict__ row_a, int* __restrict__ row_b,
                                                         int* __restrict__ link) {
    const size_t i = tid256();
    if (i >= nl) return;
    const u32 ra = (u32)(skey[i] >> 32), rb = (u32)skey[i];
    row_a[i] = (int)ra, row_b[i] = (int)rb;
    int* l = link + i * 8u;
    l[0] = c.q[ra], l[1] = c.s[ra], l[2] = c.s[rb], l[3] = c.qst[ra], l[4] = c.qed[ra], l[5] = c.qst[rb], l[6] = c.qed[rb], l[7] = c.qlen[ra];
}

thread_local std::string g_fusion_err;

auto slots(so_fusion_result* r) { return result_slots(&r->row_a, &r->row_b, &r->link); }

struct FuCols {   // the device columns of a call, and the maps they were unpacked through
    DevBuf<int> q, s, qst, qed, sst, sed, slen, qlen, qmap, smap;
    DevBuf<u32> err;
    FuRows rows() const { return FuRows{q.p, s.p, qst.p, qed.p, sst.p, sed.p, slen.p, qlen.p}; }
};

// what both entry points check before anything touches the device
void fusion_check(const std::string& who, int device, i64 n, i64 n_names, const int32_t* tax, i64 n_taxa, i64 max_overlap, int num, int den, int flags,
                  so_fusion_result* out) {
    if (!out) throw SoError(who + ": result pointer is NULL");
    memset(out, 0, sizeof *out);
    hit_table_check(who.c_str(), n, n_names, tax, n_taxa, [&] {
        if (flags & ~3) throw SoError(who + ": unknown flag bits (bit 0: components of one taxon that is not the composite's, bit 1: the stages timed by events)");
        if (n_names >= (1ll << 31) || n_taxa >= (1ll << 31)) throw SoError(who + ": 2^31 names or taxa and more are not supported (32-bit codes)");
        if (max_overlap < 0 || max_overlap >= (1ll << 31)) throw SoError(who + ": max_overlap lies in 0 .. 2^31 - 1 (it is " + std::to_string(max_overlap) + ")");
        if (num < 0 || num > den || den < 1 || den >= (1 << 20))
            throw SoError(who + ": the subject coverage num / den needs 0 <= num <= den < 2^20, den above 0 (they are " + std::to_string(num) + " and " +
                          std::to_string(den) + ")");
    });
    check_device(who.c_str(), device);
}

// the stage on the device columns of n > 0 rows
void fusion_run(DeviceCall& call, const std::string& who, int device, u32 n, const FuCols& c, i64 n_names, const int32_t* tax, i64 max_overlap, int num, int den, int flags,
                so_fusion_result* out) {
    hipStream_t st = call.st;
    const char* w = who.c_str();
    const int same_taxon = flags & 1;
    const FuRows rows = c.rows();
    StageEvents ev((flags & 2) != 0);   // marks 0 .. 4 around the row stages, the key sort, the count pass and (a timed call only) the count pass once more; 5 .. 7 around the emit pass and the sort
    DevBuf<int> d_tax;
    DevBuf<u32> head, rid, rstart, tmp, tmp2, elig, rep, pos, first;
    DevBuf<u64> key, skey, npair, off;
    DevBuf<ull> tot;
    DevBuf<int4> slot;
    DevBuf<u8> sort_tmp;
    upload(d_tax, tax, (size_t)n_names, st);
    const size_t N = n;
    head.ensure(N + 2), rid.ensure(N + 2), rstart.ensure(N + 3), tmp.ensure(scan_u32_temp_elems(N) + 2), tmp2.ensure(scan_u32_temp_elems(N) + 2);
    elig.ensure(N + 2), rep.ensure(N + 2), pos.ensure(N + 2), first.ensure(N + 2), key.ensure(N + 2), skey.ensure(N + 2), npair.ensure(N + 2), off.ensure(N + 3);
    slot.ensure(N + 2), tot.ensure(8);
    const int key_bits = 32 + ceil_log2((u64)std::max<i64>(n_names, 1));
    const size_t key_sort_bytes = sort_keys_u64_temp_bytes(N, key_bits);
    sort_tmp.ensure(key_sort_bytes + 16);
    HIP_CHECK(hipMemsetAsync(tot.p, 0, 7 * sizeof(ull), st));   // disjoint pairs, links, the emit cursor, eligible rows, all pairs; [5], [6]: the repeated count of a timed call
    // the grid of k_fu_pairs: as many workgroups as the device holds at a time (the runtime's occupancy figure)
    int cus = 0, per_cu = 0;
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_fu_pairs<true>, 256, 0));
    const dim3 pair_grid((u32)(std::max(cus, 1) * std::max(per_cu, 1)));

    ev.mark(0, st);
    hipLaunchKernelGGL(k_fu_rows, grid256(N), dim3(256), 0, st, n, rows, n_names, d_tax.p, (i64)num, (i64)den, same_taxon, elig.p, key.p, c.err.p, tot.p + 3);
    const u32* d_nruns = key_runs(rows.q, n, head.p, rid.p, tmp.p, st);   // (tmp is not scanned with again: the word stays)
    run_starts(head.p, rid.p, n, d_nruns, rstart.p, st);
    hipLaunchKernelGGL(k_fu_reps, grid256(N), dim3(256), 0, st, n, rid.p, rstart.p, rows.s, elig.p, rep.p);
    const u32* d_nreps = scan_u32(rep.p, pos.p, N, false, tmp2.p, st);
    hipLaunchKernelGGL(k_fu_compact, grid256(N), dim3(256), 0, st, n, rep.p, pos.p, rows.s, rows.qst, rows.qed, slot.p);
    hipLaunchKernelGGL(k_fu_runs, grid256(N), dim3(256), 0, st, n, d_nruns, rstart.p, pos.p, d_nreps, first.p, npair.p);
    hipLaunchKernelGGL(k_fu_scan64, dim3(1), dim3(FU_SCAN_THREADS), 0, st, d_nruns, npair.p, off.p, tot.p + 4);
    ev.mark(1, st);
    sort_keys_u64(sort_tmp.p, key_sort_bytes, key.p, skey.p, N, 0, key_bits, st);
    ev.mark(2, st);
    hipLaunchKernelGGL(k_fu_pairs<false>, pair_grid, dim3(256), 0, st, d_nruns, off.p, first.p, slot.p, d_tax.p, skey.p, n, max_overlap, same_taxon, tot.p, (u64*)nullptr, 0u);
    ev.mark(3, st);
    if (ev.on) {   // the same pass on the same data once more, into totals nobody reads: what the first one pays for coming first
        hipLaunchKernelGGL(k_fu_pairs<false>, pair_grid, dim3(256), 0, st, d_nruns, off.p, first.p, slot.p, d_tax.p, skey.p, n, max_overlap, same_taxon, tot.p + 5, (u64*)nullptr, 0u);
        ev.mark(4, st);
    }
    HIP_CHECK(hipGetLastError());
    u32 err = 0, nruns = 0, nreps = 0;
    ull t4[5] = {0, 0, 0, 0, 0};
    call.fetch(&err, c.err.p), call.fetch(&nruns, d_nruns), call.fetch(&nreps, d_nreps), call.fetch(t4, tot.p, 5);
    call.wait();   // the counters
    out->waits = call.waits;
    hit_table_errors(w, err);
    if (err & 8u) throw SoError(who + ": a row with qst < 1, qed < qst, sst < 1, sed < sst or slen < 0");
    const u64 P = t4[4];
    out->n_runs = nruns, out->n_eligible = (i64)t4[3], out->n_reps = nreps, out->n_pairs = (i64)P, out->n_disjoint = (i64)t4[0];
    out->prep_ms = ev.ms(0), out->keys_ms = ev.ms(1), out->count_ms = ev.ms(2), out->count_again_ms = ev.ms(3);
    const u64 links = t4[1];
    if (links >= (1ull << 31)) throw SoError(who + ": " + std::to_string(links) + " links: 2^31 and more are not supported (raise the coverage, lower max_overlap)");
    if (links == 0) return;
    const u32 NL = (u32)links;
    const int row_bits = 32 + ceil_log2((u64)n);
    const size_t sort_bytes = sort_keys_u64_temp_bytes(NL, row_bits);
    {   // keys before and after the sort, the result columns, the sort's scratch
        const size_t bytes = (size_t)NL * (2 * sizeof(u64) + 10 * sizeof(int)) + sort_bytes;
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        if (bytes + bytes / 8 > free_b / 2)
            throw SoError(who + ": the " + std::to_string(NL) + " links and their sort would take " + std::to_string(bytes) +
                          " bytes, more than half of the free device memory (" + std::to_string(free_b) + " bytes free): raise the coverage, lower max_overlap");
    }
    DevBuf<u64> lkey, lskey;
    DevBuf<u8> lsort;
    DevBuf<int> d_a, d_b, d_link;
    lkey.ensure((size_t)NL + 2), lskey.ensure((size_t)NL + 2), lsort.ensure(sort_bytes + 16);
    d_a.ensure((size_t)NL + 2), d_b.ensure((size_t)NL + 2), d_link.ensure((size_t)NL * 8 + 2);
    ev.mark(5, st);
    hipLaunchKernelGGL(k_fu_pairs<true>, pair_grid, dim3(256), 0, st, d_nruns, off.p, first.p, slot.p, d_tax.p, skey.p, n, max_overlap, same_taxon, tot.p, lkey.p, NL);
    ev.mark(6, st);
    sort_keys_u64(lsort.p, sort_bytes, lkey.p, lskey.p, NL, 0, row_bits, st);
    ev.mark(7, st);
    hipLaunchKernelGGL(k_fu_unpack_links, grid256(NL), dim3(256), 0, st, NL, lskey.p, rows, d_a.p, d_b.p, d_link.p);
    HIP_CHECK(hipGetLastError());
    call.fetch(t4, tot.p, 5);
    static_assert(sizeof(int) == sizeof(int32_t), "the rows are copied out as int32");
    out->row_a = host_copy(w, d_a.p, (size_t)NL, st), out->row_b = host_copy(w, d_b.p, (size_t)NL, st), out->link = host_copy(w, d_link.p, (size_t)NL * 8, st);
    call.wait();   // the result
    out->waits = call.waits;
    if (t4[2] != links) throw SoError(who + ": the emit pass wrote " + std::to_string(t4[2]) + " links where the count pass found " + std::to_string(links));
    out->n_links = NL;
    out->emit_ms = ev.ms(5), out->sort_ms = ev.ms(6);
}

// what both entry points end with: columns(call, c) brings the n rows to the device, by upload or from the records
template <class Columns>
void fusion_tail(const std::string& who, int device, bool records, i64 n, i64 n_names, const int32_t* tax, i64 max_overlap, int num, int den, int flags,
                 so_fusion_result* out, Columns columns) {
    if (n > 0) {
        DeviceCall call(device, records);
        FuCols c;
        c.err.ensure(4);
        HIP_CHECK(hipMemsetAsync(c.err.p, 0, sizeof(u32), call.st));
        columns(call, c);
        fusion_run(call, who, device, (u32)n, c, n_names, tax, max_overlap, num, den, flags, out);
    }
    fill_empty_slots(slots(out));
}

}  // namespace

extern "C" {

const char* so_fusion_last_error(void) { return g_fusion_err.c_str(); }

void so_fusion_free(so_fusion_result* r) {
    if (r) release_slots(r, slots(r));
}

int so_fusion_cols(int device, int64_t n, const int32_t* q, const int32_t* s, const int32_t* qst, const int32_t* qed, const int32_t* sst, const int32_t* sed,
                   const int32_t* slen, const int32_t* qlen, int64_t n_names, const int32_t* tax, int64_t n_taxa, int64_t max_overlap, int32_t num, int32_t den,
                   int32_t flags, so_fusion_result* out) {
    const std::string who = "so_fusion_cols";
    return guarded_call(g_fusion_err, out, so_fusion_free, [&] {
        fusion_check(who, device, n, n_names, tax, n_taxa, max_overlap, num, den, flags, out);
        if (n > 0 && (!q || !s || !qst || !qed || !sst || !sed || !slen || !qlen)) throw SoError(who + ": a column is NULL");
        fusion_tail(who, device, false, n, n_names, tax, max_overlap, num, den, flags, out, [&](DeviceCall& call, FuCols& c) {
            const size_t N = (size_t)n;
            upload(c.q, q, N, call.st), upload(c.s, s, N, call.st), upload(c.qst, qst, N, call.st), upload(c.qed, qed, N, call.st);
            upload(c.sst, sst, N, call.st), upload(c.sed, sed, N, call.st), upload(c.slen, slen, N, call.st), upload(c.qlen, qlen, N, call.st);
        });
    });
}

int so_fusion_records(int device, const so_hit* d_hits, int64_t n, const int32_t* qmap, int64_t n_q, const int32_t* smap, int64_t n_s, int64_t n_names,
                      const int32_t* tax, int64_t n_taxa, int64_t max_overlap, int32_t num, int32_t den, int32_t flags, so_fusion_result* out) {
    const std::string who = "so_fusion_records";
    return guarded_call(g_fusion_err, out, so_fusion_free, [&] {
        fusion_check(who, device, n, n_names, tax, n_taxa, max_overlap, num, den, flags, out);
        if (n_q < 0 || n_s < 0 || (n_q > 0 && !qmap) || (n_s > 0 && !smap)) throw SoError(who + ": bad arguments");
        if (n > 0 && !d_hits) throw SoError(who + ": the record pointer is NULL");
        fusion_tail(who, device, true, n, n_names, tax, max_overlap, num, den, flags, out, [&](DeviceCall& call, FuCols& c) {
            const size_t N = (size_t)n;
            upload(c.qmap, qmap, (size_t)n_q, call.st), upload(c.smap, smap, (size_t)n_s, call.st);
            c.q.ensure(N + 2), c.s.ensure(N + 2), c.qst.ensure(N + 2), c.qed.ensure(N + 2), c.sst.ensure(N + 2), c.sed.ensure(N + 2), c.slen.ensure(N + 2),
                c.qlen.ensure(N + 2);
            hipLaunchKernelGGL(k_fu_unpack, grid256(N), dim3(256), 0, call.st, d_hits, (u32)N, c.qmap.p, (i64)n_q, c.smap.p, (i64)n_s, c.q.p, c.s.p, c.qst.p, c.qed.p,
                               c.sst.p, c.sed.p, c.slen.p, c.qlen.p, c.err.p);
        });
    });
}

}  // extern "C"
