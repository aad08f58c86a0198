// operon.hip -- the operon pairs of scripts/operon_cluster.py on the device: from the distinct indexed families of every operon (a CSR,
// swiftortho_amd/operon.py `operon_table()`) to what `candidate_pairs()` defines -- every pair of operons (i, j), i == j included, that
// shares an indexed family, with nshr = the indexed families they share (+ 1 when both hold a gene of family 0), either all of them in
// the order in which j first occurs in the concatenation of the operon lists of i's families, or the pairs that pass the script's filter
// (nshr > 2 and 2 * nshr > min(length[i], length[j])) in (i, j) order.  The score is float arithmetic and stays on the host.
//
// The job is a sparse boolean product (operon x family times its transpose) with a threshold; integers only.  One path, in batches:
//   inverted index   k_operon_fam_keys -> SortedGroups (device_call.h: stable sort of (family, entry ordinal), segments) ->
//                    k_operon_lists: the operons of every family, ascending (the sort is stable), and per entry the bounds of its
//                    family's list;
//   batches          the host sums, per operon, the list lengths of its families (64 bits) and cuts the operons into consecutive
//                    batches whose expansions stay within the budget (tune.h SOHIT_OPERON_EXPAND; an operon above it is a batch of its
//                    own);
//   expansion        scan of the batch's list lengths, k_operon_expand: ONE LANE PER OUTPUT ELEMENT -- the lane finds its entry by
//                    binary search in the scan and writes key = (i - batch_lo) << 32 | j, payload = rank (the entry's place in i's
//                    slice).  Coalesced writes whatever the skew of the family sizes: a family held by every operon costs what its
//                    expansions cost, no lane or wave walks a list alone;
//   reduction        SortedGroups sort on the true bit count + segments: a run of equal keys is one pair, its length the shared indexed
//                    families, its first payload the pair's smallest rank (the expansion is emitted in (i, rank, j) order, the sort is
//                    stable).  k_operon_pairs adds has0[i] & has0[j] and tests the filter;
//   output           passing pairs: flag -> scan -> k_operon_compact (already in (i, j) order); all candidates: a second stable sort of
//                    the pairs by (i, rank), k_operon_gather; the candidates per operon are counted with integer atomics.
// Nothing depends on scheduling.  Every host wait goes through the call's DeviceCall and is counted: per batch the run count, in the
// passing-pairs mode the number of survivors, and the batch's rows.
#include "device_call.h"
#include "../../include/sohit.h"

#include <cstring>
#include <string>
#include <vector>

namespace {

typedef unsigned long long ull;

__global__ __launch_bounds__(256) void k_operon_fam_keys(u32 E, const int* __restrict__ fam, u64* __restrict__ key, u32* __restrict__ idx) {
    const size_t e = tid256();
    if (e < E) key[e] = (u64)(u32)fam[e], idx[e] = (u32)e;
}

// position p of the sorted index: lop[p] = the operon listed there; the entry standing there learns its family's list
__global__ __launch_bounds__(256) void k_operon_lists(u32 E, const u32* __restrict__ sidx, const u32* __restrict__ rid, const u32* __restrict__ gstart,
                                                      const u32* __restrict__ eop, u32* __restrict__ lop, u32* __restrict__ lbeg, u32* __restrict__ llen) {
    const size_t p = tid256();
    if (p >= E) return;
    const u32 e = sidx[p], g = rid[p] - 1u, b = gstart[g];
    lop[p] = eop[e], lbeg[e] = b, llen[e] = gstart[g + 1u] - b;
}

// one lane per expansion t < X of the batch's entries e0 .. e0 + nE - 1; off = exclusive scan of their list lengths (all >= 1: an entry
// stands in its own family's list), so the entry of t is the last one whose offset is <= t
__global__ __launch_bounds__(256) void k_operon_expand(u32 X, u32 nE, u32 e0, u32 lo, const u32* __restrict__ off, const u32* __restrict__ lbeg,
                                                       const u32* __restrict__ lop, const u32* __restrict__ eop, const u32* __restrict__ ostart,
                                                       u64* __restrict__ key, u32* __restrict__ val) {
    const size_t t = tid256();
    if (t >= X) return;
    u32 a = 0, b = nE;
    while (b - a > 1u) {
        const u32 m = a + (b - a) / 2u;
        if (off[m] <= (u32)t)
            a = m;
        else
            b = m;
    }
    const u32 e = e0 + a, i = eop[e];
    key[t] = ((u64)(i - lo) << 32) | (u64)lop[lbeg[e] + ((u32)t - off[a])];
    val[t] = e - ostart[i];
}

// one lane per run of the sorted keys = per pair.  all: the pair's key of the second sort, its operon's candidate counter and the number
// of pairs that pass; otherwise the pass flag
__global__ __launch_bounds__(256) void k_operon_pairs(u32 nruns, const u32* __restrict__ rstart, const u64* __restrict__ skey, const u32* __restrict__ srank, u32 lo,
                                                      const int* __restrict__ length, const u8* __restrict__ has0, int all, int rank_bits, int* __restrict__ pi,
                                                      int* __restrict__ pj, int* __restrict__ pn, u32* __restrict__ flag, u64* __restrict__ key2,
                                                      u32* __restrict__ idx2, u32* __restrict__ cnt, ull* __restrict__ npass) {
    const size_t r = tid256();
    bool pass = false;
    if (r < nruns) {
        const u32 b = rstart[r];
        const u64 k = skey[b];
        const u32 il = (u32)(k >> 32), i = lo + il, j = (u32)k;
        const int n = (int)(rstart[r + 1] - b) + ((has0[i] != 0 && has0[j] != 0) ? 1 : 0);
        pass = n > 2 && 2 * n > min(length[i], length[j]);
        pi[r] = (int)i, pj[r] = (int)j, pn[r] = n;
        if (all) {
            key2[r] = ((u64)il << rank_bits) | (u64)srank[b];
            idx2[r] = (u32)r;
            atomicAdd(cnt + il, 1u);
        } else {
            flag[r] = pass ? 1u : 0u;
        }
    }
    if (all) {   // (every lane of the wave is here)
        const ull np = (ull)__popcll(__ballot(pass));
        if ((threadIdx.x & 63u) == 0 && np) atomicAdd(npass, np);
    }
}

__global__ __launch_bounds__(256) void k_operon_compact(u32 nruns, const u32* __restrict__ flag, const u32* __restrict__ pos, const int* __restrict__ pi,
                                                        const int* __restrict__ pj, const int* __restrict__ pn, int* __restrict__ oi, int* __restrict__ oj,
                                                        int* __restrict__ on) {
    const size_t r = tid256();
    if (r >= nruns || !flag[r]) return;
    const u32 p = pos[r];
    oi[p] = pi[r], oj[p] = pj[r], on[p] = pn[r];
}

__global__ __launch_bounds__(256) void k_operon_gather(u32 nruns, const u32* __restrict__ order, const int* __restrict__ pi, const int* __restrict__ pj,
                                                       const int* __restrict__ pn, int* __restrict__ oi, int* __restrict__ oj, int* __restrict__ on) {
    const size_t p = tid256();
    if (p >= nruns) return;
    const u32 r = order[p];
    oi[p] = pi[r], oj[p] = pj[r], on[p] = pn[r];
}

const u64 OPERON_BATCH_MAX = (1ull << 32) - 16;   // expansions of one batch: 32-bit positions

struct Batch {
    u32 lo, hi;     // operons lo .. hi - 1
    u64 x;          // their expansions
    u32 max_len;    // longest slice among them
};

thread_local std::string g_operon_err;

auto slots(so_operon_result* r) { return result_slots(&r->i, &r->j, &r->nshr, &r->cand_start); }

template <class T>
T* host_copy_of(const char* who, const std::vector<T>& v) {
    T* p = host_array<T>(who, v.size());
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

}  // namespace

extern "C" {

const char* so_operon_last_error(void) { return g_operon_err.c_str(); }

void so_operon_free(so_operon_result* r) {
    if (r) release_slots(r, slots(r));
}

int so_operon_pairs(int device, int64_t n_ops, const int64_t* start, const int32_t* fam, const int32_t* length, const uint8_t* has0, int64_t n_fam, int32_t flags,
                    so_operon_result* out) {
    const std::string who = "so_operon_pairs";
    return guarded_call(g_operon_err, out, so_operon_free, [&] {
        if (!out) throw SoError(who + ": result pointer is NULL");
        memset(out, 0, sizeof *out);
        if (flags & ~1) throw SoError(who + ": unknown flags (bit 0: all candidates in first-occurrence order)");
        if (n_ops < 0 || n_fam < 0) throw SoError(who + ": bad arguments");
        if (n_ops >= (1ll << 31)) throw SoError(who + ": 2^31 operons and more are not supported");
        if (n_fam >= (1ll << 31)) throw SoError(who + ": 2^31 families and more are not supported");
        if (n_ops > 0 && (!start || !length || !has0)) throw SoError(who + ": start, length or has0 is NULL");
        const bool all = (flags & 1) != 0;
        const size_t N = (size_t)n_ops;
        if (N && start[0] != 0) throw SoError(who + ": start does not rise from 0");
        for (size_t i = 0; i < N; ++i)
            if (start[i + 1] < start[i]) throw SoError(who + ": start does not rise from 0 (operon " + std::to_string(i) + ")");
        const i64 n_entries = N ? start[N] : 0;
        if (n_entries >= (1ll << 31)) throw SoError(who + ": 2^31 entries and more are not supported");
        if (n_entries > 0 && !fam) throw SoError(who + ": fam is NULL");
        const size_t E = (size_t)n_entries;
        // one pass over fam: the checks, the family sizes, the operon of every entry
        std::vector<u32> fsize((size_t)n_fam, 0u), stamp((size_t)n_fam, 0u), eop(E), ostart(N + 1, 0u);
        for (size_t i = 0; i < N; ++i) {
            if (length[i] < 1) throw SoError(who + ": length[" + std::to_string(i) + "] is below 1");
            ostart[i + 1] = (u32)start[i + 1];
            for (size_t e = (size_t)start[i]; e < (size_t)start[i + 1]; ++e) {
                const i64 f = fam[e];
                if (f < 1 || f >= n_fam) throw SoError(who + ": a family outside 1 .. n_fam - 1 (operon " + std::to_string(i) + ")");
                if (stamp[(size_t)f] == (u32)i + 1u) throw SoError(who + ": a family repeated inside the slice of operon " + std::to_string(i));
                stamp[(size_t)f] = (u32)i + 1u, ++fsize[(size_t)f], eop[e] = (u32)i;
            }
        }
        // the expansions of every operon: the sum of its families' list lengths
        std::vector<u64> tot(N, 0);
        u64 n_exp = 0;
        for (size_t i = 0; i < N; ++i) {
            u64 t = 0;
            for (size_t e = (size_t)start[i]; e < (size_t)start[i + 1]; ++e) t += fsize[(size_t)fam[e]];
            if (t >= OPERON_BATCH_MAX) throw SoError(who + ": operon " + std::to_string(i) + " alone expands to 2^32 - 16 pairs or more");
            tot[i] = t, n_exp += t;
        }
        out->n_ops = n_ops, out->n_expansions = (i64)n_exp;
        check_device(who.c_str(), device);
        const char* w = who.c_str();
        if (E == 0) {   // nothing to launch: no operon has an indexed family
            if (all) out->cand_start = host_copy_of(w, std::vector<int64_t>(N + 1, 0));
            fill_empty_slots(slots(out));
            return;
        }
        DeviceCall call(device);
        hipStream_t st = call.st;
        const u64 budget = call.tn.operon_expand < 1 ? OPERON_EXPAND_DEFAULT : std::min<u64>((u64)call.tn.operon_expand, OPERON_BATCH_MAX - 1);
        std::vector<Batch> batches;
        {
            Batch b = {0u, 0u, 0ull, 0u};
            for (size_t i = 0; i < N; ++i) {
                if (i > b.lo && b.x + tot[i] > budget) {
                    b.hi = (u32)i, batches.push_back(b);
                    b = Batch{(u32)i, 0u, 0ull, 0u};
                }
                b.x += tot[i], b.max_len = std::max(b.max_len, (u32)(start[i + 1] - start[i]));
            }
            b.hi = (u32)N, batches.push_back(b);
        }
        u64 max_x = 0;
        u32 max_ne = 0, max_ops = 0;
        for (const Batch& b : batches)
            max_x = std::max(max_x, b.x), max_ne = std::max(max_ne, ostart[b.hi] - ostart[b.lo]), max_ops = std::max(max_ops, b.hi - b.lo);

        // ---- the inverted index
        const u32 En = (u32)E;
        DevBuf<int> d_fam, d_len;
        DevBuf<u8> d_has0;
        DevBuf<u32> d_eop, d_ostart, lop, lbeg, llen, idx;
        DevBuf<u64> fkey;
        SortedGroups fg;
        upload(d_fam, fam, E, st), upload(d_len, length, N, st), upload(d_has0, has0, N, st), upload(d_eop, eop.data(), E, st);
        upload(d_ostart, ostart.data(), N + 1, st);
        fkey.ensure(E + 2), idx.ensure(E + 2), lop.ensure(E + 2), lbeg.ensure(E + 2), llen.ensure(E + 2);
        hipLaunchKernelGGL(k_operon_fam_keys, grid256(E), dim3(256), 0, st, En, d_fam.p, fkey.p, idx.p);
        fg.sort(call, fkey.p, idx.p, En, ceil_log2((u64)n_fam));
        fg.segments(call, En);
        hipLaunchKernelGGL(k_operon_lists, grid256(E), dim3(256), 0, st, En, fg.sidx.p, fg.rid.p, fg.start.p, d_eop.p, lop.p, lbeg.p, llen.p);
        HIP_CHECK(hipGetLastError());

        // ---- the batches
        DevBuf<u32> off, val, flag, pos, idx2, cnt, tmp;
        DevBuf<u64> key, key2;
        DevBuf<int> pi, pj, pn, oi, oj, on;
        DevBuf<ull> npass;
        SortedGroups g, g2;
        std::vector<int32_t> vi, vj, vn;
        std::vector<int64_t> cstart(all ? N + 1 : 0, 0);
        std::vector<u32> hcnt(all ? max_ops : 0);
        ull h_npass = 0;
        u64 n_cand = 0;
        off.ensure((size_t)max_ne + 2), tmp.ensure(scan_u32_temp_elems((size_t)std::max<u64>(max_x, max_ne)) + 2);
        key.ensure((size_t)max_x + 2), val.ensure((size_t)max_x + 2);
        npass.ensure(2);
        HIP_CHECK(hipMemsetAsync(npass.p, 0, sizeof(ull), st));
        for (const Batch& b : batches) {
            ++out->batches;
            if (b.x == 0) continue;   // operons without an indexed family: no candidates
            const u32 X = (u32)b.x, e0 = ostart[b.lo], nE = ostart[b.hi] - e0, nops = b.hi - b.lo;
            const int op_bits = ceil_log2(nops), rank_bits = ceil_log2(b.max_len);
            scan_u32(llen.p + e0, off.p, nE, false, tmp.p, st);
            hipLaunchKernelGGL(k_operon_expand, grid256(X), dim3(256), 0, st, X, nE, e0, b.lo, off.p, lbeg.p, lop.p, d_eop.p, d_ostart.p, key.p, val.p);
            g.sort(call, key.p, val.p, X, 32 + op_bits);
            g.segments(call, X);
            const u32 nr = g.nseg;
            n_cand += nr;
            pi.ensure((size_t)nr + 2), pj.ensure((size_t)nr + 2), pn.ensure((size_t)nr + 2);
            if (all) {
                key2.ensure((size_t)nr + 2), idx2.ensure((size_t)nr + 2), cnt.ensure((size_t)nops + 2);
                HIP_CHECK(hipMemsetAsync(cnt.p, 0, (size_t)nops * sizeof(u32), st));
            } else {
                flag.ensure((size_t)nr + 2), pos.ensure((size_t)nr + 2);
            }
            hipLaunchKernelGGL(k_operon_pairs, grid256(nr), dim3(256), 0, st, nr, g.start.p, g.skey.p, g.sidx.p, b.lo, d_len.p, d_has0.p, all ? 1 : 0, rank_bits, pi.p, pj.p,
                               pn.p, flag.p, key2.p, idx2.p, cnt.p, npass.p);
            u32 nout = nr;
            if (all) {
                g2.sort(call, key2.p, idx2.p, nr, rank_bits + op_bits);
                oi.ensure((size_t)nr + 2), oj.ensure((size_t)nr + 2), on.ensure((size_t)nr + 2);
                hipLaunchKernelGGL(k_operon_gather, grid256(nr), dim3(256), 0, st, nr, g2.sidx.p, pi.p, pj.p, pn.p, oi.p, oj.p, on.p);
            } else {
                const u32* d_nout = scan_u32(flag.p, pos.p, nr, false, tmp.p, st);   // (tmp: sized for X >= nr)
                HIP_CHECK(hipGetLastError());
                nout = call.read(d_nout);
                oi.ensure((size_t)nout + 2), oj.ensure((size_t)nout + 2), on.ensure((size_t)nout + 2);
                hipLaunchKernelGGL(k_operon_compact, grid256(nr), dim3(256), 0, st, nr, flag.p, pos.p, pi.p, pj.p, pn.p, oi.p, oj.p, on.p);
            }
            HIP_CHECK(hipGetLastError());
            const size_t base = vi.size();
            vi.resize(base + nout), vj.resize(base + nout), vn.resize(base + nout);
            if (nout) call.fetch(vi.data() + base, oi.p, nout), call.fetch(vj.data() + base, oj.p, nout), call.fetch(vn.data() + base, on.p, nout);
            if (all) call.fetch(hcnt.data(), cnt.p, nops), call.fetch(&h_npass, npass.p);
            call.wait();   // the rows have left the batch's buffers
            if (all)
                for (u32 k = 0; k < nops; ++k) cstart[(size_t)b.lo + k + 1] = hcnt[k];
        }
        out->waits = call.waits;
        out->n_candidates = (i64)n_cand;
        out->n_pairs = all ? (i64)h_npass : (i64)vi.size();
        out->i = host_copy_of(w, vi), out->j = host_copy_of(w, vj), out->nshr = host_copy_of(w, vn);
        if (all) {
            for (size_t i = 0; i < N; ++i) cstart[i + 1] += cstart[i];
            out->cand_start = host_copy_of(w, cstart);
        }
        fill_empty_slots(slots(out));
    });
}

}  // extern "C"
