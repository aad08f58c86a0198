// k_uqchain.hip -- the hits k_ungapq leaves over, ordered per QUERY on chip (a wave's registers; a workgroup's LDS for the few long lists) and
// handed to the chain kernel (stage A of the sparse passes' chain flow; stage B is k_ungap2's QSEG instance, k_ungap1.hip).
//
// k_ungapq extends the hits that are alone on their diagonal and writes the others -- a few hundred per query and chunk -- as k_lookup's
// 8-byte keys into keys[qseg[q] .. seg_end[q]).  Those used to take the device-wide segmented library sort and k_ungap's walk over all H
// slots of the array.  Here a query's keys are sorted where they fit:
//
//   * k_uqsort_wave: a WAVE per query (work counter) for up to UQS_WAVE_CAP keys, in REGISTERS: lane l holds the keys l * NR .. l * NR + NR - 1
//     (NR = 1 .. 16 by the query's count, the rest padded with all-ones), a bitonic network whose steps at distances below NR are
//     compare-exchanges between the lane's own registers and the others one lane exchange per register -- no LDS array, no barrier.  Then,
//     per hit, a 32-bit word  query position | head flag  goes to the hit's own place of `words`, and per group head its diagonal id into
//     `garr` and (position, query) into the chain list (k_ungap1's mlist: pieces of U1_LCHUNK entries per wave, unused = UG_REC_NONE).
//     A longer query goes onto a list of its own;
//   * k_uqsort_wg: a WORKGROUP per listed query: a bitonic sort in 32 KB of LDS for up to UQS_WG_CAP keys (all compare-exchanges ascending,
//     so the slots beyond the last key never have to exist), and the same in place in the key array (global memory, one workgroup) for the
//     few queries above that -- no host decision, no host wait.
// The keys of one query are distinct and share their query bits, so the order by the whole key is the order by (subject or band,
// diagonal, query position) and stability does not matter.
#include "ungap1.h"

#define UQS_WAVES 4                      // waves per workgroup of the wave tier (each on a query of its own)
#define UQS_NRMAX 16                     // keys per lane of the wave tier's largest instance
#define UQS_WAVE_CAP (64 * UQS_NRMAX)    // keys a wave sorts in its registers (config 3: 28 % of the queries leave <= 64 hits over, half of them 257 .. 512,
                                         // 4.5 % 513 .. 1024, none more)
#define UQS_WG_CAP 4096                  // keys a workgroup sorts in LDS (32 KB)
#define UQS_HEAD 0x40000000u             // words: bit 30 = first hit of its group

// Bitonic sort of a[0 .. n) ascending, P2 = power of two >= n.  Every compare-exchange orders (i, j), i < j, ascending: with the first
// step of each merge taken against the mirrored partner the slots [n, P2) behave as +infinity without being touched.
template <typename I, typename A, typename SYNC>
__device__ __forceinline__ void uqs_bitonic(A a, I n, int lgP /*P2 = 1 << lgP >= n*/, u32 tid, u32 nthr, SYNC sync) {
    const I half = ((I)1 << lgP) >> 1;
    for (int lk = 1; lk <= lgP; ++lk) {   // merges of 2^lk slots
        const I k = (I)1 << lk, hk = k >> 1;
        for (I t = tid; t < half; t += nthr) {   // mirror step
            const I blk = t >> (lk - 1), off = t & (hk - 1);
            const I i = (blk << lk) + off, j = (blk << lk) + (k - 1 - off);
            if (j < n) {
                const u64 x = a[i], y = a[j];
                if (x > y) a[i] = y, a[j] = x;
            }
        }
        sync();
        for (int lh = lk - 2; lh >= 0; --lh) {   // distances 2^lh
            const I h = (I)1 << lh;
            for (I t = tid; t < half; t += nthr) {
                const I blk = t >> lh, off = t & (h - 1);
                const I i = (blk << (lh + 1)) + off, j = i + h;
                if (j < n) {
                    const u64 x = a[i], y = a[j];
                    if (x > y) a[i] = y, a[j] = x;
                }
            }
            sync();
        }
    }
}

// the wave's piece of the chain list
struct UqsList {
    u32 pos, end;
};

// `total` (<= U1_LCHUNK, wave-uniform) entries of the chain list for the wave: what is left of its piece first, then the head of a fresh one
// (u1_reserve's scheme: no entry of a piece stays unused but the last piece's tail).  The entry of rank k is uqs_slot(k, ...).
struct UqsSlots {
    u32 pos, avail, nbase;
};
__device__ __forceinline__ UqsSlots uqs_reserve(u32 total, int lane, UqsList& lc, u32* __restrict__ mlist_cnt) {
    UqsSlots sl = {lc.pos, lc.end - lc.pos, 0};
    if (total > sl.avail) {
        u32 nbase = 0;
        if (lane == 0) nbase = atomicAdd(mlist_cnt, (u32)U1_LCHUNK);
        sl.nbase = (u32)__builtin_amdgcn_readfirstlane((int)nbase);
        lc.pos = sl.nbase + (total - sl.avail), lc.end = sl.nbase + U1_LCHUNK;
    } else lc.pos += total;
    return sl;
}
__device__ __forceinline__ u32 uqs_slot(u32 k, const UqsSlots& sl) { return k < sl.avail ? sl.pos + k : sl.nbase + (k - sl.avail); }

// Key `key` of the sorted keys' place i (n keys in all; `prev`: the key in front of it) of the query whose segment starts at h0, a lane each: its
// word, and for a group head the diagonal id and the chain-list entry.
__device__ __forceinline__ void uqs_emit_key(u64 key, u64 prev, u32 i, u32 n, u32 h0, u32 qrel, int lane, int sh_diag, int sh_qpos, u32 pmask, u32 gmaskv,
                                             u32* __restrict__ words, u32* __restrict__ garr, u64* __restrict__ mlist, u32* __restrict__ mlist_cnt, UqsList& lc) {
    const bool valid = i < n;
    const bool head = valid && (i == 0 || (key >> sh_diag) != (prev >> sh_diag));
    if (valid) words[h0 + i] = ((u32)(key >> sh_qpos) & pmask) | (head ? UQS_HEAD : 0u);
    const unsigned long long hb = __ballot(head);
    if (!hb) return;
    const UqsSlots sl = uqs_reserve((u32)__popcll(hb), lane, lc, mlist_cnt);
    if (head) {
        garr[h0 + i] = (u32)(key >> sh_diag) & gmaskv;
        mlist[uqs_slot((u32)__popcll(hb & ((1ull << lane) - 1ull)), sl)] = (u64)(h0 + i) | ((u64)qrel << 32);
    }
}
// ... of the sorted keys a[i0 .. i0 + 64) in LDS or global memory
template <typename A>
__device__ __forceinline__ void uqs_emit(A a, u32 n, u32 i0, u32 h0, u32 qrel, int lane, int sh_diag, int sh_qpos, u32 pmask, u32 gmaskv, u32* __restrict__ words,
                                         u32* __restrict__ garr, u64* __restrict__ mlist, u32* __restrict__ mlist_cnt, UqsList& lc) {
    const u32 i = i0 + (u32)lane;
    u64 key = 0, prev = 0;
    if (i < n) {
        key = a[i];
        if (i) prev = a[i - 1];
    }
    uqs_emit_key(key, prev, i, n, h0, qrel, lane, sh_diag, sh_qpos, pmask, gmaskv, words, garr, mlist, mlist_cnt, lc);
}

// ---- the wave tier: 64 * NR keys in registers, lane l holding places l * NR + r ----
__device__ __forceinline__ void uqs_cx(u64& a, u64& b, bool asc) {   // a: the lower place
    const bool sw = (a > b) == asc;
    const u64 x = sw ? b : a, y = sw ? a : b;
    a = x, b = y;
}
__device__ __forceinline__ u64 uqs_shfl_xor(u64 v, u32 m) {
    const u32 lo = (u32)__shfl_xor((int)(u32)v, (int)m), hi = (u32)__shfl_xor((int)(u32)(v >> 32), (int)m);
    return ((u64)hi << 32) | lo;
}
template <int NR>
__device__ __forceinline__ void uqs_local(u64 (&v)[NR], bool asc) {   // the steps at distances NR / 2 .. 1 of a merge whose direction is the lane's
#pragma unroll
    for (int j = NR >> 1; j >= 1; j >>= 1) {
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if ((r & j) == 0) uqs_cx(v[r], v[r | j], asc);
    }
}
template <int NR>
__device__ void uqs_wave_query(const u64* __restrict__ keys, u32 n, u32 h0, u32 qrel, int lane, int sh_diag, int sh_qpos, u32 pmask, u32 gmaskv, u32* __restrict__ words,
                               u32* __restrict__ garr, u64* __restrict__ mlist, u32* __restrict__ mlist_cnt, UqsList& lc) {
    u64 v[NR];
    const u32 l0 = (u32)lane * NR;   // the lane's first place
#pragma unroll
    for (int r = 0; r < NR; r += 2) {   // 16 bytes per load where the lane holds two keys and more (no key is all-ones: that is the dropped key of the library-sort flow)
        if (NR >= 2 && l0 + r + 1 < n) {
            const uint4 t = u1_load16(reinterpret_cast<const u8*>(keys + h0 + l0 + r));
            v[r] = ((u64)t.y << 32) | t.x, v[r + (NR >= 2 ? 1 : 0)] = ((u64)t.w << 32) | t.z;
        } else {
            v[r] = l0 + r < n ? keys[h0 + l0 + r] : ~0ull;
            if (NR >= 2) v[r + (NR >= 2 ? 1 : 0)] = ~0ull;
        }
    }
    // merges of 2 .. NR places: inside the lane (direction by the place's own bits; of the last one by the lane's lowest)
#pragma unroll
    for (int k = 2; k <= NR; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j >= 1; j >>= 1) {
#pragma unroll
            for (int r = 0; r < NR; ++r)
                if ((r & j) == 0) uqs_cx(v[r], v[r | j], k < NR ? (r & k) == 0 : (lane & 1) == 0);
        }
    }
    // merges of 2 NR .. 64 NR places: distances of whole lanes by exchange, the rest inside the lane
    for (u32 kk = 2; kk <= 64; kk <<= 1) {
        const bool asc = ((u32)lane & kk) == 0;
        for (u32 jj = kk >> 1; jj >= 1; jj >>= 1) {
            const bool keepmin = (((u32)lane & jj) == 0) == asc;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const u64 o = uqs_shfl_xor(v[r], jj);
                v[r] = ((o < v[r]) == keepmin) ? o : v[r];
            }
        }
        uqs_local<NR>(v, asc);
    }
    // ---- words, diagonal ids, chain-list entries: the heads in the order of their places (rank = heads of the lanes before + of the lane's earlier places) ----
    // the key in front of the lane's first one: the last key of the lane before it
    u64 prev = ((u64)(u32)__shfl_up((int)(u32)(v[NR - 1] >> 32), 1) << 32) | (u32)__shfl_up((int)(u32)v[NR - 1], 1);
    u32 wd[NR], hm = 0;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const u32 i = l0 + r;
        const bool head = i < n && (i == 0 || (v[r] >> sh_diag) != (prev >> sh_diag));
        wd[r] = ((u32)(v[r] >> sh_qpos) & pmask) | (head ? UQS_HEAD : 0u);
        hm |= (head ? 1u : 0u) << r;
        prev = v[r];
    }
    if (NR >= 4) {
#pragma unroll
        for (int r = 0; r < NR; r += 4) {
            if (l0 + r + 3 < n) __builtin_memcpy(words + h0 + l0 + r, &wd[r], 16);
            else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (l0 + r + k < n) words[h0 + l0 + r + k] = wd[r + (NR >= 4 ? k : 0)];
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (l0 + r < n) words[h0 + l0 + r] = wd[r];
    }
    const u32 cnt = (u32)__popc(hm);
    u32 incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u32 t = (u32)__shfl_up((int)incl, o);
        if (lane >= o) incl += t;
    }
    const u32 total = (u32)__builtin_amdgcn_readlane((int)incl, 63);   // (>= 1: place 0 is a head; <= n <= U1_LCHUNK)
    const UqsSlots sl = uqs_reserve(total, lane, lc, mlist_cnt);
    u32 rank = incl - cnt;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if ((hm >> r) & 1u) {
            garr[h0 + l0 + r] = (u32)(v[r] >> sh_diag) & gmaskv;
            mlist[uqs_slot(rank++, sl)] = (u64)(h0 + l0 + r) | ((u64)qrel << 32);
        }
    }
}
static_assert(UQS_WAVE_CAP <= U1_LCHUNK, "a query's heads are reserved at once");

// ustat: [0] += queries with leftover hits, [2] += queries above the LDS tiers, [3] = max leftover hits of a query
// (A wave takes `batch` consecutive queries per visit to the work counter: one same-address atomic per query -- 100 k of them, served one
// after the other at about 10 ns -- took longer than all the sorting.)
__global__ __launch_bounds__(64 * UQS_WAVES) void k_uqsort_wave(const u32* __restrict__ qseg, const u32* __restrict__ seg_end, u32 nqp, u32 batch, const u64* __restrict__ keys, u32 cap,
                                                               int sh_diag, int sh_qpos, u32 pmask, u32 gmaskv, u32* __restrict__ words, u32* __restrict__ garr,
                                                               u64* __restrict__ mlist, u32* __restrict__ mlist_cnt, u32* __restrict__ work_ctr, u32* __restrict__ big,
                                                               u32* __restrict__ big_cnt, unsigned long long* __restrict__ ustat) {
    const int lane = threadIdx.x & 63;
    UqsList lc = {0, 0};
    u32 nq = 0, nmax = 0;
    u32 q_next = 0, q_end = 0;   // the wave's batch of queries
    for (;;) {
        if (q_next == q_end) {
            u32 b0 = 0;
            if (lane == 0) b0 = atomicAdd(work_ctr, batch);
            q_next = (u32)__builtin_amdgcn_readfirstlane((int)b0);
            if (q_next >= nqp) break;
            q_end = min(q_next + batch, nqp);
        }
        const u32 qrel = q_next++;
        const u32 h0 = (u32)__builtin_amdgcn_readfirstlane((int)qseg[qrel]);
        const u32 n = (u32)__builtin_amdgcn_readfirstlane((int)seg_end[qrel]) - h0;
        if (!n) continue;
        ++nq, nmax = max(nmax, n);
        if (n > cap) {   // the workgroup tier's
            if (lane == 0) big[atomicAdd(big_cnt, 1u)] = qrel;
            continue;
        }
#define UQS_GO(NR) uqs_wave_query<NR>(keys, n, h0, qrel, lane, sh_diag, sh_qpos, pmask, gmaskv, words, garr, mlist, mlist_cnt, lc)
        if (n <= 64) UQS_GO(1);
        else if (n <= 128) UQS_GO(2);
        else if (n <= 256) UQS_GO(4);
        else if (n <= 512) UQS_GO(8);
        else UQS_GO(16);
#undef UQS_GO
        static_assert(UQS_NRMAX == 16, "instances up to 16 keys per lane");
    }
    for (u32 k = lc.pos + (u32)lane; k < lc.end; k += 64) mlist[k] = UG_REC_NONE;
    if (lane == 0 && nq) atomicAdd(&ustat[0], (unsigned long long)nq), atomicMax(&ustat[3], (unsigned long long)nmax);
}

__global__ __launch_bounds__(256) void k_uqsort_wg(const u32* __restrict__ qseg, const u32* __restrict__ seg_end, u64* __restrict__ keys, u32 cap /*<= UQS_WG_CAP*/,
                                                   int sh_diag, int sh_qpos, u32 pmask, u32 gmaskv, u32* __restrict__ words, u32* __restrict__ garr, u64* __restrict__ mlist,
                                                   u32* __restrict__ mlist_cnt, u32* __restrict__ work_ctr, const u32* __restrict__ big, const u32* __restrict__ big_cnt,
                                                   unsigned long long* __restrict__ ustat) {
    __shared__ u64 s_keys[UQS_WG_CAP];
    __shared__ u32 s_next;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const u32 nbig = *big_cnt;
    UqsList lc = {0, 0};
    u32 nover = 0;
    for (;;) {
        __syncthreads();   // (s_next and s_keys are free again)
        if (threadIdx.x == 0) s_next = atomicAdd(work_ctr, 1u);
        __syncthreads();
        const u32 it = s_next;
        if (it >= nbig) break;
        const u32 qrel = big[it];
        const u32 h0 = qseg[qrel], n = seg_end[qrel] - h0;
        if (n <= cap) {
            for (u32 i = threadIdx.x; i < n; i += 256) s_keys[i] = keys[h0 + i];
            __syncthreads();
            int lgP = 0;
            while ((1u << lgP) < n) ++lgP;
            uqs_bitonic<u32>(s_keys, n, lgP, threadIdx.x, 256u, [] { __syncthreads(); });
            for (u32 i0 = 64u * (u32)w; i0 < n; i0 += 256) uqs_emit(s_keys, n, i0, h0, qrel, lane, sh_diag, sh_qpos, pmask, gmaskv, words, garr, mlist, mlist_cnt, lc);
        } else {   // above the LDS tiers: in place in the key array
            u64* g = keys + h0;
            int lgP = 0;
            while ((1ull << lgP) < (u64)n) ++lgP;
            uqs_bitonic<u64>(g, (u64)n, lgP, threadIdx.x, 256u, [] { __threadfence_block(); __syncthreads(); });
            for (u32 i0 = 64u * (u32)w; i0 < n; i0 += 256) uqs_emit(g, n, i0, h0, qrel, lane, sh_diag, sh_qpos, pmask, gmaskv, words, garr, mlist, mlist_cnt, lc);
            ++nover;
        }
    }
    for (u32 k = lc.pos + (u32)lane; k < lc.end; k += 64) mlist[k] = UG_REC_NONE;
    if (threadIdx.x == 0 && nover) atomicAdd(&ustat[2], (unsigned long long)nover);
}

u32 uqchain_tier(int tier) { return tier == 0 ? UQS_WAVE_CAP : UQS_WG_CAP; }
static u32 uqs_wave_grid(u32 ncu, u32 nqp) { return (u32)std::min<u64>((u64)ncu * 8u, ((u64)nqp + UQS_WAVES - 1) / UQS_WAVES); }
static u32 uqs_wg_grid(u32 ncu, u32 nqp) { return (u32)std::min<u64>((u64)ncu * 2u, nqp); }
// Entries of the chain list of a pass of H hits and nqp queries.  Every leftover hit may head a group (<= H entries used), a piece is filled to
// its last entry before the next one is taken, and every wave of the two kernels that meets a head ends inside a piece of its own: at most
// H / U1_LCHUNK + waves pieces are ever reserved.
size_t uqchain_mlist_cap(u32 H, u32 ncu, u32 nqp) {
    const size_t waves = (size_t)uqs_wave_grid(ncu, nqp) * UQS_WAVES + (size_t)uqs_wg_grid(ncu, nqp) * 4;
    return ((size_t)H / U1_LCHUNK + waves + 2) * U1_LCHUNK;
}

// words: H + 8 words (the chain kernel reads four ahead), garr: H words.  ctr: four zeroed words (work counters of the two tiers, length of the
// long-query list, -); big: nqp words.  cap_max: SOHIT_UQ_CHAINS (< 0: the compiled limits).  mlist_cap: entries `mlist` holds; nothing is
// launched and false comes back when that is less than uqchain_mlist_cap(H, ncu, nqp).
bool launch_uqsort(u32 ncu, const u32* qseg, const u32* seg_end, u32 nqp, u32 H, u64* keys, const KeyLayout& kl, long long cap_max, u32* words, u32* garr, u64* mlist,
                   size_t mlist_cap, u32* mlist_cnt, u32* ctr, u32* big, unsigned long long* ustat, hipStream_t st) {
    if (!nqp) return true;
    if (mlist_cap < uqchain_mlist_cap(H, ncu, nqp)) return false;
    const u32 cap_wg = cap_max > 0 ? (u32)std::min<long long>(cap_max, UQS_WG_CAP) : (u32)UQS_WG_CAP;
    const u32 cap_wave = std::min<u32>(cap_wg, UQS_WAVE_CAP);
    const u32 pmask = (1u << kl.bp) - 1u;
    const int gbits = kl.bs + kl.bd;
    const u32 gmaskv = gbits >= 32 ? 0xFFFFFFFFu : ((1u << gbits) - 1u);
    const u32 gw = uqs_wave_grid(ncu, nqp);
    const u32 batch = std::max<u32>(1u, std::min<u32>(16u, nqp / (gw * UQS_WAVES)));
    hipLaunchKernelGGL(k_uqsort_wave, dim3(gw), dim3(64 * UQS_WAVES), 0, st, qseg, seg_end, nqp, batch, keys, cap_wave, kl.sh_diag, kl.sh_qpos, pmask, gmaskv,
                       words, garr, mlist, mlist_cnt, ctr, big, ctr + 2, ustat);
    hipLaunchKernelGGL(k_uqsort_wg, dim3(uqs_wg_grid(ncu, nqp)), dim3(256), 0, st, qseg, seg_end, keys, cap_wg, kl.sh_diag, kl.sh_qpos, pmask, gmaskv, words, garr, mlist,
                       mlist_cnt, ctr + 1, big, ctr + 2, ustat);
    return true;
}
