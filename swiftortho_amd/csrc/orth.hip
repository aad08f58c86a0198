// orth.hip -- the candidate stage of find_orth on the device: from the hit rows of a search (columns uploaded from the host, or the so_hit
// records so_search_device left in HBM) to the three candidate tables swiftortho_amd/find_orth.py `candidates()` defines -- the ortholog
// and in-paralog pairs proposed exactly twice, and the best score of every co-ortholog candidate pair.  It is the one part of that stage
// that touches every row.  so_orth_candidates_* hand those tables to the host; so_orth_relations_* go on from them on the device (the
// relations part below: normalisers, co-ortholog products, repeat rule, normalisation) and hand out the relation tables -- the text stays
// on the host.
//
// The numpy function is the definition, and the tables are reproduced bit for bit:
//   * a row is kept unless (1 + |qed - qst|) / qlen < coverage or idy < identity (a NaN coverage keeps the row); the score is the bit
//     score, bit / aln (bal), or bit / (bit score of the first kept row of the same query CODE, anywhere in the input) (bsr) -- one IEEE
//     division each;
//   * a run = consecutive kept rows of one query code; per (run, subject) the largest score; per (run, subject taxon) and per run over
//     the subjects of another taxon than the query's the largest of those, both starting from 0;
//   * a (run, subject) group is an in-paralog candidate (same taxon, score >= the run's out-of-taxon maximum, not the query itself;
//     emitted in both orientations), an ortholog candidate (other taxon, score >= its taxon's maximum) or a co-ortholog candidate (other
//     taxon otherwise), keyed min(q, s) * M + max(q, s);
//   * a key proposed exactly twice is a pair scored ((0 + s0) + s1) / 2 -- the LAST key of the sorted list, when it is one, max(s0, s1);
//     co-ortholog candidates: distinct keys with their maximum.
// Every maximum is exact whatever the order, so the order of a run's rows and of the candidates never reaches the output: scores are
// compared through an order-preserving 64-bit code of the double (orth_enc) and reduced with integer atomic maxima.  A NaN is the largest
// code, as numpy's maximum lets it win; its payload is not kept.  (Where +0 and -0 tie numpy keeps the one it met first; here +0 wins.
// Bit scores are integers, and their quotients are zero only as +0.)
//
// Kernels.  k_orth_unpack (records -> columns; hit_codes, hit_table.h), k_orth_rows (keep flags) -> scan -> k_orth_compact (kept rows,
// scores, first row per code) -> k_orth_bsr -> key_runs -> run_starts (k_util.hip: k_run_heads -> scan -> k_run_starts, the run bounds).
// Every host wait goes through the call's DeviceCall (device_call.h: read, fetch + wait).  The host reads the run bounds and sorts the
// runs into three lists by length (tune.h: ORTH_WAVE_ROWS, ORTH_LDS_ROWS, ORTH_LDS_TAXA; SOHIT_ORTH_TIER forces one tier wherever it can take the run):
//   k_orth_run_wave     a run of up to 64 rows, a row per lane of one wave: dedupe and maxima with shuffles over the run's lanes;
//   k_orth_run_table    one run per workgroup: an open-addressing table subject -> best score and a table taxon -> maximum, in LDS
//                       (<false>) or, for longer runs and more taxa, in global scratch whose extents the host planned (<true>).
// All three append their candidates to the three lists, one reservation per wave and list.  Then per list: library radix sort of
// (key, score), k_orth_twice / k_orth_distinct flag the key groups, scan, k_orth_twice_emit / k_orth_distinct_emit write the tables.
#include "common.h"
#include "hit_table.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace {

#define ORTH_EMPTY 0xFFFFFFFFu                 // free slot of a subject table
#define ORTH_ENC_ZERO 0x8000000000000000ull    // orth_enc(+0.)
#define ORTH_LDS_SLOTS (2 * ORTH_LDS_ROWS)
#define ORTH_MIN_SLOTS 256u                    // smallest table: one slot per thread of the workgroup (the passes over it stay wave-uniform)

// order-preserving code of a double: a < b  <=>  enc(a) < enc(b) for everything but NaN, which is the largest code; 0 is no value's code
__device__ __forceinline__ u64 orth_enc(double v) {
    if (v != v) return ~0ull;
    const u64 b = (u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | ORTH_ENC_ZERO);
}
__device__ __forceinline__ double orth_dec(u64 e) {
    if (e == ~0ull) return __longlong_as_double(0x7FF8000000000000ll);
    return __longlong_as_double((long long)((e >> 63) ? (e & ~ORTH_ENC_ZERO) : ~e));
}
__device__ __forceinline__ u64 umax64(u64 a, u64 b) { return a < b ? b : a; }

struct OrthLists {   // candidate (key, score bits) lists and their fill counters: cnt[0] orthologs, [1] in-paralogs, [2] co-orthologs, [3] groups
    u64 *ot_k, *ot_v, *ip_k, *ip_v, *co_k, *co_v;
    u32* cnt;
};

// `per` list slots for every lane that wants them, one atomic per wave; called by all 64 lanes of the wave
__device__ __forceinline__ u32 wave_reserve(u32* ctr, bool want, u32 per) {
    const unsigned long long m = __ballot(want);
    if (!m) return 0;
    const u32 lane = threadIdx.x & 63u;
    const int leader = __builtin_ctzll(m);
    u32 base = 0;
    if ((int)lane == leader) base = atomicAdd(ctr, per * (u32)__popcll(m));
    base = __shfl(base, leader);
    return base + per * (u32)__popcll(m & ((1ull << lane) - 1ull));
}

// one (run, subject) group: classified and appended; `have` false on lanes without a group (they only take part in the reservations)
__device__ __forceinline__ void orth_emit(bool have, int q, int s, int qtx, int stx, u64 ebest, u64 etmax, u64 eomax, u64 M, const OrthLists& L) {
    const double sco = orth_dec(ebest);
    const bool same = qtx == stx;
    const bool is_ip = have && same && sco >= orth_dec(eomax) && q != s;
    const bool is_ot = have && !same && sco >= orth_dec(etmax);
    const bool is_co = have && !same && !is_ot;
    const u64 a = (u64)min(q, s), b = (u64)max(q, s);
    const u64 v = (u64)__double_as_longlong(sco);
    u32 p = wave_reserve(L.cnt + 0, is_ot, 1);
    if (is_ot) L.ot_k[p] = a * M + b, L.ot_v[p] = v;
    p = wave_reserve(L.cnt + 1, is_ip, 2);
    if (is_ip) L.ip_k[p] = a * M + b, L.ip_v[p] = v, L.ip_k[p + 1] = b * M + a, L.ip_v[p + 1] = v;
    p = wave_reserve(L.cnt + 2, is_co, 1);
    if (is_co) L.co_k[p] = a * M + b, L.co_v[p] = v;
    const unsigned long long g = __ballot(have);
    if (g && (threadIdx.x & 63u) == 0) atomicAdd(L.cnt + 3, (u32)__popcll(g));
}

// ---- rows ----------------------------------------------------------------------------------------------------------------------------
// so_hit records -> the columns columns_from_records() builds; err |= 1 / 2: a qidx / sidx outside its map
__global__ __launch_bounds__(256) void k_orth_unpack(const so_hit* __restrict__ h, u32 n, const int* __restrict__ qmap, i64 nq, const int* __restrict__ smap, i64 ns,
                                                     int* __restrict__ q, int* __restrict__ s, double* __restrict__ idy, double* __restrict__ aln,
                                                     double* __restrict__ qst, double* __restrict__ qed, double* __restrict__ score, double* __restrict__ qlen,
                                                     u32* __restrict__ err) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const so_hit r = h[i];
    int qc, sc;
    hit_codes(r, qmap, nq, smap, ns, qc, sc, err);
    q[i] = qc, s[i] = sc;
    // numpy rounds to 6 decimals as rint(x * 1e6) / 1e6; then the two decimals the text row would carry
    const double r6 = __ddiv_rn(rint(__dmul_rn(r.identity, 1e6)), 1e6);
    idy[i] = __ddiv_rn(floor(__dadd_rn(__dmul_rn(r6, 100.), 1e-7)), 100.);
    aln[i] = (double)r.aln, qst[i] = (double)r.qst, qed[i] = (double)r.qed, score[i] = (double)r.bit, qlen[i] = (double)r.qlen;
}

// keep[i] = the row passes the filter; err |= 4: a name code outside [0, n_names)
__global__ __launch_bounds__(256) void k_orth_rows(u32 n, const int* __restrict__ q, const int* __restrict__ s, const double* __restrict__ idy,
                                                   const double* __restrict__ qst, const double* __restrict__ qed, const double* __restrict__ qlen, i64 n_names,
                                                   double coverage, double identity, u32* __restrict__ keep, u32* __restrict__ err) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (q[i] < 0 || q[i] >= n_names || s[i] < 0 || s[i] >= n_names) atomicOr(err, 4u);
    const double qcv = __ddiv_rn(__dadd_rn(1., fabs(__dadd_rn(qed[i], -qst[i]))), qlen[i]);
    keep[i] = ((qcv < coverage) | (idy[i] < identity)) ? 0u : 1u;
}

// the kept rows in order; norm 2 (bal): score = bit / aln; norm 1 (bsr): first[code] = the code's first kept row
__global__ __launch_bounds__(256) void k_orth_compact(u32 n, const u32* __restrict__ keep, const u32* __restrict__ pos, const int* __restrict__ q, const int* __restrict__ s,
                                                      const double* __restrict__ score, const double* __restrict__ aln, int norm, int* __restrict__ kq,
                                                      int* __restrict__ ks, double* __restrict__ ksco, u32* __restrict__ first) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const u32 j = pos[i];
    kq[j] = q[i], ks[j] = s[i];
    ksco[j] = norm == 2 ? __ddiv_rn(score[i], aln[i]) : score[i];
    if (norm == 1) atomicMin(first + q[i], j);
}

__global__ __launch_bounds__(256) void k_orth_bsr(u32 nk, const int* __restrict__ kq, const double* __restrict__ bit, const u32* __restrict__ first, double* __restrict__ sco) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i < nk) sco[i] = __ddiv_rn(bit[i], bit[first[kq[i]]]);
}

// ---- runs ----------------------------------------------------------------------------------------------------------------------------
// a run of up to 64 rows per wave, a row per lane
__global__ __launch_bounds__(256) void k_orth_run_wave(const u32* __restrict__ list, u32 nlist, const u32* __restrict__ rstart, const int* __restrict__ kq,
                                                       const int* __restrict__ ks, const double* __restrict__ ksco, const int* __restrict__ tax, u64 M, OrthLists L) {
    const u32 w = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (w >= nlist) return;   // (a whole wave)
    const u32 lane = threadIdx.x & 63u;
    const u32 r = list[w];
    const u32 b = rstart[r], len = rstart[r + 1] - b;   // 1 .. 64
    const bool have = lane < len;
    const int q = kq[b];
    int s = -1;
    u64 e = 0;
    if (have) s = ks[b + lane], e = orth_enc(ksco[b + lane]);
    // dedupe: the best score of this lane's subject over the run; the first lane of a subject stands for the group
    u64 best = e;
    bool rep = have;
    for (u32 j = 0; j < len; ++j) {
        const int sj = __shfl(s, (int)j);
        const u64 ej = __shfl(e, (int)j);
        if (have && sj == s) {
            best = umax64(best, ej);
            if (j < lane) rep = false;
        }
    }
    const int qtx = tax[q];
    const int stx = have ? tax[s] : -1;
    u64 tm = ORTH_ENC_ZERO, om = ORTH_ENC_ZERO;
    for (unsigned long long m = __ballot(rep); m; m &= m - 1ull) {
        const int j = __builtin_ctzll(m);
        const int tj = __shfl(stx, j);
        const u64 bj = __shfl(best, j);
        if (tj == stx) tm = umax64(tm, bj);
        if (tj != qtx) om = umax64(om, bj);
    }
    orth_emit(rep, q, s, qtx, stx, best, tm, om, M, L);
}

template <class T>
__device__ __forceinline__ T tab_load(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct OrthPlan {   // scratch tier: where run list[k] keeps its tables
    u64 slot0;      // first slot of its subject table in hk / hv
    u32 cap;        // slots (a power of two >= 2 * rows, >= ORTH_MIN_SLOTS)
    u32 pad;
};

// one run per workgroup; GLOBAL: the subject table and the taxon maxima live in global scratch (plan), else in LDS
template <bool GLOBAL>
__global__ __launch_bounds__(256) void k_orth_run_table(const u32* __restrict__ list, u32 nlist, const OrthPlan* __restrict__ plan, u32* __restrict__ ghk, u64* __restrict__ ghv,
                                                        u64* __restrict__ gtm, const u32* __restrict__ rstart, const int* __restrict__ kq, const int* __restrict__ ks,
                                                        const double* __restrict__ ksco, const int* __restrict__ tax, u32 T, u64 M, OrthLists L) {
    __shared__ u32 s_hk[GLOBAL ? 1 : ORTH_LDS_SLOTS];
    __shared__ u64 s_hv[GLOBAL ? 1 : ORTH_LDS_SLOTS];
    __shared__ u64 s_tm[GLOBAL ? 1 : ORTH_LDS_TAXA];
    __shared__ u64 s_om;
    const u32 k = blockIdx.x;
    if (k >= nlist) return;
    const u32 tid = threadIdx.x;
    const u32 r = list[k];
    const u32 b = rstart[r], len = rstart[r + 1] - b;
    u32 cap;
    u32* hk;
    u64 *hv, *tm;
    if (GLOBAL) {
        cap = plan[k].cap;
        hk = ghk + plan[k].slot0, hv = ghv + plan[k].slot0, tm = gtm + (size_t)k * T;
    } else {
        cap = ORTH_MIN_SLOTS;
        while (cap < 2u * len && cap < ORTH_LDS_SLOTS) cap <<= 1;   // (the host sends only runs of up to ORTH_LDS_ROWS rows here)
        hk = s_hk, hv = s_hv, tm = s_tm;
    }
    const u32 mask = cap - 1u;
    for (u32 i = tid; i < cap; i += 256u) hk[i] = ORTH_EMPTY, hv[i] = 0;
    for (u32 i = tid; i < T; i += 256u) tm[i] = ORTH_ENC_ZERO;
    if (tid == 0) s_om = ORTH_ENC_ZERO;
    // (plain stores, then atomics of other waves on the same words: the barrier waits for this workgroup's stores, which are written through
    // to the L2 its atomics work in -- a release / acquire at workgroup scope -- so every atomic below meets the initial value, in LDS and
    // in global scratch alike; no other workgroup touches a run's tables)
    __syncthreads();
    // dedupe: subject -> best score
    for (u32 i = tid; i < len; i += 256u) {
        const u32 s = (u32)ks[b + i];
        const u64 e = orth_enc(ksco[b + i]);
        u32 h = (s * 0x9E3779B1u) >> 7 & mask;
        for (;;) {   // (the table is at most half full: a free slot is always met)
            const u32 prev = atomicCAS(hk + h, ORTH_EMPTY, s);
            if (prev == ORTH_EMPTY || prev == s) break;
            h = (h + 1u) & mask;
        }
        atomicMax((unsigned long long*)hv + h, (unsigned long long)e);
    }
    __syncthreads();
    const int q = kq[b];
    const int qtx = tax[q];
    // (the tables were written by atomics, which work in L2 when the tables are global: they are read back the same way)
    for (u32 i = tid; i < cap; i += 256u) {
        const u32 s = tab_load(hk + i);
        if (s == ORTH_EMPTY) continue;
        const int t = tax[s];
        const u64 e = tab_load(hv + i);
        atomicMax((unsigned long long*)tm + t, (unsigned long long)e);
        if (t != qtx) atomicMax((unsigned long long*)&s_om, (unsigned long long)e);
    }
    __syncthreads();
    const u64 om = tab_load(&s_om);
    for (u32 i = tid; i < cap; i += 256u) {   // (cap is a multiple of 256: every wave makes the same number of turns, all lanes in it)
        const u32 s = tab_load(hk + i);
        const bool have = s != ORTH_EMPTY;
        const int stx = have ? tax[s] : -1;
        orth_emit(have, q, have ? (int)s : 0, qtx, stx, tab_load(hv + i), have ? tab_load(tm + stx) : 0, om, M, L);
    }
}

// ---- pairs ---------------------------------------------------------------------------------------------------------------------------
// flag[i] = 1 where a key group of exactly two members starts
__global__ __launch_bounds__(256) void k_orth_twice(const u64* __restrict__ key, u32 n, u32* __restrict__ flag) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    const bool head = i == 0 || key[i - 1] != k;
    flag[i] = (head && i + 1 < n && key[i + 1] == k && (i + 2 >= n || key[i + 2] != k)) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_orth_twice_emit(const u64* __restrict__ key, const u64* __restrict__ val, u32 n, const u32* __restrict__ flag, const u32* __restrict__ pos,
                                                         u64 M, i64* __restrict__ oa, i64* __restrict__ ob, double* __restrict__ os) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const double s0 = __longlong_as_double((long long)val[i]), s1 = __longlong_as_double((long long)val[i + 1]);
    const u32 p = pos[i];
    const u64 k = key[i];
    oa[p] = (i64)(k / M), ob[p] = (i64)(k % M);
    // the last pair of the sorted list keeps the larger proposal, every other one the mean
    os[p] = i + 2 == n ? (s1 > s0 ? s1 : s0) : __ddiv_rn(__dadd_rn(__dadd_rn(0., s0), s1), 2.);
}

__global__ __launch_bounds__(256) void k_orth_distinct(const u64* __restrict__ key, u32 n, u32* __restrict__ flag) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) flag[i] = (i == 0 || key[i - 1] != key[i]) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_orth_distinct_emit(const u64* __restrict__ key, const u64* __restrict__ val, u32 n, const u32* __restrict__ flag,
                                                            const u32* __restrict__ pos, i64* __restrict__ okey, double* __restrict__ obest) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const u64 k = key[i];
    double acc = -INFINITY;
    for (u32 j = i; j < n && key[j] == k; ++j) {   // numpy's maximum: the accumulator stays unless the newcomer is larger; a NaN stays
        const double v = __longlong_as_double((long long)val[j]);
        if (!(acc >= v || acc != acc)) acc = v;
    }
    okey[pos[i]] = (i64)k, obest[pos[i]] = acc;
}

thread_local std::string g_orth_err;

struct OrthCols {   // device columns of n rows
    const int *q, *s;
    const double *idy, *aln, *qst, *qed, *score, *qlen;
};

// sorted (key, value) list -> its flags and their exclusive scan; returns the device word holding the number of flagged groups
struct PairStage {
    DevBuf<u64> sk, sv;
    DevBuf<u32> flag, pos, tmp;
    DevBuf<u8> sort_tmp;
    const u32* total = nullptr;
    void run(bool twice, const u64* k, const u64* v, u32 n, int bits, hipStream_t st) {
        sk.ensure(n + 2), sv.ensure(n + 2), flag.ensure(n + 2), pos.ensure(n + 2), tmp.ensure(scan_u32_temp_elems(n) + 2);
        const size_t tb = sort_pairs_u64_u64_temp_bytes(n, bits);
        sort_tmp.ensure(tb + 16);
        sort_pairs_u64_u64(sort_tmp.p, tb, k, sk.p, v, sv.p, n, bits, st);
        if (n) {
            if (twice) hipLaunchKernelGGL(k_orth_twice, grid256(n), dim3(256), 0, st, sk.p, n, flag.p);
            else hipLaunchKernelGGL(k_orth_distinct, grid256(n), dim3(256), 0, st, sk.p, n, flag.p);
        }
        total = scan_u32(flag.p, pos.p, n, false, tmp.p, st);
    }
};

// the candidate tables of one call, left on the device: what so_orth_candidates_* download and so_orth_relations_* work on
struct OrthDev {
    DevBuf<int> tax;                  // taxon code of every name
    DevBuf<i64> ot_a, ot_b, ip_a, ip_b, co_key;
    DevBuf<double> ot_s, ip_s, co_best;
    u32 n_ot = 0, n_ip = 0, n_co = 0;
    i64 n_rows = 0, n_runs = 0, n_groups = 0;
    u64 M = 1;
    u32 T = 1;
};

void orth_run(DeviceCall& call, i64 n, const OrthCols& c, i64 n_names, const int32_t* tax, i64 n_taxa, double coverage, double identity, int norm, u32* d_err,
              const char* who, OrthDev* out) {
    hipStream_t st = call.st;
    const Tune& tn = call.tn;
    const u64 M = (u64)(n_names > 0 ? n_names : 1);
    const u32 T = (u32)(n_taxa > 0 ? n_taxa : 1);
    const u32 N = (u32)n;
    out->M = M, out->T = T;
    DevBuf<int>& d_tax = out->tax;
    DevBuf<int> kq, ks;
    DevBuf<u32> keep, pos, tmp_a, tmp_b, first, head, rid, rstart;
    DevBuf<double> kbit, ksco;
    upload(d_tax, tax, (size_t)n_names, st);
    keep.ensure(N + 2), pos.ensure(N + 2), tmp_a.ensure(scan_u32_temp_elems(N) + 2);
    hipLaunchKernelGGL(k_orth_rows, grid256(N), dim3(256), 0, st, N, c.q, c.s, c.idy, c.qst, c.qed, c.qlen, n_names, coverage, identity, keep.p, d_err);
    const u32* d_nk = scan_u32(keep.p, pos.p, N, false, tmp_a.p, st);
    u32 nk = 0, err = 0;
    call.read(d_nk, nk, d_err, err);
    hit_table_errors(who, err);
    out->n_rows = nk;
    if (!nk) return;   // every row filtered: all tables empty

    // kept rows, scores, runs
    kq.ensure(nk + 2), ks.ensure(nk + 2), kbit.ensure(nk + 2);
    if (norm == 1) {
        first.ensure((size_t)M + 2), ksco.ensure(nk + 2);
        HIP_CHECK(hipMemsetAsync(first.p, 0xFF, (size_t)M * sizeof(u32), st));
    }
    hipLaunchKernelGGL(k_orth_compact, grid256(N), dim3(256), 0, st, N, keep.p, pos.p, c.q, c.s, c.score, c.aln, norm, kq.p, ks.p, kbit.p, first.p);
    const double* sco = kbit.p;
    if (norm == 1) {
        hipLaunchKernelGGL(k_orth_bsr, grid256(nk), dim3(256), 0, st, nk, kq.p, kbit.p, first.p, ksco.p);
        sco = ksco.p;
    }
    head.ensure(nk + 2), rid.ensure(nk + 2), rstart.ensure(nk + 3), tmp_b.ensure(scan_u32_temp_elems(nk) + 2);
    const u32* d_nruns = key_runs(kq.p, nk, head.p, rid.p, tmp_b.p, st);
    run_starts(head.p, rid.p, nk, d_nruns, rstart.p, st);
    const u32 nruns = call.read(d_nruns);
    std::vector<u32> rs((size_t)nruns + 1);
    call.fetch(rs.data(), rstart.p, rs.size());
    call.wait();
    out->n_runs = nruns;

    // the runs by tier; the scratch tier's tables laid out one behind the other
    std::vector<u32> l_wave, l_lds, l_scr;
    std::vector<OrthPlan> plan;
    u64 slots = 0;
    const bool lds_taxa = T <= ORTH_LDS_TAXA;
    for (u32 r = 0; r < nruns; ++r) {
        const u32 len = rs[r + 1] - rs[r];
        int tier = len <= ORTH_WAVE_ROWS ? ORTH_TIER_WAVE : (len <= ORTH_LDS_ROWS && lds_taxa) ? ORTH_TIER_LDS : ORTH_TIER_SCRATCH;
        if (tn.orth_tier == ORTH_TIER_SCRATCH) tier = ORTH_TIER_SCRATCH;
        if (tn.orth_tier == ORTH_TIER_LDS && len <= ORTH_LDS_ROWS && lds_taxa) tier = ORTH_TIER_LDS;
        // (forcing the wave tier changes nothing: it already takes every run it can hold)
        if (tier == ORTH_TIER_WAVE) l_wave.push_back(r);
        else if (tier == ORTH_TIER_LDS) l_lds.push_back(r);
        else {
            u32 cap = ORTH_MIN_SLOTS;
            while (cap < 2ull * len) cap <<= 1;   // len < 2^31 - but 2 * len may need 2^32 slots: refused below
            if (cap < 2ull * len) throw SoError(std::string(who) + ": a run of 2^30 rows and more is not supported");
            l_scr.push_back(r);
            plan.push_back(OrthPlan{slots, cap, 0});
            slots += cap;
        }
    }
    DevBuf<u32> d_lw, d_ll, d_ls, ghk, cnt;
    DevBuf<u64> ghv, gtm;
    DevBuf<OrthPlan> d_plan;
    upload(d_lw, l_wave.data(), l_wave.size(), st), upload(d_ll, l_lds.data(), l_lds.size(), st), upload(d_ls, l_scr.data(), l_scr.size(), st);
    upload(d_plan, plan.data(), plan.size(), st);
    if (!l_scr.empty()) ghk.ensure(slots + 2), ghv.ensure(slots + 2), gtm.ensure(l_scr.size() * (size_t)T + 2);

    // candidate lists: at most one ortholog or co-ortholog candidate, or two in-paralog entries, per kept row
    OrthLists L;
    DevBuf<u64> ot_k, ot_v, ip_k, ip_v, co_k, co_v;
    ot_k.ensure(nk + 2), ot_v.ensure(nk + 2), co_k.ensure(nk + 2), co_v.ensure(nk + 2), ip_k.ensure(2 * (size_t)nk + 2), ip_v.ensure(2 * (size_t)nk + 2);
    cnt.ensure(8);
    HIP_CHECK(hipMemsetAsync(cnt.p, 0, 8 * sizeof(u32), st));
    L.ot_k = ot_k.p, L.ot_v = ot_v.p, L.ip_k = ip_k.p, L.ip_v = ip_v.p, L.co_k = co_k.p, L.co_v = co_v.p, L.cnt = cnt.p;
    if (!l_wave.empty())
        hipLaunchKernelGGL(k_orth_run_wave, dim3((u32)((l_wave.size() + 3) / 4)), dim3(256), 0, st, d_lw.p, (u32)l_wave.size(), rstart.p, kq.p, ks.p, sco, d_tax.p, M, L);
    if (!l_lds.empty())
        hipLaunchKernelGGL(k_orth_run_table<false>, dim3((u32)l_lds.size()), dim3(256), 0, st, d_ll.p, (u32)l_lds.size(), (const OrthPlan*)nullptr, (u32*)nullptr, (u64*)nullptr,
                           (u64*)nullptr, rstart.p, kq.p, ks.p, sco, d_tax.p, T, M, L);
    if (!l_scr.empty())
        hipLaunchKernelGGL(k_orth_run_table<true>, dim3((u32)l_scr.size()), dim3(256), 0, st, d_ls.p, (u32)l_scr.size(), d_plan.p, ghk.p, ghv.p, gtm.p, rstart.p, kq.p, ks.p,
                           sco, d_tax.p, T, M, L);
    u32 hc[4] = {0, 0, 0, 0};
    call.fetch(hc, cnt.p, 4);
    HIP_CHECK(hipGetLastError());
    call.wait();
    out->n_groups = hc[3];
    if (hc[1] >= (1u << 31)) throw SoError(std::string(who) + ": 2^31 in-paralog candidates and more are not supported");
    if (hc[0] > nk || hc[2] > nk || hc[1] > 2ull * nk) throw SoError(std::string(who) + ": internal error: a candidate list overflowed");

    // pairs proposed exactly twice; distinct co-ortholog keys
    const int bits = ceil_log2(M * M);
    PairStage p_ot, p_ip, p_co;
    p_ot.run(true, ot_k.p, ot_v.p, hc[0], bits, st);
    p_ip.run(true, ip_k.p, ip_v.p, hc[1], bits, st);
    p_co.run(false, co_k.p, co_v.p, hc[2], bits, st);
    u32 tot[3] = {0, 0, 0};
    call.fetch(tot + 0, p_ot.total), call.fetch(tot + 1, p_ip.total), call.fetch(tot + 2, p_co.total);
    call.wait();
    DevBuf<i64>&o_ota = out->ot_a, &o_otb = out->ot_b, &o_ipa = out->ip_a, &o_ipb = out->ip_b, &o_cok = out->co_key;
    DevBuf<double>&o_ots = out->ot_s, &o_ips = out->ip_s, &o_cob = out->co_best;
    o_ota.ensure(tot[0] + 2), o_otb.ensure(tot[0] + 2), o_ots.ensure(tot[0] + 2), o_ipa.ensure(tot[1] + 2), o_ipb.ensure(tot[1] + 2), o_ips.ensure(tot[1] + 2);
    o_cok.ensure(tot[2] + 2), o_cob.ensure(tot[2] + 2);
    if (hc[0]) hipLaunchKernelGGL(k_orth_twice_emit, grid256(hc[0]), dim3(256), 0, st, p_ot.sk.p, p_ot.sv.p, hc[0], p_ot.flag.p, p_ot.pos.p, M, o_ota.p, o_otb.p, o_ots.p);
    if (hc[1]) hipLaunchKernelGGL(k_orth_twice_emit, grid256(hc[1]), dim3(256), 0, st, p_ip.sk.p, p_ip.sv.p, hc[1], p_ip.flag.p, p_ip.pos.p, M, o_ipa.p, o_ipb.p, o_ips.p);
    if (hc[2]) hipLaunchKernelGGL(k_orth_distinct_emit, grid256(hc[2]), dim3(256), 0, st, p_co.sk.p, p_co.sv.p, hc[2], p_co.flag.p, p_co.pos.p, o_cok.p, o_cob.p);
    HIP_CHECK(hipGetLastError());
    out->n_ot = tot[0], out->n_ip = tot[1], out->n_co = tot[2];
}

// so_orth_candidates_*: the tables come to the host
void orth_finish(OrthDev& D, DeviceCall& call, const char* who, so_orth_cand* out) {
    hipStream_t st = call.st;
    out->n_rows = D.n_rows, out->n_runs = D.n_runs, out->n_groups = D.n_groups;
    out->n_ot = D.n_ot, out->n_ip = D.n_ip, out->n_co = D.n_co;
    out->ot_a = host_copy(who, D.ot_a.p, D.n_ot, st), out->ot_b = host_copy(who, D.ot_b.p, D.n_ot, st), out->ot_s = host_copy(who, D.ot_s.p, D.n_ot, st);
    out->ip_a = host_copy(who, D.ip_a.p, D.n_ip, st), out->ip_b = host_copy(who, D.ip_b.p, D.n_ip, st), out->ip_s = host_copy(who, D.ip_s.p, D.n_ip, st);
    out->co_key = host_copy(who, D.co_key.p, D.n_co, st), out->co_best = host_copy(who, D.co_best.p, D.n_co, st);
    call.wait();
}

// ---- relations -----------------------------------------------------------------------------------------------------------------------
// so_orth_relations_*: find_orth.py `relation_tables()` on the tables above, which never leave the device -- the in-paralog normalisers,
// the co-ortholog products, the repeat rule and the per-(block, subject taxon) normalisation; bit for bit.
// What that rests on: numpy's bincount(weights=) adds a group's rows in array order, so every float64 sum here is ONE chain
// ((0 + x0) + x1) + ... over the group's rows in table order: the rows are grouped by a STABLE radix sort of (group key, row), and one wave
// per group loads 64 rows at a time, coalesced, and adds them one after the other (k_rel_ip_avg, k_rel_group_norm: the same kernel shape
// for a group of one row and of a million -- no size tiers).  No float atomics, no tree or wave reductions, nothing to contract (the sums
// and quotients are single __dadd_rn / __ddiv_rn).  Positions come from count -> scan -> emit throughout; the one atomic (the 64-bit total
// of the co-ortholog products) decides no position.
//   k_rel_has_ot -> k_rel_fwd_flag / scan / k_rel_fwd_emit (forward in-paralog pairs, keyed by the taxon of a) -> sort -> segments ->
//   k_rel_ip_avg -> k_rel_ip_flag / scan / k_rel_ip_emit;  k_rel_co_count / scan / k_rel_co_probe / scan / k_rel_co_emit;
//   per section (OT, CO): k_rel_blk_heads / scan / run_starts, [sort by pair, k_rel_occ], scan, k_rel_keep_emit, sort by group,
//   segments, k_rel_group_norm.  (sort, segments: SortedGroups, device_call.h -- stable radix sort, then key_runs / run_starts.)
__device__ __forceinline__ u32 lower_i64(const i64* __restrict__ a, u32 n, i64 x) {   // first position with a[p] >= x
    u32 lo = 0, hi = n;
    while (lo < hi) {
        const u32 m = lo + ((hi - lo) >> 1);
        if (a[m] < x) lo = m + 1u;
        else hi = m;
    }
    return lo;
}
__device__ __forceinline__ u32 upper_i64(const i64* __restrict__ a, u32 n, i64 x) {   // first position with a[p] > x
    u32 lo = 0, hi = n;
    while (lo < hi) {
        const u32 m = lo + ((hi - lo) >> 1);
        if (a[m] <= x) lo = m + 1u;
        else hi = m;
    }
    return lo;
}
static_assert(ORTH_WAVE_ROWS == 64, "the group kernels walk a group one wave-wide chunk of rows at a time");
// the value lane j holds (j the same in all lanes)
__device__ __forceinline__ double lane_get(double v, int j) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(256) void k_rel_has_ot(const i64* __restrict__ ot_a, const i64* __restrict__ ot_b, u32 n, u32* __restrict__ has) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) has[ot_a[i]] = 1u, has[ot_b[i]] = 1u;
}

__global__ __launch_bounds__(256) void k_rel_fwd_flag(const i64* __restrict__ ip_a, const i64* __restrict__ ip_b, u32 n, u32* __restrict__ flag) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) flag[i] = ip_a[i] < ip_b[i] ? 1u : 0u;
}

// the forward pairs in table order: fidx = row of the in-paralog table, fkey = taxon of its a
__global__ __launch_bounds__(256) void k_rel_fwd_emit(const i64* __restrict__ ip_a, u32 n, const u32* __restrict__ flag, const u32* __restrict__ pos,
                                                      const int* __restrict__ tax, u32* __restrict__ fidx, u64* __restrict__ fkey) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const u32 p = pos[i];
    fidx[p] = i, fkey[p] = (u64)tax[ip_a[i]];
}

// one wave per taxon that has forward pairs: the sum over all its pairs and over those with an ortholog on either side, each one chain in
// table order (sidx ascends inside a segment: the sort is stable) -> avg[taxon]
__global__ __launch_bounds__(256) void k_rel_ip_avg(const u32* __restrict__ start, u32 nseg, const u64* __restrict__ skey, const u32* __restrict__ sidx,
                                                    const i64* __restrict__ ip_a, const i64* __restrict__ ip_b, const double* __restrict__ ip_s,
                                                    const u32* __restrict__ has, double* __restrict__ avg) {
    const u32 w = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (w >= nseg) return;   // (a whole wave)
    const u32 lane = threadIdx.x & 63u;
    const u32 lo = (u32)__builtin_amdgcn_readfirstlane((int)start[w]), hi = (u32)__builtin_amdgcn_readfirstlane((int)start[w + 1]);
    double all = 0., near = 0.;
    u32 ncnt = 0;
    for (u32 base = lo; base < hi; base += ORTH_WAVE_ROWS) {
        const u32 i = base + lane;
        double v = 0.;
        bool nr = false;
        if (i < hi) {
            const u32 r = sidx[i];
            v = ip_s[r];
            nr = (has[ip_a[r]] | has[ip_b[r]]) != 0u;
        }
        const unsigned long long m = __ballot(nr);
        const int cnt = (int)min((u32)ORTH_WAVE_ROWS, hi - base);
        ncnt += (u32)__popcll(m);
        for (int j = 0; j < cnt; ++j) {
            const double x = lane_get(v, j);
            all = __dadd_rn(all, x);
            if ((m >> j) & 1ull) near = __dadd_rn(near, x);
        }
    }
    if (lane == 0) avg[skey[lo]] = ncnt > 0 ? __ddiv_rn(near, (double)ncnt) : __ddiv_rn(all, (double)(hi - lo));
}

// a forward pair is a row unless its taxon's normaliser is zero (a NaN normaliser keeps it, as numpy's != does)
__global__ __launch_bounds__(256) void k_rel_ip_flag(const u32* __restrict__ fidx, u32 nf, const i64* __restrict__ ip_a, const int* __restrict__ tax,
                                                     const double* __restrict__ avg, u32* __restrict__ flag) {
    const u32 p = blockIdx.x * 256u + threadIdx.x;
    if (p < nf) flag[p] = avg[tax[ip_a[fidx[p]]]] != 0. ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_rel_ip_emit(const u32* __restrict__ fidx, u32 nf, const u32* __restrict__ flag, const u32* __restrict__ pos,
                                                     const i64* __restrict__ ip_a, const i64* __restrict__ ip_b, const double* __restrict__ ip_s,
                                                     const int* __restrict__ tax, const double* __restrict__ avg, i64* __restrict__ oa, i64* __restrict__ ob,
                                                     double* __restrict__ ov) {
    const u32 p = blockIdx.x * 256u + threadIdx.x;
    if (p >= nf || !flag[p]) return;
    const u32 r = fidx[p], o = pos[p];
    oa[o] = ip_a[r], ob[o] = ip_b[r], ov[o] = __ddiv_rn(ip_s[r], avg[tax[ip_a[r]]]);
}

// per ortholog pair: where the in-paralogs of its two genes lie in the table, and how many products it expands to; the products' 64-bit
// total (an integer: any order); err |= 8: one pair alone has 2^32 products or more
__global__ __launch_bounds__(256) void k_rel_co_count(const i64* __restrict__ ot_a, const i64* __restrict__ ot_b, u32 n, const i64* __restrict__ ip_a, u32 n_ip,
                                                      u32* __restrict__ lo_q, u32* __restrict__ nq, u32* __restrict__ lo_s, u32* __restrict__ ns,
                                                      u32* __restrict__ cnt, unsigned long long* __restrict__ total, u32* __restrict__ err) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    unsigned long long c = 0;
    if (i < n) {
        const i64 a = ot_a[i], b = ot_b[i];
        const u32 lq = lower_i64(ip_a, n_ip, a), cq = upper_i64(ip_a, n_ip, a) - lq;
        const u32 ls = lower_i64(ip_a, n_ip, b), cs = upper_i64(ip_a, n_ip, b) - ls;
        lo_q[i] = lq, nq[i] = cq, lo_s[i] = ls, ns[i] = cs;
        if (cq > 0 || cs > 0) c = ((unsigned long long)cq + 1ull) * ((unsigned long long)cs + 1ull);
        if (c > 0xFFFFFFFFull) atomicOr(err, 8u);
        cnt[i] = (u32)c;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(total, c);
}

// one thread per product, in (pair, qi-major, si-minor) order: partners in table order, the gene itself last; hit = the product is a
// co-ortholog candidate in this orientation (cpos: where)
__global__ __launch_bounds__(256) void k_rel_co_probe(u32 P, const u32* __restrict__ base, u32 n_ot, const u32* __restrict__ lo_q, const u32* __restrict__ nq,
                                                      const u32* __restrict__ lo_s, const u32* __restrict__ ns, const i64* __restrict__ ot_a,
                                                      const i64* __restrict__ ot_b, const i64* __restrict__ ip_b, const i64* __restrict__ co_key, u32 n_co, u64 M,
                                                      u32* __restrict__ hit, u32* __restrict__ cpos) {
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t >= P) return;
    u32 lo = 0, hi = n_ot;   // the last pair whose first product is <= t (pairs without products share their successor's base)
    while (lo < hi) {
        const u32 m = lo + ((hi - lo) >> 1);
        if (base[m] <= t) lo = m + 1u;
        else hi = m;
    }
    const u32 u = lo - 1u;
    const u32 local = t - base[u];
    const u32 cs = ns[u] + 1u;
    const u32 qi = local / cs, si = local % cs;
    const i64 qip = qi < nq[u] ? ip_b[lo_q[u] + qi] : ot_a[u];
    const i64 sip = si < ns[u] ? ip_b[lo_s[u] + si] : ot_b[u];
    const i64 k = (i64)((u64)qip * M + (u64)sip);
    const u32 p = lower_i64(co_key, n_co, k);
    const bool h = p < n_co && co_key[p] == k;
    hit[t] = h ? 1u : 0u, cpos[t] = p;
}
__global__ __launch_bounds__(256) void k_rel_co_emit(u32 P, const u32* __restrict__ hit, const u32* __restrict__ pos, const u32* __restrict__ cpos,
                                                     const i64* __restrict__ co_key, const double* __restrict__ co_best, u64 M, i64* __restrict__ oa,
                                                     i64* __restrict__ ob, double* __restrict__ os) {
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t >= P || !hit[t]) return;
    const u32 c = cpos[t], o = pos[t];
    const u64 k = (u64)co_key[c];
    oa[o] = (i64)(k / M), ob[o] = (i64)(k % M), os[o] = co_best[c];
}

// blocks of a section: runs of consecutive rows whose a has one taxon
__global__ __launch_bounds__(256) void k_rel_blk_heads(const i64* __restrict__ pa, const int* __restrict__ tax, u32 n, u32* __restrict__ head) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) head[i] = (i == 0 || tax[pa[i]] != tax[pa[i - 1]]) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_rel_pair_keys(const i64* __restrict__ pa, const i64* __restrict__ pb, u32 n, u64 M, u64* __restrict__ key, u32* __restrict__ idx) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) key[i] = (u64)pa[i] * M + (u64)pb[i], idx[i] = i;
}
// rows sorted by pair (stable: rows of one pair ascend, and so do their blocks): a row stays when it is the first of its (pair, block), or the
// second and the pair is its block's first pair.  bid: block number + 1; bstart: first row of every block
__global__ __launch_bounds__(256) void k_rel_occ(const u64* __restrict__ skey, const u32* __restrict__ sidx, u32 n, const u32* __restrict__ bid,
                                                 const u32* __restrict__ bstart, const i64* __restrict__ pa, const i64* __restrict__ pb, u64 M, u32* __restrict__ keep) {
    const u32 j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const u32 r = sidx[j];
    const u32 b = bid[r];
    const u64 k = skey[j];
    const bool same1 = j >= 1u && skey[j - 1] == k && bid[sidx[j - 1]] == b;
    const bool same2 = same1 && j >= 2u && skey[j - 2] == k && bid[sidx[j - 2]] == b;
    const u32 f = bstart[b - 1u];
    const bool first_pair = k == (u64)pa[f] * M + (u64)pb[f];
    keep[r] = (!same1 || (!same2 && first_pair)) ? 1u : 0u;
}
// the kept rows in order, with their group key block * T + taxon of b
__global__ __launch_bounds__(256) void k_rel_keep_emit(u32 n, const u32* __restrict__ keep, const u32* __restrict__ pos, const i64* __restrict__ pa,
                                                       const i64* __restrict__ pb, const double* __restrict__ ps, const u32* __restrict__ bid,
                                                       const int* __restrict__ tax, u32 T, i64* __restrict__ oa, i64* __restrict__ ob, double* __restrict__ os,
                                                       u64* __restrict__ gkey, u32* __restrict__ gidx) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const u32 p = pos[i];
    oa[p] = pa[i], ob[p] = pb[i], os[p] = ps[i];
    gkey[p] = (u64)(bid[i] - 1u) * T + (u64)tax[pb[i]], gidx[p] = p;
}
// one wave per (block, subject taxon) group: the sum of its rows' scores as one chain in kept order, then v = s / (sum / count)
__global__ __launch_bounds__(256) void k_rel_group_norm(const u32* __restrict__ start, u32 nseg, const u32* __restrict__ sidx, const double* __restrict__ s,
                                                        double* __restrict__ v) {
    const u32 w = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (w >= nseg) return;   // (a whole wave)
    const u32 lane = threadIdx.x & 63u;
    const u32 lo = (u32)__builtin_amdgcn_readfirstlane((int)start[w]), hi = (u32)__builtin_amdgcn_readfirstlane((int)start[w + 1]);
    double sum = 0.;
    for (u32 base = lo; base < hi; base += ORTH_WAVE_ROWS) {
        const u32 i = base + lane;
        const double x = i < hi ? s[sidx[i]] : 0.;
        const int cnt = (int)min((u32)ORTH_WAVE_ROWS, hi - base);
        for (int j = 0; j < cnt; ++j) sum = __dadd_rn(sum, lane_get(x, j));
    }
    const double mean = __ddiv_rn(sum, (double)(hi - lo));
    for (u32 i = lo + lane; i < hi; i += ORTH_WAVE_ROWS) {
        const u32 r = sidx[i];
        v[r] = __ddiv_rn(s[r], mean);
    }
}

struct RelSection {   // one output section on the device
    DevBuf<i64> a, b;
    DevBuf<double> v;
    u32 n = 0;
};

// the repeat rule and the normalisation of one section (n > 0 rows pa, pb, ps); distinct: no pair occurs twice (the ortholog table: one row
// per key that was proposed twice), so every row stays
void rel_section(DeviceCall& call, const i64* pa, const i64* pb, const double* ps, u32 n, bool distinct, const OrthDev& D, RelSection* out) {
    hipStream_t st = call.st;
    DevBuf<u32> head, bid, bstart, keep, pos, idx, gidx, tmp;
    DevBuf<u64> key, gkey;
    DevBuf<double> ks;
    head.ensure(n + 2), bid.ensure(n + 2), keep.ensure(n + 2), pos.ensure(n + 2), tmp.ensure(scan_u32_temp_elems(n) + 2);
    hipLaunchKernelGGL(k_rel_blk_heads, grid256(n), dim3(256), 0, st, pa, D.tax.p, n, head.p);
    const u32* d_nblk = scan_u32(head.p, bid.p, n, true, tmp.p, st);
    HIP_CHECK(hipGetLastError());
    const u32 nblk = call.read(d_nblk);
    if (distinct) fill_u32(keep.p, n, 1u, st);
    else {
        bstart.ensure((size_t)nblk + 3), key.ensure(n + 2), idx.ensure(n + 2);
        run_starts(head.p, bid.p, n, d_nblk, bstart.p, st);   // (d_nblk lies in tmp, which is scanned with again only below)
        hipLaunchKernelGGL(k_rel_pair_keys, grid256(n), dim3(256), 0, st, pa, pb, n, D.M, key.p, idx.p);
        SortedGroups g;
        g.sort(call, key.p, idx.p, n, ceil_log2(D.M * D.M));
        hipLaunchKernelGGL(k_rel_occ, grid256(n), dim3(256), 0, st, g.skey.p, g.sidx.p, n, bid.p, bstart.p, pa, pb, D.M, keep.p);
        HIP_CHECK(hipGetLastError());
        call.wait();   // (g's buffers go away here)
    }
    const u32* d_nk = scan_u32(keep.p, pos.p, n, false, tmp.p, st);
    HIP_CHECK(hipGetLastError());
    const u32 nk = call.read(d_nk);
    out->n = nk;
    out->a.ensure(nk + 2), out->b.ensure(nk + 2), out->v.ensure(nk + 2), ks.ensure(nk + 2), gkey.ensure(nk + 2), gidx.ensure(nk + 2);
    hipLaunchKernelGGL(k_rel_keep_emit, grid256(n), dim3(256), 0, st, n, keep.p, pos.p, pa, pb, ps, bid.p, D.tax.p, D.T, out->a.p, out->b.p, ks.p, gkey.p, gidx.p);
    SortedGroups g;
    g.sort(call, gkey.p, gidx.p, nk, ceil_log2((u64)nblk * D.T));
    g.segments(call, nk);
    hipLaunchKernelGGL(k_rel_group_norm, dim3((g.nseg + 3u) / 4u), dim3(256), 0, st, g.start.p, g.nseg, g.sidx.p, ks.p, out->v.p);
    HIP_CHECK(hipGetLastError());
    call.wait();
}

// so_orth_relations_*: the relation tables are computed where the candidate tables are; only they come to the host
void orth_finish(OrthDev& D, DeviceCall& call, const char* who, so_orth_rel* out) {
    hipStream_t st = call.st;
    out->n_rows = D.n_rows, out->n_runs = D.n_runs, out->n_groups = D.n_groups;
    RelSection ip, ot, co;
    DevBuf<u32> tmp;   // scan scratch, grown before every scan; each total is read before the next scan
    auto scan_total = [&](const u32* in, u32* pos, u32 n) {
        tmp.ensure(scan_u32_temp_elems(n) + 2);
        const u32* d = scan_u32(in, pos, n, false, tmp.p, st);
        HIP_CHECK(hipGetLastError());
        return call.read(d);
    };
    DevBuf<i64> c_a, c_b;   // the co-ortholog rows before the repeat rule
    DevBuf<double> c_s;
    u32 n_c = 0;
    if (D.n_ip) {
        // ---- in-paralog normalisers and values
        const u32 n = D.n_ip;
        DevBuf<u32> has, flag, pos, fidx, flag2, pos2;
        DevBuf<u64> fkey;
        DevBuf<double> avg;
        has.ensure((size_t)D.M + 2), flag.ensure(n + 2), pos.ensure(n + 2);
        HIP_CHECK(hipMemsetAsync(has.p, 0, (size_t)D.M * sizeof(u32), st));
        if (D.n_ot) hipLaunchKernelGGL(k_rel_has_ot, grid256(D.n_ot), dim3(256), 0, st, D.ot_a.p, D.ot_b.p, D.n_ot, has.p);
        hipLaunchKernelGGL(k_rel_fwd_flag, grid256(n), dim3(256), 0, st, D.ip_a.p, D.ip_b.p, n, flag.p);
        const u32 nf = scan_total(flag.p, pos.p, n);
        if (nf) {
            fidx.ensure(nf + 2), fkey.ensure(nf + 2), flag2.ensure(nf + 2), pos2.ensure(nf + 2), avg.ensure((size_t)D.T + 2);
            hipLaunchKernelGGL(k_rel_fwd_emit, grid256(n), dim3(256), 0, st, D.ip_a.p, n, flag.p, pos.p, D.tax.p, fidx.p, fkey.p);
            SortedGroups g;
            g.sort(call, fkey.p, fidx.p, nf, ceil_log2(D.T));
            g.segments(call, nf);
            hipLaunchKernelGGL(k_rel_ip_avg, dim3((g.nseg + 3u) / 4u), dim3(256), 0, st, g.start.p, g.nseg, g.skey.p, g.sidx.p, D.ip_a.p, D.ip_b.p, D.ip_s.p, has.p, avg.p);
            hipLaunchKernelGGL(k_rel_ip_flag, grid256(nf), dim3(256), 0, st, fidx.p, nf, D.ip_a.p, D.tax.p, avg.p, flag2.p);
            ip.n = scan_total(flag2.p, pos2.p, nf);
            ip.a.ensure(ip.n + 2), ip.b.ensure(ip.n + 2), ip.v.ensure(ip.n + 2);
            hipLaunchKernelGGL(k_rel_ip_emit, grid256(nf), dim3(256), 0, st, fidx.p, nf, flag2.p, pos2.p, D.ip_a.p, D.ip_b.p, D.ip_s.p, D.tax.p, avg.p, ip.a.p, ip.b.p, ip.v.p);
            HIP_CHECK(hipGetLastError());
            call.wait();
        }
    }
    if (D.n_ip && D.n_co && D.n_ot) {
        // ---- co-orthologs: count -> scan -> probe -> scan -> emit
        const u32 n = D.n_ot;
        DevBuf<u32> lo_q, nq, lo_s, ns, cnt, base, err, hit, hpos, cpos;
        DevBuf<unsigned long long> total;
        lo_q.ensure(n + 2), nq.ensure(n + 2), lo_s.ensure(n + 2), ns.ensure(n + 2), cnt.ensure(n + 2), base.ensure(n + 2), err.ensure(4), total.ensure(2);
        HIP_CHECK(hipMemsetAsync(err.p, 0, sizeof(u32), st));
        HIP_CHECK(hipMemsetAsync(total.p, 0, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(k_rel_co_count, grid256(n), dim3(256), 0, st, D.ot_a.p, D.ot_b.p, n, D.ip_a.p, D.n_ip, lo_q.p, nq.p, lo_s.p, ns.p, cnt.p, total.p, err.p);
        unsigned long long tot = 0;
        u32 e = 0;
        call.fetch(&tot, total.p), call.fetch(&e, err.p);
        HIP_CHECK(hipGetLastError());
        call.wait();
        if (e || tot >= (1ull << 31)) throw SoError(std::string(who) + ": 2^31 co-ortholog products and more are not supported (32-bit product numbers)");
        if (tot) {
            const u32 P = (u32)tot;
            if (scan_total(cnt.p, base.p, n) != P) throw SoError(std::string(who) + ": internal error: the co-ortholog products do not add up");
            hit.ensure((size_t)P + 2), hpos.ensure((size_t)P + 2), cpos.ensure((size_t)P + 2);
            hipLaunchKernelGGL(k_rel_co_probe, grid256(P), dim3(256), 0, st, P, base.p, n, lo_q.p, nq.p, lo_s.p, ns.p, D.ot_a.p, D.ot_b.p, D.ip_b.p, D.co_key.p, D.n_co, D.M,
                               hit.p, cpos.p);
            n_c = scan_total(hit.p, hpos.p, P);
            c_a.ensure(n_c + 2), c_b.ensure(n_c + 2), c_s.ensure(n_c + 2);
            hipLaunchKernelGGL(k_rel_co_emit, grid256(P), dim3(256), 0, st, P, hit.p, hpos.p, cpos.p, D.co_key.p, D.co_best.p, D.M, c_a.p, c_b.p, c_s.p);
            HIP_CHECK(hipGetLastError());
            call.wait();
        }
    }
    // ---- the repeat rule and the normalisation
    if (D.n_ot) rel_section(call, D.ot_a.p, D.ot_b.p, D.ot_s.p, D.n_ot, true, D, &ot);
    if (n_c) rel_section(call, c_a.p, c_b.p, c_s.p, n_c, false, D, &co);
    out->n_ip = ip.n, out->n_ot = ot.n, out->n_co = co.n;
    out->ip_a = host_copy(who, ip.a.p, ip.n, st), out->ip_b = host_copy(who, ip.b.p, ip.n, st), out->ip_v = host_copy(who, ip.v.p, ip.n, st);
    out->ot_a = host_copy(who, ot.a.p, ot.n, st), out->ot_b = host_copy(who, ot.b.p, ot.n, st), out->ot_v = host_copy(who, ot.v.p, ot.n, st);
    out->co_a = host_copy(who, co.a.p, co.n, st), out->co_b = host_copy(who, co.b.p, co.n, st), out->co_v = host_copy(who, co.v.p, co.n, st);
    call.wait();
}

// what every entry point checks before anything touches the device
template <class Out>
void orth_check(const char* who, int device, i64 n, i64 n_names, const int32_t* tax, i64 n_taxa, int norm, Out* out) {
    if (!out) throw SoError(std::string(who) + ": result pointer is NULL");
    memset(out, 0, sizeof *out);
    if (norm < 0 || norm > 2) throw SoError(std::string(who) + ": bad arguments");
    hit_table_check(who, n, n_names, tax, n_taxa, [&] {
        if (n_names > 3037000499ll) throw SoError(std::string(who) + ": n_names * n_names reaches 2^63 (pair keys a * n_names + b are 63-bit)");
    });
    check_device(who, device);
}

auto slots(so_orth_cand* r) { return result_slots(&r->ot_a, &r->ot_b, &r->ot_s, &r->ip_a, &r->ip_b, &r->ip_s, &r->co_key, &r->co_best); }
auto slots(so_orth_rel* r) { return result_slots(&r->ip_a, &r->ip_b, &r->ip_v, &r->ot_a, &r->ot_b, &r->ot_v, &r->co_a, &r->co_b, &r->co_v); }
template <class Out>
void orth_release(Out* r) {
    release_slots(r, slots(r));
}

struct OrthColBufs {   // the device columns of a call, and the maps they were unpacked through
    DevBuf<int> q, s, qmap, smap;
    DevBuf<double> idy, aln, qst, qed, score, qlen;
    DevBuf<u32> err;
};

// What the two entry families (host columns / device records) end with: columns(call, b) brings the n rows to the device -- records must
// be complete before this call's own stream reads them, so everything queued on the device so far is waited for (so_search_device has
// synchronised its stream when it returns; a torch tensor's producer is on torch's stream) -- then the candidate tables, then
// orth_finish for the kind of result asked for
template <class Out, class Columns>
void orth_tail(const char* who, int device, bool records, i64 n, i64 n_names, const int32_t* tax, i64 n_taxa, double coverage, double identity, int norm, Out* out,
               Columns columns) {
    if (n > 0) {
        DeviceCall call(device, records);
        OrthDev D;
        {
            OrthColBufs b;
            b.err.ensure(4);
            HIP_CHECK(hipMemsetAsync(b.err.p, 0, sizeof(u32), call.st));
            columns(call, b);
            const OrthCols c{b.q.p, b.s.p, b.idy.p, b.aln.p, b.qst.p, b.qed.p, b.score.p, b.qlen.p};
            orth_run(call, n, c, n_names, tax, n_taxa, coverage, identity, norm, b.err.p, who, &D);
            call.wait();   // (the columns go away here)
        }
        orth_finish(D, call, who, out);
    }
    fill_empty_slots(slots(out));
}

template <class Out>
int orth_from_cols(const char* who, int device, int64_t n, const int32_t* q, const int32_t* s, const double* idy, const double* aln, const double* qst, const double* qed,
                   const double* score, const double* qlen, int64_t n_names, const int32_t* tax, int64_t n_taxa, double coverage, double identity, int norm, Out* out) {
    return guarded_call(g_orth_err, out, orth_release<Out>, [&] {
        orth_check(who, device, n, n_names, tax, n_taxa, norm, out);
        if (n > 0 && (!q || !s || !idy || !aln || !qst || !qed || !score || !qlen)) throw SoError(std::string(who) + ": a column is NULL");
        orth_tail(who, device, false, n, n_names, tax, n_taxa, coverage, identity, norm, out, [&](DeviceCall& call, OrthColBufs& b) {
            const size_t N = (size_t)n;
            const hipStream_t st = call.st;
            upload(b.q, q, N, st), upload(b.s, s, N, st), upload(b.idy, idy, N, st), upload(b.aln, aln, N, st), upload(b.qst, qst, N, st), upload(b.qed, qed, N, st);
            upload(b.score, score, N, st), upload(b.qlen, qlen, N, st);
        });
    });
}

template <class Out>
int orth_from_records(const char* who, int device, const so_hit* d_hits, int64_t n, const int32_t* qmap, int64_t n_q, const int32_t* smap, int64_t n_s, int64_t n_names,
                      const int32_t* tax, int64_t n_taxa, double coverage, double identity, int norm, Out* out) {
    return guarded_call(g_orth_err, out, orth_release<Out>, [&] {
        orth_check(who, device, n, n_names, tax, n_taxa, norm, out);
        if (n_q < 0 || n_s < 0 || (n_q > 0 && !qmap) || (n_s > 0 && !smap)) throw SoError(std::string(who) + ": bad arguments");
        if (n > 0 && !d_hits) throw SoError(std::string(who) + ": the record pointer is NULL");
        orth_tail(who, device, true, n, n_names, tax, n_taxa, coverage, identity, norm, out, [&](DeviceCall& call, OrthColBufs& b) {
            const size_t N = (size_t)n;
            upload(b.qmap, qmap, (size_t)n_q, call.st), upload(b.smap, smap, (size_t)n_s, call.st);
            b.q.ensure(N + 2), b.s.ensure(N + 2), b.idy.ensure(N + 2), b.aln.ensure(N + 2), b.qst.ensure(N + 2), b.qed.ensure(N + 2), b.score.ensure(N + 2), b.qlen.ensure(N + 2);
            hipLaunchKernelGGL(k_orth_unpack, grid256(N), dim3(256), 0, call.st, d_hits, (u32)N, b.qmap.p, (i64)n_q, b.smap.p, (i64)n_s, b.q.p, b.s.p, b.idy.p, b.aln.p, b.qst.p,
                               b.qed.p, b.score.p, b.qlen.p, b.err.p);
        });
    });
}

}  // namespace

extern "C" {

const char* so_orth_last_error(void) { return g_orth_err.c_str(); }

void so_orth_free(so_orth_cand* r) {
    if (r) orth_release(r);
}

void so_orth_rel_free(so_orth_rel* r) {
    if (r) orth_release(r);
}

int so_orth_candidates_cols(int device, int64_t n, const int32_t* q, const int32_t* s, const double* idy, const double* aln, const double* qst, const double* qed,
                            const double* score, const double* qlen, int64_t n_names, const int32_t* tax, int64_t n_taxa, double coverage, double identity, int norm,
                            so_orth_cand* out) {
    return orth_from_cols("so_orth_candidates_cols", device, n, q, s, idy, aln, qst, qed, score, qlen, n_names, tax, n_taxa, coverage, identity, norm, out);
}

int so_orth_candidates_records(int device, const so_hit* d_hits, int64_t n, const int32_t* qmap, int64_t n_q, const int32_t* smap, int64_t n_s, int64_t n_names,
                               const int32_t* tax, int64_t n_taxa, double coverage, double identity, int norm, so_orth_cand* out) {
    return orth_from_records("so_orth_candidates_records", device, d_hits, n, qmap, n_q, smap, n_s, n_names, tax, n_taxa, coverage, identity, norm, out);
}

int so_orth_relations_cols(int device, int64_t n, const int32_t* q, const int32_t* s, const double* idy, const double* aln, const double* qst, const double* qed,
                           const double* score, const double* qlen, int64_t n_names, const int32_t* tax, int64_t n_taxa, double coverage, double identity, int norm,
                           so_orth_rel* out) {
    return orth_from_cols("so_orth_relations_cols", device, n, q, s, idy, aln, qst, qed, score, qlen, n_names, tax, n_taxa, coverage, identity, norm, out);
}

int so_orth_relations_records(int device, const so_hit* d_hits, int64_t n, const int32_t* qmap, int64_t n_q, const int32_t* smap, int64_t n_s, int64_t n_names,
                              const int32_t* tax, int64_t n_taxa, double coverage, double identity, int norm, so_orth_rel* out) {
    return orth_from_records("so_orth_relations_records", device, d_hits, n, qmap, n_q, smap, n_s, n_names, tax, n_taxa, coverage, identity, norm, out);
}

}  // extern "C"
