// scan64.h -- the 64-bit scan of one workgroup, shared by the kernels that scan 64-bit values with a running carry: k_util.hip (the seed
// slots' two scans in one, k_scan_blocksums64) and fusion.hip (the pairs of every run, k_fu_scan64).
#pragma once
#include "common.h"

#ifdef __HIPCC__
__device__ __forceinline__ u64 wave_incl_scan_u64(u64 v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up((unsigned long long)v, o);
        if (lane >= o) v += t;
    }
    return v;
}
// exclusive scan over the THREADS lanes of the workgroup (lds: THREADS / 64 words); *total = their sum.  Every lane calls it.
template <int THREADS = 256>
__device__ __forceinline__ u64 block_excl_scan_u64(u64 v, u64* lds, u64* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const u64 inc = wave_incl_scan_u64(v, lane);
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    u64 base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < THREADS / 64; ++k) {
        const u64 s = lds[k];
        if (k < w) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}
#endif
