// pan_bits.h -- what the stages over the family-by-taxon presence matrix (pan.hip, phyletic.hip) share: the check of a (row, taxon) member
// pair and the row-major presence words made from the pairs.
#pragma once
#include "tree_stage.h"

#ifdef __HIPCC__
namespace {

// err |= 1: a row outside 0 .. n_rows - 1; err |= 2: a taxon outside 0 .. T - 1 (nothing is written for such a pair)
__device__ __forceinline__ bool pan_pair(u32 i, const int* __restrict__ row, const int* __restrict__ tax, u32 n_rows, u32 T, u32& r, u32& t, u32* __restrict__ err) {
    r = (u32)row[i], t = (u32)tax[i];
    if (r >= n_rows) {
        atomicOr(err, 1u);
        return false;
    }
    if (t >= T) {
        atomicOr(err, 2u);
        return false;
    }
    return true;
}

// the row-major twin of k_pan_bits: bit t & 63 of rowbits[r * TW + (t >> 6)] is the presence of taxon t in row r (TW = ceil(T / 64))
__global__ __launch_bounds__(256) void k_pan_rowbits(u32 m, const int* __restrict__ row, const int* __restrict__ tax, u32 n_rows, u32 T, u32 TW, ull* __restrict__ rowbits,
                                                     u32* __restrict__ err) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    u32 r, t;
    if (i < m && pan_pair(i, row, tax, n_rows, T, r, t, err)) atomicOr(rowbits + (size_t)r * TW + (t >> 6), 1ull << (t & 63u));
}

}  // namespace
#endif
