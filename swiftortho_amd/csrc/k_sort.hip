// k_sort.hip -- device radix sorts used for diagonal binning and candidate ordering.
// The sort itself is the rocPRIM library primitive (a plain library sort, like a plain
// library GEMM); everything around it (key construction, grouping, extension) is
// hand-written in the other k_*.hip files.
#include "common.h"
#include "kernels.h"
#include <hipcub/hipcub.hpp>

#include <algorithm>

// the library takes the count as an int: what does not fit is refused, by the sorts and by their *_temp_bytes
static int sort_count(const char* who, size_t n) {
    if (n > 0x7FFFFFFFull) throw SoError(std::string(who) + ": 2^31 keys and more are not served");
    return static_cast<int>(n);
}

// the thresholds of rocprim::radix_sort (device_radix_sort.hpp) under the default configuration, from the library's own types
template <class V>
static int tier_of(size_t n, size_t* single_block, size_t* merge_limit) {
    using base = typename rocprim::detail::radix_sort_block_sort_config_base<u64, V>::type;
    constexpr size_t single = (size_t)rocprim::min(256u, base::block_size) * rocprim::min(4u, base::items_per_thread);
    constexpr size_t limit = rocprim::radix_sort_config<>::merge_sort_limit;
    if (single_block) *single_block = single;
    if (merge_limit) *merge_limit = limit;
    return n <= single ? 0 : n <= limit ? 1 : 2;
}
int sort_u64_tier(size_t n, int value_bytes, size_t* single_block, size_t* merge_limit) {
    if (value_bytes == 0) return tier_of<rocprim::empty_type>(n, single_block, merge_limit);
    if (value_bytes == 4) return tier_of<u32>(n, single_block, merge_limit);
    if (value_bytes == 8) return tier_of<u64>(n, single_block, merge_limit);
    throw SoError("sort_u64_tier: values of 0, 4 or 8 bytes");
}

// NOTE a field that begins above bit 0 and ends at bit 64: rocPRIM's merge-sort comparator builds its mask as (1 << (begin + bits)) - 1, a
// shift by the word size, and ends up comparing the bits BELOW begin_bit (ROCm 7.2; the same slip as in the segmented sorts' short
// segments, k_sortseg.hip) -- between one block's keys and merge_sort_limit the output was not even a permutation of the input (found
// by tests/test_gpu_prim.py; seed_pass sorts [sh_diag, total) and total may be 64).  Such a sort leaves the merge tier out: one block,
// or onesweep, both of which extract digits.
bool sort_keys_skips_merge(int begin_bit, int end_bit) { return begin_bit > 0 && end_bit >= 64; }
using NoMergeConfig = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 0>;

size_t sort_keys_u64_temp_bytes(size_t n, int bits) {
    const int N = sort_count("sort_keys_u64_temp_bytes", n);
    size_t bytes = 0, bytes2 = 0;
    (void)hipcub::DeviceRadixSort::SortKeys((void*)nullptr, bytes, (const u64*)nullptr, (u64*)nullptr, N, 0, bits, (hipStream_t)0);
    if (bits >= 64)   // the begin bit is not known here: room for either way
        (void)rocprim::radix_sort_keys<NoMergeConfig>(nullptr, bytes2, (const u64*)nullptr, (u64*)nullptr, N, 0u, 64u, (hipStream_t)0, false);
    return std::max(bytes, bytes2);
}

// stable LSD radix sort on key bits [begin_bit, end_bit)
void sort_keys_u64(void* temp, size_t temp_bytes, const u64* in, u64* out, size_t n, int begin_bit, int end_bit, hipStream_t st) {
    const int N = sort_count("sort_keys_u64", n);
    if (n == 0) return;
    if (sort_keys_skips_merge(begin_bit, end_bit)) {
        HIP_CHECK(rocprim::radix_sort_keys<NoMergeConfig>(temp, temp_bytes, in, out, N, (unsigned)begin_bit, (unsigned)end_bit, st, false));
        return;
    }
    HIP_CHECK(hipcub::DeviceRadixSort::SortKeys(temp, temp_bytes, in, out, N, begin_bit, end_bit, st));
}

size_t sort_pairs_u64_u32_temp_bytes(size_t n, int bits) {
    const int N = sort_count("sort_pairs_u64_u32_temp_bytes", n);
    size_t bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs((void*)nullptr, bytes, (const u64*)nullptr, (u64*)nullptr, (const u32*)nullptr, (u32*)nullptr,
                                       N, 0, bits, (hipStream_t)0);
    return bytes;
}

void sort_pairs_u64_u32(void* temp, size_t temp_bytes, const u64* kin, u64* kout, const u32* vin, u32* vout, size_t n, int bits,
                        hipStream_t st) {
    const int N = sort_count("sort_pairs_u64_u32", n);
    if (n == 0) return;
    HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, kin, kout, vin, vout, N, 0, bits, st));
}

size_t sort_pairs_u64_u64_temp_bytes(size_t n, int bits) {
    const int N = sort_count("sort_pairs_u64_u64_temp_bytes", n);
    size_t bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs((void*)nullptr, bytes, (const u64*)nullptr, (u64*)nullptr, (const u64*)nullptr, (u64*)nullptr,
                                       N, 0, bits, (hipStream_t)0);
    return bytes;
}

void sort_pairs_u64_u64(void* temp, size_t temp_bytes, const u64* kin, u64* kout, const u64* vin, u64* vout, size_t n, int bits,
                        hipStream_t st) {
    const int N = sort_count("sort_pairs_u64_u64", n);
    if (n == 0) return;
    HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, kin, kout, vin, vout, N, 0, bits, st));
}

__global__ __launch_bounds__(256) void k_stride_gather(const u32* __restrict__ src, u32 stride, u32 n, u32* __restrict__ dst) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) dst[i] = src[(size_t)i * stride];
}
void launch_stride_gather(const u32* src, u32 stride, u32 n, u32* dst, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_stride_gather, dim3((n + 255) / 256), dim3(256), 0, st, src, stride, n, dst);
}
