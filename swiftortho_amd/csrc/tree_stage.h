// tree_stage.h -- what the stages that make trees from replicates or families (phy.hip, pan.hip) share: the one draw of a replicate, the
// grid of a kernel that walks a length in ranges, the event timer of the stages and how many items half of the free device memory holds.
#pragma once
#include "device_call.h"

#include <utility>
#include <vector>

typedef unsigned long long ull;

// A length cut into ranges of whole chunks until about target_wgs workgroups exist, `tiles` of them per range -> (elements per range,
// ranges).  forced > 0: that many ranges (as far as there are elements), chunks or not; `most`: never more ranges than that.
inline std::pair<u32, u32> range_grid(u32 len, u32 chunk, u64 tiles, u32 target_wgs, long long forced = 0, u32 most = ~0u) {
    u32 per;
    if (forced > 0) {
        const u32 want = (u32)std::min<u64>({(u64)forced, (u64)len, (u64)most});
        per = (len + want - 1u) / want;
    } else {
        const u32 chunks = (len + chunk - 1u) / chunk;
        const u32 want = std::min({chunks, most, std::max(1u, (u32)((target_wgs + tiles - 1u) / tiles))});
        per = ((chunks + want - 1u) / want) * chunk;
    }
    return {per, (len + per - 1u) / per};
}

// Marks around the stages of a call (a timed call only: else nothing is created or recorded and every time is 0): recorded on the
// stream, read after a wait for it.  A call that waits per batch records the same marks again for every batch and sums ms(k) after
// each wait; one that waits once numbers its marks on through the batches and reads them all behind that wait.
struct StageEvents {
    std::vector<hipEvent_t> e;
    const bool on;
    explicit StageEvents(bool on) : on(on) {}
    ~StageEvents() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
    StageEvents(const StageEvents&) = delete;
    StageEvents& operator=(const StageEvents&) = delete;
    void mark(size_t k, hipStream_t st) {
        if (!on) return;
        if (e.size() <= k) e.resize(k + 1, nullptr);
        if (!e[k]) HIP_CHECK(hipEventCreate(&e[k]));
        HIP_CHECK(hipEventRecord(e[k], st));
    }
    double ms(size_t k) {   // between mark k and mark k + 1, both reached: the stream has been waited for
        float v = 0.f;
        if (on) HIP_CHECK(hipEventElapsedTime(&v, e[k], e[k + 1]));
        return v;
    }
};

// Items (replicates, families) per batch of a call whose device is the current one: the forced switch, else what half of the free device
// memory holds at bytes_each a piece, an eighth added (a DevBuf takes an eighth more than it is asked for), one at least; never more than
// cap.  so_pan_shared counts the 64 slack words of an item into bytes_each, so the eighth is taken of them too: its automatic batch may
// differ by rounding from one sized without -- no result depends on the batch size (the tests that force the batches show it).
inline size_t device_batch(const DeviceCall&, long long forced, size_t bytes_each, size_t cap) {
    size_t batch = forced > 0 ? (size_t)forced : 0;
    if (!batch) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        batch = std::max<size_t>(1, free_b / 2 / (bytes_each + bytes_each / 8));
    }
    return std::min(batch, cap);
}

// a result that has to lie in device memory as a whole: refused where it (an eighth added) takes more than half of what is free
inline void refuse_over_half_free(const std::string& who, const std::string& what, size_t bytes) {
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (bytes + bytes / 8 > free_b / 2)
        throw SoError(who + ": the " + what + " would take " + std::to_string(bytes) + " bytes, more than half of the free device memory (" + std::to_string(free_b) +
                      " bytes free): ask for fewer replicates per call");
}

#ifdef __HIPCC__
// draw k of replicate b from K columns (or rows): phy.py boot_columns(), splitmix64 in 64-bit integers that wrap
__device__ __forceinline__ u32 replicate_draw(ull seed, ull b, ull k, u32 K) {
    ull z = seed + ((b << 32) + k + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (u32)(((z >> 32) * (ull)K) >> 32);   // < K: the left factor is below 2^32
}
#endif
