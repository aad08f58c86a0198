// device_call.h -- what an entry point that runs without a context (so_mcl*, so_cnc_*, so_apc*, so_orth_*, so_rbh_*, so_nr_expand) begins
// and ends with: the device check, the scope of the call (DeviceCall: device, switches, poison, one stream, its counted host waits), the
// host arrays of a result (host_array, host_copy; result_slots -> fill_empty_slots / release_slots), SortedGroups (stable sort of
// (key, index) pairs and the bounds of the key groups) and the epilogue every entry point ends through (guarded_call).
#pragma once
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <array>
#include <cstring>
#include <string>

#define NONE32 0xFFFFFFFFu   // no position / no row yet (both stay below 2^32 - 1); what a memset of 0xFF leaves

// the device, or the refusal: before the empty-input return, and before anything touches the device
inline void check_device(const char* who, int device) {
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) throw SoError(std::string(who) + ": no HIP device available (libsohit has no CPU fallback)");
    if (device < 0 || device >= nd) throw SoError(std::string(who) + ": device index out of range");
}

// The scope of one call that has something to launch.  Declare it BEFORE every DevBuf of the call: the buffers then go first, and the
// stream they were queued on is waited for and destroyed after them, whichever way the call ends.  (mcl.hip's Mcl keeps the handle its
// methods launch on: `m.st = call.st`, with m declared after the scope like any other owner of buffers.)
// wait_for_device: the call reads records another stream wrote (so_orth_*_records, so_nr_expand) -- everything queued on the device so
// far is waited for before this call's own stream exists.
struct DeviceCall {
    Tune tn;              // no context: the switches are read per call
    PoisonScope poison;   // ... and set before the first DevBuf::ensure
    hipStream_t st = nullptr;
    int waits = 0;        // host waits for the stream that went through wait() / read()

    explicit DeviceCall(int device, bool wait_for_device = false) : tn(begin(device, wait_for_device)), poison((int)tn.poison) { HIP_CHECK(hipStreamCreate(&st)); }
    ~DeviceCall() { (void)hipStreamSynchronize(st), (void)hipStreamDestroy(st); }
    DeviceCall(const DeviceCall&) = delete;
    DeviceCall& operator=(const DeviceCall&) = delete;

    // one host wait for everything queued on the stream so far
    void wait() {
        HIP_CHECK(hipStreamSynchronize(st));
        ++waits;
    }
    // queue the copy of n device elements to the host: they have arrived after the next wait().  Several words that one decision needs
    // are fetched one after the other and share that wait.
    template <class T>
    void fetch(T* h, const T* d, size_t n = 1) {
        HIP_CHECK(hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, st));
    }
    // one host wait for one device word, or for two (a null b is skipped)
    u32 read(const u32* a) {
        u32 va = 0, none = 0;
        read(a, va, nullptr, none);
        return va;
    }
    void read(const u32* a, u32& va, const u32* b, u32& vb) {
        fetch(&va, a);
        if (b) fetch(&vb, b);
        wait();
    }

private:
    static Tune begin(int device, bool wait_for_device) {
        HIP_CHECK(hipSetDevice(device));
        if (wait_for_device) HIP_CHECK(hipDeviceSynchronize());
        Tune t;
        t.read();
        return t;
    }
};

// a host array of n elements that the result's free function can release (never a null pointer for n = 0)
template <class T>
T* host_array(const char* who, size_t n) {
    T* p = (T*)malloc(std::max<size_t>(n, 1) * sizeof(T));
    if (!p) throw SoError(std::string(who) + ": out of host memory");
    return p;
}

// n device elements in such a host array; the copy is queued on st (on failure the array is gone)
template <class T>
T* host_copy(const char* who, const T* d, size_t n, hipStream_t st) {
    T* h = host_array<T>(who, n);
    if (n) {
        const hipError_t e = hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) {
            free(h);
            HIP_CHECK(e);
        }
    }
    return h;
}

// The pointer slots of a result struct, named once: `auto slots(so_x* r) { return result_slots(&r->a, &r->b, ...); }`.
template <class... P>
std::array<void**, sizeof...(P)> result_slots(P**... p) {
    return {{(void**)p...}};
}
// a result of no rows still hands out arrays that its free function can release
template <size_t N>
void fill_empty_slots(const std::array<void**, N>& slots) {
    for (void** p : slots)
        if (!*p) *p = calloc(1, 8);
}
// what a so_*_free does: every array released, the struct zeroed
template <class R, size_t N>
void release_slots(R* r, const std::array<void**, N>& slots) {
    for (void** p : slots) free(*p);
    memset(r, 0, sizeof *r);
}

// The epilogue of an entry point: body() is the call; it throws to refuse and returns early where there is nothing (more) to do.
// 0: done, the module's error string cleared.  1: the message is in the error string and what the result held so far is released.
template <class R, class Free, class Body>
int guarded_call(std::string& err, R* out, Free free_result, Body body) {
    try {
        body();
        err.clear();
        return 0;
    } catch (const std::exception& e) {
        if (out) free_result(out);
        err = e.what();
        return 1;
    }
}

// n host elements into a buffer of the call; the copy has left the host array when this returns (it may go away before the stream is waited for)
template <class T>
void upload(DevBuf<T>& d, const T* h, size_t n, hipStream_t st) {
    d.ensure(n + 2);
    if (!n) return;
    HIP_CHECK(hipMemcpyAsync(d.p, h, n * sizeof(T), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
}

// one lane per element, 256 to a workgroup
inline dim3 grid256(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
#ifdef __HIPCC__
__device__ __forceinline__ size_t tid256() { return (size_t)blockIdx.x * 256u + threadIdx.x; }
#endif

// (key, index) pairs sorted by key -- a stable radix sort: the indices of one key keep their order -- and the bounds of the key groups:
// start[g] = first position of group g, start[nseg] = n; rid[i] = group of position i, from 1.  segments() costs the call one wait.
struct SortedGroups {
    DevBuf<u64> skey;
    DevBuf<u32> sidx, head, rid, start, tmp;
    DevBuf<u8> sort_tmp;
    u32 nseg = 0;
    void sort(DeviceCall& call, const u64* key, const u32* idx, u32 n, int bits) {
        skey.ensure(n + 2), sidx.ensure(n + 2);
        const size_t tb = sort_pairs_u64_u32_temp_bytes(n, bits);
        sort_tmp.ensure(tb + 16);
        sort_pairs_u64_u32(sort_tmp.p, tb, key, skey.p, idx, sidx.p, n, bits, call.st);
    }
    void segments(DeviceCall& call, u32 n) {
        head.ensure(n + 2), rid.ensure(n + 2), tmp.ensure(scan_u32_temp_elems(n) + 2);
        const u32* d_nseg = key_runs(skey.p, n, head.p, rid.p, tmp.p, call.st);
        HIP_CHECK(hipGetLastError());
        nseg = call.read(d_nseg);
        start.ensure((size_t)nseg + 3);
        run_starts(head.p, rid.p, n, d_nseg, start.p, call.st);
    }
};
