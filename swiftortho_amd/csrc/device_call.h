// device_call.h -- what an entry point that runs without a context (so_mcl*, so_cnc_*, so_apc*, so_orth_*, so_nr_expand) begins with:
// the device check, the scope of the call (device, switches, poison, one stream) and the small helpers every such call uses.
#pragma once
#include "common.h"

#include <algorithm>
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
    int waits = 0;        // host waits for the stream that went through read()

    explicit DeviceCall(int device, bool wait_for_device = false) : tn(begin(device, wait_for_device)), poison((int)tn.poison) { HIP_CHECK(hipStreamCreate(&st)); }
    ~DeviceCall() { (void)hipStreamSynchronize(st), (void)hipStreamDestroy(st); }
    DeviceCall(const DeviceCall&) = delete;
    DeviceCall& operator=(const DeviceCall&) = delete;

    // one host wait for one device word, or for two (a null b is skipped)
    u32 read(const u32* a) {
        u32 va = 0, none = 0;
        read(a, va, nullptr, none);
        return va;
    }
    void read(const u32* a, u32& va, const u32* b, u32& vb) {
        HIP_CHECK(hipMemcpyAsync(&va, a, sizeof(u32), hipMemcpyDeviceToHost, st));
        if (b) HIP_CHECK(hipMemcpyAsync(&vb, b, sizeof(u32), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        ++waits;
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
