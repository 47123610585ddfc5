// mi_sa_host.h -- the host side every C entry point shares: the error channel, the exception guard, the device check and
// the owners of one call's device scratch, events and stream.  What an owner holds is released when its scope ends, on
// every way out.  No device code: plain g++ -D__HIP_PLATFORM_AMD__ compiles it (tests/host/scratch_main.cpp runs it
// over a fake runtime).
#pragma once

#include <hip/hip_runtime_api.h>

#include <exception>
#include <new>
#include <utility>
#include <vector>

#include "../../include/mi_sa.h"

namespace mi_sa_impl {

int fail(int code, const char *fmt, ...);

// No C++ exception may cross the C ABI: every extern "C" entry that allocates host memory runs its body through
// guarded(), which turns std::bad_alloc (and anything else) into an MI_E* code + mi_last_error() text.
template <typename F>
int guarded(F &&body) noexcept
{
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return fail(MI_ENOMEM, "out of host memory");
    } catch (const std::exception &e) {
        return fail(MI_EINVAL, "unexpected C++ exception: %s", e.what());
    } catch (...) {
        return fail(MI_EINVAL, "unexpected C++ exception");
    }
}

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return ::mi_sa_impl::fail(MI_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),  \
                                      __FILE__, __LINE__);                                       \
    } while (0)

#define MI_TRY(expr)                  \
    do {                              \
        const int rc_ = (expr);       \
        if (rc_ != MI_OK) return rc_; \
    } while (0)

// is there a device, is `device` one of them; makes it current
inline int pick_device(int device)
{
    int cnt = 0;
    const hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess || cnt <= 0) return fail(MI_ENODEV, "no HIP device visible (%s)", hipGetErrorString(e));
    if (device < 0 || device >= cnt) return fail(MI_EINVAL, "device %d out of range [0,%d)", device, cnt);
    HIP_TRY(hipSetDevice(device));
    return MI_OK;
}

struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

// device scratch of one call (a buffer that outlives the call is a DevArray member of its handle)
struct DevBufs : NoCopy {
    std::vector<void *> p;
    ~DevBufs()
    {
        for (void *b : p)
            if (b) (void)hipFree(b);
    }
    // at least one element, so that a count of 0 still yields a pointer; may throw std::bad_alloc (run under guarded())
    template <typename T>
    hipError_t alloc(T **out, size_t count)
    {
        *out = nullptr;
        p.push_back(nullptr);                                     // the slot first: a throwing growth cannot lose a buffer
        const hipError_t e = hipMalloc(&p.back(), (count ? count : 1) * sizeof(T));
        if (e != hipSuccess) p.back() = nullptr;
        *out = static_cast<T *>(p.back());
        return e;
    }
    // alloc(), then the copy of `count` elements from the host (none for a count of 0)
    template <typename T>
    hipError_t upload(T **out, const T *host, size_t count)
    {
        const hipError_t e = alloc(out, count);
        return e != hipSuccess || count == 0 ? e : hipMemcpy(*out, host, count * sizeof(T), hipMemcpyHostToDevice);
    }
};

// One device array of T that outlives a call, with its element count: a member of a handle, freed when the handle is
// deleted (mi_*_destroy).  Never dangling: null with count 0 after reset() and after a failed allocation, whatever the
// failed hipMalloc wrote.  Contents are not kept when the size changes.
template <typename T>
struct DevArray : NoCopy {
    T *p = nullptr;
    size_t count = 0;
    ~DevArray() { reset(); }
    operator T *() const { return p; }
    void reset()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        count = 0;
    }
    // exactly n elements; allocates at least one, so that a count of 0 still yields a pointer
    hipError_t resize(size_t n)
    {
        if (p && count == n) return hipSuccess;
        reset();
        void *raw = nullptr;
        const hipError_t e = hipMalloc(&raw, (n ? n : 1) * sizeof(T));
        if (e != hipSuccess) return e;
        p = static_cast<T *>(raw);
        count = n;
        return hipSuccess;
    }
    // at least n elements
    hipError_t reserve(size_t n) { return p && count >= n ? hipSuccess : resize(n); }
    // exactly n elements, copied from the host
    hipError_t upload(const T *host, size_t n)
    {
        const hipError_t e = resize(n);
        return e != hipSuccess || n == 0 ? e : hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t upload(const std::vector<T> &host) { return upload(host.data(), host.size()); }
    void swap(DevArray &o)
    {
        std::swap(p, o.p);
        std::swap(count, o.count);
    }
};

// N events: the holder creates them (HIP_TRY(hipEventCreate(&ev.e[i]))), the scope destroys them
template <int N>
struct Events : NoCopy {
    hipEvent_t e[N] = {};
    ~Events()
    {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

// the span between start() and stop() on stream `st`, in ms; stop() waits for it
struct Timer {
    Events<2> ev;
    int start(hipStream_t st)
    {
        HIP_TRY(hipEventCreate(&ev.e[0]));
        HIP_TRY(hipEventCreate(&ev.e[1]));
        HIP_TRY(hipEventRecord(ev.e[0], st));
        return MI_OK;
    }
    int stop(hipStream_t st, float *out_ms)
    {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev.e[1], st));
        HIP_TRY(hipEventSynchronize(ev.e[1]));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        if (out_ms) *out_ms = ms;
        return MI_OK;
    }
};

// a stream the holder creates into `st`; the scope (or the handle it is a member of) destroys it
struct ScopedStream : NoCopy {
    hipStream_t st = nullptr;
    operator hipStream_t() const { return st; }
    ~ScopedStream()
    {
        if (st) (void)hipStreamDestroy(st);
    }
};

}  // namespace mi_sa_impl
