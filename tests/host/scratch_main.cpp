// Stand-alone host program over csrc/mi_sa_host.h: the device check and the scope owners of a call's scratch, events and
// stream, run against a fake HIP runtime defined here (counting fakes over malloc that keep the set of live handles,
// abort on a release of something not live, and fail the k-th call on request).  A function shaped like the library's
// entry points is failed at every runtime call in turn: it must answer MI_EHIP (or the device check's code) and leave
// nothing live.  Built with -fsanitize=address,undefined by tests/test_scratch_host.py, without the HIP runtime; prints
// "ok" and returns 0.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "../../scrna_seq_qannealing_clustering_amd/csrc/mi_sa_host.h"

using namespace mi_sa_impl;

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond);    \
            exit(1);                                                                    \
        }                                                                               \
    } while (0)

// ---- the fake runtime -------------------------------------------------------------------------------------------------
static std::set<void *> g_live;
static int g_calls = 0, g_fail_at = 0, g_devices = 2, g_current = -1;
static char g_last_error[256];

// every call that can fail counts; the g_fail_at-th one does (releases cannot: the owners ignore their results)
static bool failing() { return ++g_calls == g_fail_at; }

static void *acquire(size_t bytes)
{
    void *h = malloc(bytes);
    CHECK(h != nullptr);
    g_live.insert(h);
    return h;
}

static void release(void *h)
{
    if (!g_live.erase(h)) {
        fprintf(stderr, "release of %p, which is not live\n", h);
        abort();
    }
    free(h);
}

hipError_t hipMalloc(void **ptr, size_t size)
{
    *ptr = reinterpret_cast<void *>(0x1);                          // (what a failed call leaves behind must not be freed)
    if (failing()) return hipErrorOutOfMemory;
    CHECK(size > 0);
    *ptr = acquire(size);
    return hipSuccess;
}
hipError_t hipFree(void *ptr) { release(ptr); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *event)
{
    if (failing()) return hipErrorOutOfMemory;
    *event = static_cast<hipEvent_t>(acquire(1));
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t event) { release(event); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream)
{
    CHECK(g_live.count(event) && (!stream || g_live.count(stream)));
    return failing() ? hipErrorInvalidHandle : hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t event)
{
    CHECK(g_live.count(event));
    return failing() ? hipErrorInvalidHandle : hipSuccess;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t start, hipEvent_t stop)
{
    CHECK(g_live.count(start) && g_live.count(stop));
    if (failing()) return hipErrorInvalidHandle;
    *ms = 1.5f;
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *stream, unsigned int)
{
    if (failing()) return hipErrorOutOfMemory;
    *stream = static_cast<hipStream_t>(acquire(1));
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t stream) { release(stream); return hipSuccess; }
hipError_t hipGetDeviceCount(int *count)
{
    if (failing()) return hipErrorNoDevice;
    *count = g_devices;
    return hipSuccess;
}
hipError_t hipSetDevice(int device)
{
    if (failing()) return hipErrorInvalidDevice;
    g_current = device;
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return failing() ? hipErrorLaunchFailure : hipSuccess; }
const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "fake runtime error"; }

int mi_sa_impl::fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof g_last_error, fmt, ap);
    va_end(ap);
    return code;
}

// ---- a call shaped like the library's -----------------------------------------------------------------------------------
// the device check, a scratch stream, four marks, scratch (one buffer of count 0), a timed span, a nested owner that
// releases early (the symmetric trim of the SNN build), then success
static int entry(int device, float *out_ms)
{
    MI_TRY(pick_device(device));
    return guarded([&]() -> int {
        ScopedStream stream;
        HIP_TRY(hipStreamCreateWithFlags(&stream.st, hipStreamNonBlocking));
        const hipStream_t st = stream.st;
        Events<4> ev;
        for (auto &e : ev.e) HIP_TRY(hipEventCreate(&e));
        DevBufs bufs;
        float *d_a = nullptr;
        int *d_b = nullptr;
        double *d_none = nullptr;
        HIP_TRY(bufs.alloc(&d_a, 100));
        HIP_TRY(bufs.alloc(&d_b, 7));
        HIP_TRY(bufs.alloc(&d_none, 0));
        CHECK(d_none != nullptr);
        d_a[99] = 1.0f; d_b[6] = 1; d_none[0] = 1.0;              // (each at least as large as asked: the sanitizer checks)
        HIP_TRY(hipEventRecord(ev.e[0], st));
        Timer t;
        MI_TRY(t.start(st));
        const size_t before = g_live.size();
        {
            DevBufs inner;
            unsigned int *d_ctrl = nullptr, *d_done = nullptr;
            unsigned char *d_save = nullptr;
            HIP_TRY(inner.alloc(&d_ctrl, 2));
            HIP_TRY(inner.alloc(&d_done, 33));
            HIP_TRY(inner.alloc(&d_save, 1));
            CHECK(g_live.size() == before + 3);
            HIP_TRY(hipGetLastError());
        }
        CHECK(g_live.size() == before);                           // released where the inner scope ends, not at the return
        MI_TRY(t.stop(st, out_ms));
        for (int i = 1; i < 4; ++i) HIP_TRY(hipEventRecord(ev.e[i], st));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[3]));
        return MI_OK;
    });
}

static int run(int fail_at, int device, float *out_ms)
{
    g_calls = 0;
    g_fail_at = fail_at;
    g_last_error[0] = 0;
    const int rc = entry(device, out_ms);
    CHECK(g_live.empty());
    return rc;
}

int main()
{
    float ms = 0.0f;
    CHECK(run(0, 1, &ms) == MI_OK && ms == 1.5f && g_current == 1);
    const int total = g_calls;
    CHECK(total >= 25);
    CHECK(run(0, 0, nullptr) == MI_OK && g_calls == total);       // out_ms may be null
    for (int k = 1; k <= total; ++k) {
        const int rc = run(k, 0, &ms);
        CHECK(g_calls == k);                                      // it stopped at the failure
        CHECK(rc == (k == 1 ? MI_ENODEV : MI_EHIP));              // (call 1 is hipGetDeviceCount)
        CHECK(strstr(g_last_error, "fake runtime error") != nullptr);
    }
    // the device check's own answers: nothing else is called after them
    CHECK(run(0, -1, &ms) == MI_EINVAL && g_calls == 1 && strstr(g_last_error, "device -1 out of range [0,2)"));
    CHECK(run(0, 2, &ms) == MI_EINVAL && g_calls == 1);
    g_devices = 0;
    CHECK(run(0, 0, &ms) == MI_ENODEV && g_calls == 1 && strstr(g_last_error, "no HIP device visible"));
    printf("ok: %d runtime calls on the success path, each failed in turn\n", total);
    return 0;
}
