// Stand-alone host program over csrc/mi_sa_host.h: the device check, the scope owners of a call's scratch, events and
// stream, and the owner of a handle's device array (DevArray), run against a fake HIP runtime defined here (counting fakes over malloc that keep the set of live handles,
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
static bool g_malloc_failed = false;                              // the failing call of this run was a hipMalloc
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
    if (failing()) { g_malloc_failed = true; return hipErrorOutOfMemory; }
    CHECK(size > 0);
    *ptr = acquire(size);
    return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    CHECK(kind == hipMemcpyHostToDevice && g_live.count(dst) && bytes > 0);
    if (failing()) return hipErrorInvalidValue;
    memcpy(dst, src, bytes);                                       // (past the end of either side: the sanitizer reports it)
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
// the device check, a scratch stream, four marks, scratch (one buffer of count 0, two uploads), a timed span, a nested
// owner that releases early (the symmetric trim of the SNN build), then success
static int handle_life();

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
        // upload: the allocation, then the copy; none for a count of 0 (the fake copy refuses 0 bytes), though a pointer
        // all the same.  A failed copy leaves the buffer with its owner: released once, where the scope ends.
        const int h_up[7] = {1, 2, 3, 4, 5, 6, 7};
        int *d_up = nullptr, *d_empty = nullptr;
        const size_t held = g_live.size();
        const hipError_t up = bufs.upload(&d_up, h_up, 7);
        CHECK(g_live.size() == held + (up != hipSuccess && g_malloc_failed ? 0 : 1));
        CHECK((d_up == nullptr) == (up != hipSuccess && g_malloc_failed));
        HIP_TRY(up);
        CHECK(d_up[0] == 1 && d_up[6] == 7);
        const int calls = g_calls;
        HIP_TRY(bufs.upload(&d_empty, static_cast<const int *>(nullptr), 0));
        CHECK(d_empty != nullptr && g_calls == calls + 1);        // (the hipMalloc alone)
        d_empty[0] = 1;
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
        return handle_life();
    });
}

// ---- the device arrays of a handle, through its life ---------------------------------------------------------------------
// four owners: uploads, one regrown larger and one smaller, an upload at another size, one reset early, the rest released
// where the scope ends.  After every step, failed or not, what is live beyond the caller's is exactly what the owners
// hold; an owner whose allocation failed is null with count 0.
static int handle_life()
{
    const size_t before = g_live.size();
    int rc = MI_OK;
    {
        DevArray<float> a;
        DevArray<int> b;
        DevArray<double> c, d;
        auto accounted = [&]() {
            size_t held = 0;
            for (void *q : {(void *)a.p, (void *)b.p, (void *)c.p, (void *)d.p})
                if (q) { CHECK(g_live.count(q)); ++held; }
            CHECK(g_live.size() == before + held);
            CHECK((a.p || a.count == 0) && (b.p || b.count == 0) && (c.p || c.count == 0) && (d.p || d.count == 0));
        };
#define STEP(owner, call)                                                                        \
    do {                                                                                         \
        const hipError_t err_ = owner.call;                                                       \
        accounted();                                                                             \
        if (err_ != hipSuccess && g_malloc_failed) CHECK(owner.p == nullptr && owner.count == 0);  \
        HIP_TRY(err_);                                                                           \
    } while (0)
        rc = [&]() -> int {
            const std::vector<float> ha(100, 2.0f);
            const int hb[7] = {1, 2, 3, 4, 5, 6, 7};
            const double hc[3] = {0.5, 1.5, 2.5};
            STEP(a, upload(ha));
            STEP(b, upload(hb, 7));
            CHECK(a.count == 100 && a[99] == 2.0f && b.count == 7 && b[6] == 7);
            STEP(c, resize(0));
            CHECK(c.p != nullptr && c.count == 0);                // a count of 0 still yields a pointer
            c[0] = 1.0;
            const float *kept = a;
            STEP(a, reserve(50));                                 // large enough already: the same buffer, no runtime call
            CHECK(a == kept && a.count == 100);
            STEP(a, reserve(300));                                // regrown larger
            CHECK(a.count == 300);
            a[299] = 1.0f;
            STEP(b, resize(3));                                   // ... and smaller: exactly three
            CHECK(b.count == 3);
            b[2] = 1;
            STEP(b, upload(hb, 5));                               // an upload at another size
            CHECK(b.count == 5 && b[4] == 5);
            STEP(c, upload(hc, 3));
            CHECK(c.count == 3 && c[2] == 2.5);
            STEP(d, upload(hc, 2));                               // filled beside c, then in its place
            c.swap(d);
            CHECK(c.count == 2 && c[1] == 1.5 && d.count == 3);
            return MI_OK;
        }();
#undef STEP
        accounted();
        a.reset();                                                // released early
        CHECK(a.p == nullptr && a.count == 0);
        a.reset();                                                // ... and once
        accounted();
    }
    CHECK(g_live.size() == before);                               // the rest went where the scope ended
    return rc;
}

static int run(int fail_at, int device, float *out_ms)
{
    g_calls = 0;
    g_fail_at = fail_at;
    g_malloc_failed = false;
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
    CHECK(total >= 41);
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
