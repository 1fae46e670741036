// rt_host.h -- private to the two host files of the C ABI (not installed): what rt_api.cpp (scenes, renders, jobs) and
// rt_post.cpp (the image-space stages) both need.  Everything here that has external linkage only so that the two files can
// share it is hidden: the library's dynamic symbol table does not know it.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "../../include/rt_mi355x.h"
#include "rt_launch.h"

#define RT_HIDDEN __attribute__((visibility("hidden")))

// the message rt_last_error() returns: one thread-local, in rt_api.cpp
RT_HIDDEN rt_status fail(rt_status st, const char *fmt, ...);
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(RT_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

RT_HIDDEN bool device_is_gfx950(int dev);
RT_HIDDEN void camera_setup(const rt_camera &cam, DevCamera &dc);      // of RenderPixel (rt_api.cpp)
// rt_scene_destroy of the last scene: the per-device scratch of the image-space stages goes with it (rt_post.cpp)
RT_HIDDEN void post_release_all();

struct DevBuf {
    void *p = nullptr; size_t bytes = 0;
    rt_status ensure(size_t n)
    {
        if (n <= bytes && p) return RT_OK;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        if (n == 0) n = 16;
        HIP_TRY(hipMalloc(&p, n));
        bytes = n;
        return RT_OK;
    }
    rt_status upload(const void *src, size_t n)
    {
        rt_status st = ensure(n);
        if (st) return st;
        if (n) HIP_TRY(hipMemcpy(p, src, n, hipMemcpyHostToDevice));
        return RT_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};
// a DevBuf released when its scope ends (DeviceState releases its own explicitly, on its device)
struct ScopedDevBuf : DevBuf {
    ScopedDevBuf() = default;
    ScopedDevBuf(const ScopedDevBuf &) = delete;
    ScopedDevBuf &operator=(const ScopedDevBuf &) = delete;
    ~ScopedDevBuf() { release(); }
};

// an owned hipEvent_t: destroyed with its owner, handed on by a move
struct RT_HIDDEN Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e, flags); }      // once per Event
    operator hipEvent_t() const { return e; }
};
