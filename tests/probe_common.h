// probe_common.h -- test-only: what the kernel probes (adaptive_probe.hip, denoise_probe.hip) share.  A device array that is a copy of
// a host array or 0xFF bytes, the first-error macro, and the check that ends an entry point.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace {

#define PROBE_TRY(expr)                          \
    do {                                         \
        const hipError_t e_ = (expr);            \
        if (e_ != hipSuccess && st == hipSuccess) st = e_; \
    } while (0)

// Device array of `count` elements: a copy of `host`, or 0xFF bytes when host is null.  Freed with the object; any failure is
// kept in `st` and makes the pointer null.
template <typename T>
struct Buf {
    T *d = nullptr;
    size_t n = 0;
    hipError_t st = hipSuccess;
    Buf(const T *host, size_t count) : n(count) {
        PROBE_TRY(hipMalloc(reinterpret_cast<void **>(&d), (count ? count : 1) * sizeof(T)));
        if (st != hipSuccess) { d = nullptr; return; }
        if (host && count) PROBE_TRY(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
        else PROBE_TRY(hipMemset(d, 0xFF, (count ? count : 1) * sizeof(T)));
    }
    ~Buf() { if (d) (void)hipFree(d); }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    hipError_t download(T *host) {
        if (st == hipSuccess && n) PROBE_TRY(hipMemcpy(host, d, n * sizeof(T), hipMemcpyDeviceToHost));
        return st;
    }
};

inline int finish(hipError_t st) {
    PROBE_TRY(hipGetLastError());
    PROBE_TRY(hipDeviceSynchronize());
    return (int)st;
}

}  // namespace
