// host_stage.hpp — the host-mode pieces that the libraries built beside
// liblcb_hash_gpu.so share (host only, header only): the "return map_err on a
// HIP error" macro, up16, the chunk size with its environment override, and
// the staging context of one thread.  Nothing here is exported: the functions
// are static and the struct is hidden, so every library carries its own copy
// and its own thread_local instance.  Not for the hash library's own files.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "lcb_internal.hpp"

#define LCB_HOST_TRY(expr)                                \
    do {                                                  \
        hipError_t _e = (expr);                           \
        if (_e != hipSuccess) return lcbgpu::map_err(_e); \
    } while (0)

namespace lcbgpu {

static inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

// Staging bytes per chunk: 64 MiB, or what the variable `env` holds (0 or
// unparsable: the default), never below `floor`.  Tests force a batch across
// a chunk boundary with it.
static inline size_t chunk_bytes(const char* env, size_t floor) {
    size_t v = 64ull << 20;
    if (const char* e = getenv(env)) {
        const unsigned long long x = strtoull(e, nullptr, 0);
        if (x) v = (size_t)x;
    }
    return std::max(v, floor);
}

// One thread's staging on one device: a private stream and two pairs of a
// page-locked and a device buffer (a chunk and what goes beside it: a key
// table, or per-message metadata).  The buffers only ever grow.
struct __attribute__((visibility("hidden"))) HostStage {
    int device = -1;
    hipStream_t st = nullptr;
    uint8_t *h = nullptr, *d = nullptr;    // the first pair, `cap` bytes each
    uint8_t *h2 = nullptr, *d2 = nullptr;  // the second pair, `cap2` bytes each; none while cap2 is 0
    size_t cap = 0, cap2 = 0;

    void release() {
        if (h) (void)hipHostFree(h);
        if (h2) (void)hipHostFree(h2);
        if (d) (void)hipFree(d);
        if (d2) (void)hipFree(d2);
        if (st) (void)hipStreamDestroy(st);
        h = d = h2 = d2 = nullptr;
        st = nullptr;
        cap = cap2 = 0;
        device = -1;
    }
    ~HostStage() { release(); }

    int ensure(int dev, size_t bytes, size_t bytes2) {
        if (device == dev && cap >= bytes && cap2 >= bytes2) return 0;
        const size_t nb = std::max(bytes, cap), nb2 = std::max(bytes2, cap2);
        release();
        device = dev;
        LCB_HOST_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        LCB_HOST_TRY(hipHostMalloc(reinterpret_cast<void**>(&h), nb, hipHostMallocDefault));
        LCB_HOST_TRY(hipMalloc(reinterpret_cast<void**>(&d), nb));
        if (nb2) {
            LCB_HOST_TRY(hipHostMalloc(reinterpret_cast<void**>(&h2), nb2, hipHostMallocDefault));
            LCB_HOST_TRY(hipMalloc(reinterpret_cast<void**>(&d2), nb2));
        }
        cap = nb;
        cap2 = nb2;
        return 0;
    }

    // Zeros over everything a call staged (`bytes` of the first pair, `bytes2`
    // of the second), on the host and on the device; waits.
    int wipe(size_t bytes, size_t bytes2) {
        hipError_t e = hipSuccess, e2;
        if (h) memset(h, 0, std::min(bytes, cap));
        if (h2) memset(h2, 0, std::min(bytes2, cap2));
        if (d && st && (e2 = hipMemsetAsync(d, 0, std::min(bytes, cap), st)) != hipSuccess) e = e2;
        if (d2 && st && bytes2 && (e2 = hipMemsetAsync(d2, 0, std::min(bytes2, cap2), st)) != hipSuccess) e = e2;
        if (st && (e2 = hipStreamSynchronize(st)) != hipSuccess) e = e2;
        return e == hipSuccess ? 0 : map_err(e);
    }
};

}  // namespace lcbgpu
