// lcb_ecdsa_wide_gpu.cpp — exported C-ABI of the batched ECDSA / GOST R 34.10
// signature verification on 384- and 512-bit curves
// (include/lcb_ecdsa_wide_gpu.h), built into liblcb_ecdsa_wide_gpu.so and
// linked against liblcb_hash_gpu.so for the shared runtime pieces
// (ensure_init, map_err).
//
// Device mode enqueues one kernel on the caller's stream and never
// synchronises; the per-curve constant block travels as a kernel argument.
// Host mode stages chunk by chunk through page-locked memory on a private
// stream: copy -> H2D -> kernel -> D2H -> copy, one chunk in flight (the
// kernel dwarfs the copies).  The staging context is host_stage.hpp's, the
// parsed curve table ecdsa_wide_host.hpp's.  It stages only public data and
// wipes nothing.  Nothing falls back to the CPU.
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "../../include/lcb_ecdsa_wide_gpu.h"
#include "../../include/lcb_hash_gpu.h"
#include "ecdsa_wide_host.hpp"
#include "ecdsa_wide_internal.hpp"
#include "host_stage.hpp"
#include "lcb_internal.hpp"

using namespace lcbgpu;
using namespace lcbec;

namespace {

void launch(int curve, const EcWideArgs& a, hipStream_t s) {
    if (kWideCurves[curve].bytes == 48)
        launch_ecdsa_wide_verify(a, wide_table().c12[curve], s);
    else
        launch_ecdsa_wide_verify(a, wide_table().c16[curve], s);
}

// ------------------------------------------------------------ host mode
// h / d: one chunk, hashes | sigs | keys | key_idx | status.  h2 / d2: the whole
// key table of a key_idx batch.
thread_local HostStage g_stage;
constexpr size_t kChunkItems = 1u << 16;

int verify_host(int curve, int le, const uint8_t* hashes, size_t hash_size, const uint8_t* sigs, const uint8_t* keys,
                size_t nkeys, const uint32_t* key_idx, size_t count, int32_t* status) {
    int dev = 0;
    LCB_HOST_TRY(hipGetDevice(&dev));
    const size_t B2 = 2 * (size_t)kWideCurves[curve].bytes;
    const size_t chunk = std::min(count, kChunkItems);
    const size_t o_sig = up16(chunk * hash_size), o_key = o_sig + chunk * B2;
    const size_t o_idx = o_key + (key_idx ? 0 : chunk * B2), o_st = o_idx + up16(chunk * 4);
    const size_t key_bytes = key_idx ? nkeys * B2 : 0;
    if (int rc = g_stage.ensure(dev, o_st + chunk * 4, key_bytes)) return rc;
    HostStage& S = g_stage;
    if (key_bytes) {
        memcpy(S.h2, keys, key_bytes);
        LCB_HOST_TRY(hipMemcpyAsync(S.d2, S.h2, key_bytes, hipMemcpyHostToDevice, S.st));
    }
    for (size_t i = 0; i < count; i += chunk) {
        const size_t n = std::min(chunk, count - i);
        memcpy(S.h, hashes + i * hash_size, n * hash_size);
        memcpy(S.h + o_sig, sigs + i * B2, n * B2);
        if (key_idx)
            memcpy(S.h + o_idx, key_idx + i, n * 4);
        else
            memcpy(S.h + o_key, keys + i * B2, n * B2);
        LCB_HOST_TRY(hipMemcpyAsync(S.d, S.h, o_st, hipMemcpyHostToDevice, S.st));
        EcWideArgs a;
        a.hashes = S.d;
        a.sigs = S.d + o_sig;
        a.keys = key_idx ? S.d2 : S.d + o_key;
        a.key_idx = key_idx ? reinterpret_cast<const uint32_t*>(S.d + o_idx) : nullptr;
        a.status = reinterpret_cast<int32_t*>(S.d + o_st);
        a.count = n;
        a.nkeys = key_idx ? nkeys : n;
        a.hash_size = (uint32_t)hash_size;
        a.le = le ? 1u : 0u;
        launch(curve, a, S.st);
        LCB_HOST_TRY(hipGetLastError());
        LCB_HOST_TRY(hipMemcpyAsync(S.h + o_st, S.d + o_st, n * 4, hipMemcpyDeviceToHost, S.st));
        LCB_HOST_TRY(hipStreamSynchronize(S.st));
        memcpy(status + i, S.h + o_st, n * 4);
    }
    return 0;
}

}  // namespace

extern "C" {

int lcb_ecdsa_wide_curve_count(void) { return kWideCurveCount; }

const char* lcb_ecdsa_wide_curve_name(int id) {
    return (id >= 0 && id < kWideCurveCount) ? kWideCurves[id].name : nullptr;
}

int lcb_ecdsa_wide_curve_id(const char* name) {
    if (!name) return -1;
    for (int id = 0; id < kWideCurveCount; ++id)
        if (strcmp(kWideCurves[id].name, name) == 0) return id;
    return -1;
}

int lcb_ecdsa_wide_curve_bytes(int id) { return (id >= 0 && id < kWideCurveCount) ? (int)kWideCurves[id].bytes : -1; }

int lcb_ecdsa_wide_curve_params(int id, uint8_t* out, uint32_t* algo, uint32_t* h) {
    if (!wide_known(id) || !out || !algo || !h) return EINVAL;
    memcpy(out, wide_table().raw[id], 6 * (size_t)kWideCurves[id].bytes);
    *algo = kWideCurves[id].algo;
    *h = kWideCofactor;
    return 0;
}

int lcb_ecdsa_wide_verify_batch(int curve, int le, const uint8_t* hashes, size_t hash_size, const uint8_t* sigs,
                                const uint8_t* pub_keys, size_t nkeys, const uint32_t* key_idx, size_t count,
                                int32_t* status, uint32_t flags, void* stream) {
    if (flags & ~LCB_HASH_F_DEVICE) return EINVAL;
    if (!wide_known(curve) || hash_size < 1 || hash_size > 128) return EINVAL;
    if (!key_idx && nkeys != count) return EINVAL;
    if (count > 0xffffffffull || nkeys > 0xffffffffull) return EINVAL;
    if (count == 0) return 0;
    if (!hashes || !sigs || !pub_keys || !status) return EINVAL;
    if (int rc = ensure_init()) return rc;
    if (flags & LCB_HASH_F_DEVICE) {
        EcWideArgs a;
        a.hashes = hashes;
        a.sigs = sigs;
        a.keys = pub_keys;
        a.key_idx = key_idx;
        a.status = status;
        a.count = count;
        a.nkeys = nkeys;
        a.hash_size = (uint32_t)hash_size;
        a.le = le ? 1u : 0u;
        launch(curve, a, reinterpret_cast<hipStream_t>(stream));
        return map_err(hipGetLastError());
    }
    return verify_host(curve, le, hashes, hash_size, sigs, pub_keys, nkeys, key_idx, count, status);
}

int ecdsa_verify_be_wide_batch(int curve, const uint8_t* hashes, size_t hash_size, const uint8_t* sigs,
                               const uint8_t* pub_keys, size_t nkeys, const uint32_t* key_idx, size_t count,
                               int32_t* status, uint32_t flags, void* stream) {
    return lcb_ecdsa_wide_verify_batch(curve, 0, hashes, hash_size, sigs, pub_keys, nkeys, key_idx, count, status,
                                       flags, stream);
}

int ecdsa_verify_le_wide_batch(int curve, const uint8_t* hashes, size_t hash_size, const uint8_t* sigs,
                               const uint8_t* pub_keys, size_t nkeys, const uint32_t* key_idx, size_t count,
                               int32_t* status, uint32_t flags, void* stream) {
    return lcb_ecdsa_wide_verify_batch(curve, 1, hashes, hash_size, sigs, pub_keys, nkeys, key_idx, count, status,
                                       flags, stream);
}

}  // extern "C"
