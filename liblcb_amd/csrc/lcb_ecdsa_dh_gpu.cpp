// lcb_ecdsa_dh_gpu.cpp — exported C-ABI of batched ECDH key agreement
// (include/lcb_ecdsa_dh_gpu.h), built into liblcb_ecdsa_dh_gpu.so and linked
// against liblcb_hash_gpu.so for the shared runtime pieces (ensure_init,
// map_err).  The curve table is ecdsa_curves.hpp, parsed here by
// ecdsa_host.hpp; neither the verification nor the signing library is linked.
//
// Device mode enqueues one kernel on the caller's stream and never
// synchronises.  Host mode stages chunk by chunk through page-locked memory on
// a private stream: copy -> H2D -> kernel -> D2H -> copy, one chunk in flight;
// a key table that goes with an index array is staged whole, once.  After the
// last chunk every staging buffer, page-locked and on the device, is
// overwritten with zeros: they held private keys and shared secrets (the
// staging context and its wipe() are host_stage.hpp's).  Nothing falls back
// to the CPU.
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "../../include/lcb_ecdsa_dh_gpu.h"
#include "../../include/lcb_hash_gpu.h"
#include "ecdsa_host.hpp"
#include "ecdsa_dh_internal.hpp"
#include "host_stage.hpp"
#include "lcb_internal.hpp"

using namespace lcbgpu;
using namespace lcbec;

namespace {

// ------------------------------------------------------------ host mode
// h / d: one chunk.  h2 / d2: the whole key tables of an indexed batch.
thread_local HostStage g_stage;
constexpr size_t kChunkItems = 1u << 18;

// One chunk: pub | priv | pub_idx | priv_idx | shared | status.  A part whose
// keys come from a table is empty.  The tables: pub | priv.
struct DhLayout {
    size_t chunk, o_priv, o_pidx, o_didx, o_out, o_st, bytes, k_priv, key_bytes;
};

int dh_chunks(HostStage& S, const DhLayout& y, const Curve<kLimbs>& c, int le, const uint8_t* pub, size_t npub,
              const uint32_t* pub_idx, const uint8_t* priv, size_t npriv, const uint32_t* priv_idx, size_t count,
              uint8_t* shared, int32_t* status) {
    if (y.key_bytes) {
        if (pub_idx) memcpy(S.h2, pub, npub * 2 * kNumBytes);
        if (priv_idx) memcpy(S.h2 + y.k_priv, priv, npriv * kNumBytes);
        LCB_HOST_TRY(hipMemcpyAsync(S.d2, S.h2, y.key_bytes, hipMemcpyHostToDevice, S.st));
    }
    for (size_t i = 0; i < count; i += y.chunk) {
        const size_t n = std::min(y.chunk, count - i);
        if (pub_idx)
            memcpy(S.h + y.o_pidx, pub_idx + i, n * 4);
        else
            memcpy(S.h, pub + i * 2 * kNumBytes, n * 2 * kNumBytes);
        if (priv_idx)
            memcpy(S.h + y.o_didx, priv_idx + i, n * 4);
        else
            memcpy(S.h + y.o_priv, priv + i * kNumBytes, n * kNumBytes);
        LCB_HOST_TRY(hipMemcpyAsync(S.d, S.h, y.o_out, hipMemcpyHostToDevice, S.st));
        DhArgs a;
        a.pub = pub_idx ? S.d2 : S.d;
        a.pub_idx = pub_idx ? reinterpret_cast<const uint32_t*>(S.d + y.o_pidx) : nullptr;
        a.priv = priv_idx ? S.d2 + y.k_priv : S.d + y.o_priv;
        a.priv_idx = priv_idx ? reinterpret_cast<const uint32_t*>(S.d + y.o_didx) : nullptr;
        a.shared = S.d + y.o_out;
        a.status = reinterpret_cast<int32_t*>(S.d + y.o_st);
        a.count = n;
        a.npub = pub_idx ? npub : n;
        a.npriv = priv_idx ? npriv : n;
        a.le = le ? 1u : 0u;
        launch_ecdsa_dh(a, c, S.st);
        LCB_HOST_TRY(hipGetLastError());
        LCB_HOST_TRY(
            hipMemcpyAsync(S.h + y.o_out, S.d + y.o_out, y.o_st - y.o_out + n * 4, hipMemcpyDeviceToHost, S.st));
        LCB_HOST_TRY(hipStreamSynchronize(S.st));
        memcpy(shared + i * kNumBytes, S.h + y.o_out, n * kNumBytes);
        memcpy(status + i, S.h + y.o_st, n * 4);
    }
    return 0;
}

int dh_host(const Curve<kLimbs>& c, int le, const uint8_t* pub, size_t npub, const uint32_t* pub_idx,
            const uint8_t* priv, size_t npriv, const uint32_t* priv_idx, size_t count, uint8_t* shared,
            int32_t* status) {
    int dev = 0;
    LCB_HOST_TRY(hipGetDevice(&dev));
    DhLayout y;
    y.chunk = std::min(count, kChunkItems);
    y.o_priv = pub_idx ? 0 : y.chunk * 2 * kNumBytes;
    y.o_pidx = y.o_priv + (priv_idx ? 0 : y.chunk * kNumBytes);
    y.o_didx = y.o_pidx + (pub_idx ? up16(y.chunk * 4) : 0);
    y.o_out = y.o_didx + (priv_idx ? up16(y.chunk * 4) : 0);
    y.o_st = y.o_out + y.chunk * kNumBytes;
    y.bytes = y.o_st + y.chunk * 4;
    y.k_priv = pub_idx ? npub * 2 * kNumBytes : 0;
    y.key_bytes = y.k_priv + (priv_idx ? npriv * kNumBytes : 0);
    if (int rc = g_stage.ensure(dev, y.bytes, y.key_bytes)) return rc;
    const int rc = dh_chunks(g_stage, y, c, le, pub, npub, pub_idx, priv, npriv, priv_idx, count, shared, status);
    const int wrc = g_stage.wipe(y.bytes, y.key_bytes);  // also after an error
    return rc ? rc : wrc;
}

}  // namespace

extern "C" {

int lcb_ecdsa_dh_batch(int curve, int le, int use_cofactor, const uint8_t* pub_keys, size_t npub,
                       const uint32_t* pub_idx, const uint8_t* priv_keys, size_t npriv, const uint32_t* priv_idx,
                       size_t count, uint8_t* shared, int32_t* status, uint32_t flags, void* stream) {
    (void)use_cofactor;  // h = 1 on every curve of the table: h d = d
    static_assert(kCofactor == 1, "use_cofactor would have to multiply d by h mod n");
    if (flags & ~LCB_HASH_F_DEVICE) return EINVAL;
    if (!known(curve)) return EINVAL;
    if ((!pub_idx && npub != count) || (!priv_idx && npriv != count)) return EINVAL;
    if (count > 0xffffffffull || npub > 0xffffffffull || npriv > 0xffffffffull) return EINVAL;
    if (count == 0) return 0;
    if (!pub_keys || !priv_keys || !shared || !status) return EINVAL;
    if (int rc = ensure_init()) return rc;
    const Curve<kLimbs>& c = table().c[curve];
    if (flags & LCB_HASH_F_DEVICE) {
        DhArgs a;
        a.pub = pub_keys;
        a.pub_idx = pub_idx;
        a.priv = priv_keys;
        a.priv_idx = priv_idx;
        a.shared = shared;
        a.status = status;
        a.count = count;
        a.npub = npub;
        a.npriv = npriv;
        a.le = le ? 1u : 0u;
        launch_ecdsa_dh(a, c, reinterpret_cast<hipStream_t>(stream));
        return map_err(hipGetLastError());
    }
    return dh_host(c, le, pub_keys, npub, pub_idx, priv_keys, npriv, priv_idx, count, shared, status);
}

int ecdsa_dh_be_batch(int curve, int use_cofactor, const uint8_t* pub_keys, size_t npub, const uint32_t* pub_idx,
                      const uint8_t* priv_keys, size_t npriv, const uint32_t* priv_idx, size_t count,
                      uint8_t* shared, int32_t* status, uint32_t flags, void* stream) {
    return lcb_ecdsa_dh_batch(curve, 0, use_cofactor, pub_keys, npub, pub_idx, priv_keys, npriv, priv_idx, count,
                              shared, status, flags, stream);
}

int ecdsa_dh_le_batch(int curve, int use_cofactor, const uint8_t* pub_keys, size_t npub, const uint32_t* pub_idx,
                      const uint8_t* priv_keys, size_t npriv, const uint32_t* priv_idx, size_t count,
                      uint8_t* shared, int32_t* status, uint32_t flags, void* stream) {
    return lcb_ecdsa_dh_batch(curve, 1, use_cofactor, pub_keys, npub, pub_idx, priv_keys, npriv, priv_idx, count,
                              shared, status, flags, stream);
}

}  // extern "C"
