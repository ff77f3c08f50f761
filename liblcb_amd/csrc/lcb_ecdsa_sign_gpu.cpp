// lcb_ecdsa_sign_gpu.cpp — exported C-ABI of batched ECDSA / GOST R 34.10
// signing, key generation and public keys from private keys
// (include/lcb_ecdsa_sign_gpu.h), built into liblcb_ecdsa_sign_gpu.so and
// linked against liblcb_hash_gpu.so for the shared runtime pieces
// (ensure_init, map_err).  The curve table is ecdsa_curves.hpp, parsed here
// by ecdsa_host.hpp; the verification library is not linked.
//
// Here are the argument checks and the exported wrappers.  The window-table
// cache, the host-mode staging with its wipe and the launch of either memory
// mode are ecdsa_sign_host.hpp's, shared with the wide library.
#include <errno.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "../../include/lcb_ecdsa_sign_gpu.h"
#include "../../include/lcb_hash_gpu.h"
#include "ecdsa_host.hpp"
#include "ecdsa_sign_host.hpp"
#include "ecdsa_sign_internal.hpp"
#include "lcb_internal.hpp"

using namespace lcbgpu;
using namespace lcbec;

namespace {

// What ecdsa_sign_host.hpp takes from this library.
struct Lib {
    static constexpr size_t kChunkItems = 1u << 18;
    static void sign(const SignArgs& a, const Curve<kLimbs>& c, const Table* t, hipStream_t s) {
        launch_ecdsa_sign(a, c, t, s);
    }
    static void keys(const KeyArgs& a, const Curve<kLimbs>& c, const Table* t, hipStream_t s) {
        launch_ecdsa_keys(a, c, t, s);
    }
};

int keys_batch(int curve, int le, bool from_rnd, const uint8_t* in, size_t count, uint8_t* priv, uint8_t* pub,
               int32_t* status, uint32_t flags, void* stream) {
    if (flags & ~LCB_HASH_F_DEVICE) return EINVAL;
    if (!known(curve)) return EINVAL;
    if (count > 0xffffffffull) return EINVAL;
    if (count == 0) return 0;
    if (!in || !pub || !status || (from_rnd && !priv)) return EINVAL;
    if (int rc = ensure_init()) return rc;
    return keys_run<Lib>(curve, table().c[curve], le, from_rnd, in, count, priv, pub, status, flags, stream);
}

}  // namespace

extern "C" {

int lcb_ecdsa_sign_batch(int curve, int le, const uint8_t* hashes, size_t hash_size, const uint8_t* priv_keys,
                         size_t nkeys, const uint32_t* key_idx, const uint8_t* rnd, size_t count, uint8_t* sigs,
                         int32_t* status, uint32_t flags, void* stream) {
    if (flags & ~LCB_HASH_F_DEVICE) return EINVAL;
    if (!known(curve) || hash_size < 1 || hash_size > 64) return EINVAL;
    if (!key_idx && nkeys != count) return EINVAL;
    if (count > 0xffffffffull || nkeys > 0xffffffffull) return EINVAL;
    if (count == 0) return 0;
    if (!hashes || !priv_keys || !rnd || !sigs || !status) return EINVAL;
    if (int rc = ensure_init()) return rc;
    return sign_run<Lib>(curve, table().c[curve], le, hashes, hash_size, priv_keys, nkeys, key_idx, rnd, count, sigs,
                         status, flags, stream);
}

int lcb_ecdsa_key_gen_batch(int curve, int le, const uint8_t* rnd, size_t count, uint8_t* priv_keys,
                            uint8_t* pub_keys, int32_t* status, uint32_t flags, void* stream) {
    return keys_batch(curve, le, true, rnd, count, priv_keys, pub_keys, status, flags, stream);
}

int lcb_ecdsa_pub_key_batch(int curve, int le, const uint8_t* priv_keys, size_t count, uint8_t* pub_keys,
                            int32_t* status, uint32_t flags, void* stream) {
    return keys_batch(curve, le, false, priv_keys, count, nullptr, pub_keys, status, flags, stream);
}

int ecdsa_sign_be_batch(int curve, const uint8_t* hashes, size_t hash_size, const uint8_t* priv_keys, size_t nkeys,
                        const uint32_t* key_idx, const uint8_t* rnd, size_t count, uint8_t* sigs, int32_t* status,
                        uint32_t flags, void* stream) {
    return lcb_ecdsa_sign_batch(curve, 0, hashes, hash_size, priv_keys, nkeys, key_idx, rnd, count, sigs, status,
                                flags, stream);
}

int ecdsa_sign_le_batch(int curve, const uint8_t* hashes, size_t hash_size, const uint8_t* priv_keys, size_t nkeys,
                        const uint32_t* key_idx, const uint8_t* rnd, size_t count, uint8_t* sigs, int32_t* status,
                        uint32_t flags, void* stream) {
    return lcb_ecdsa_sign_batch(curve, 1, hashes, hash_size, priv_keys, nkeys, key_idx, rnd, count, sigs, status,
                                flags, stream);
}

int ecdsa_key_gen_be_batch(int curve, const uint8_t* rnd, size_t count, uint8_t* priv_keys, uint8_t* pub_keys,
                           int32_t* status, uint32_t flags, void* stream) {
    return lcb_ecdsa_key_gen_batch(curve, 0, rnd, count, priv_keys, pub_keys, status, flags, stream);
}

int ecdsa_key_gen_le_batch(int curve, const uint8_t* rnd, size_t count, uint8_t* priv_keys, uint8_t* pub_keys,
                           int32_t* status, uint32_t flags, void* stream) {
    return lcb_ecdsa_key_gen_batch(curve, 1, rnd, count, priv_keys, pub_keys, status, flags, stream);
}

int ecdsa_recover_pub_key_from_priv_key_be_batch(int curve, const uint8_t* priv_keys, size_t count,
                                                 uint8_t* pub_keys, int32_t* status, uint32_t flags, void* stream) {
    return lcb_ecdsa_pub_key_batch(curve, 0, priv_keys, count, pub_keys, status, flags, stream);
}

int ecdsa_recover_pub_key_from_priv_key_le_batch(int curve, const uint8_t* priv_keys, size_t count,
                                                 uint8_t* pub_keys, int32_t* status, uint32_t flags, void* stream) {
    return lcb_ecdsa_pub_key_batch(curve, 1, priv_keys, count, pub_keys, status, flags, stream);
}

}  // extern "C"
