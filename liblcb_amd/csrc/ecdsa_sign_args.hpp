// ecdsa_sign_args.hpp — the device-side description of one batch of signing
// or of key generation, the same at every limb count: what the kernel TUs and
// the C-ABI TUs of liblcb_ecdsa_sign_gpu.so and liblcb_ecdsa_wide_sign_gpu.so
// pass to each other.  B = 4 L bytes per number, L the curve's limb count.
#pragma once
#include <stdint.h>

namespace lcbec {

// Device-side description of one signing batch.
struct SignArgs {
    const uint8_t* hashes = nullptr;    // count x hash_size
    const uint8_t* priv = nullptr;      // nkeys x B
    const uint32_t* key_idx = nullptr;  // nullptr: key i for item i
    const uint8_t* rnd = nullptr;       // count x B
    uint8_t* sigs = nullptr;            // count x 2 B: r || s
    int32_t* status = nullptr;          // count
    uint64_t count = 0, nkeys = 0;
    uint32_t hash_size = 0;
    uint32_t le = 0;
};

// Key generation (from_rnd: in = rnd, priv is written) and public keys from
// private keys (in = the private keys, priv = nullptr).
struct KeyArgs {
    const uint8_t* in = nullptr;  // count x B
    uint8_t* priv = nullptr;      // count x B, or nullptr
    uint8_t* pub = nullptr;       // count x 2 B: x || y
    int32_t* status = nullptr;    // count
    uint64_t count = 0;
    uint32_t from_rnd = 0;
    uint32_t le = 0;
};

}  // namespace lcbec
