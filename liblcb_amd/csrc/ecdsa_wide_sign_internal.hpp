// ecdsa_wide_sign_internal.hpp — types shared by the kernel TU and the C-ABI
// TU of liblcb_ecdsa_wide_sign_gpu.so (include/lcb_ecdsa_wide_sign_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ecdsa_sign_math.hpp"

namespace lcbec {

constexpr int kLimbs384 = 12, kLimbs512 = 16;

// Device-side description of one signing batch; B = 4 L bytes per number.
struct WideSignArgs {
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
struct WideKeyArgs {
    const uint8_t* in = nullptr;  // count x B
    uint8_t* priv = nullptr;      // count x B, or nullptr
    uint8_t* pub = nullptr;       // count x 2 B: x || y
    int32_t* status = nullptr;    // count
    uint64_t count = 0;
    uint32_t from_rnd = 0;
    uint32_t le = 0;
};

// One sign and one keys kernel per limb count.  The per-curve constant block
// travels as a kernel argument (scalar loads); `t` is the curve's window
// table in device memory.
void launch_ecdsa_wide_sign(const WideSignArgs& a, const Curve<kLimbs384>& c, const BaseTable<kLimbs384>* t,
                            hipStream_t s);
void launch_ecdsa_wide_sign(const WideSignArgs& a, const Curve<kLimbs512>& c, const BaseTable<kLimbs512>* t,
                            hipStream_t s);
void launch_ecdsa_wide_keys(const WideKeyArgs& a, const Curve<kLimbs384>& c, const BaseTable<kLimbs384>* t,
                            hipStream_t s);
void launch_ecdsa_wide_keys(const WideKeyArgs& a, const Curve<kLimbs512>& c, const BaseTable<kLimbs512>* t,
                            hipStream_t s);

}  // namespace lcbec
