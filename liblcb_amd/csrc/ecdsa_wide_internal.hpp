// ecdsa_wide_internal.hpp — types shared by the kernel TU and the C-ABI TU of
// liblcb_ecdsa_wide_gpu.so (include/lcb_ecdsa_wide_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ecdsa_math.hpp"

namespace lcbec {

constexpr int kLimbs384 = 12, kLimbs512 = 16;

// Device-side description of one verification batch; B = 4 L bytes per number.
struct EcWideArgs {
    const uint8_t* hashes = nullptr;    // count x hash_size
    const uint8_t* sigs = nullptr;      // count x 2 B: r || s
    const uint8_t* keys = nullptr;      // nkeys x 2 B: x || y
    const uint32_t* key_idx = nullptr;  // nullptr: key i for item i
    int32_t* status = nullptr;          // count
    uint64_t count = 0, nkeys = 0;
    uint32_t hash_size = 0;
    uint32_t le = 0;
};

// One kernel per limb count; the per-curve constant block travels as a kernel
// argument (scalar loads).
void launch_ecdsa_wide_verify(const EcWideArgs& a, const Curve<kLimbs384>& c, hipStream_t s);
void launch_ecdsa_wide_verify(const EcWideArgs& a, const Curve<kLimbs512>& c, hipStream_t s);

}  // namespace lcbec
