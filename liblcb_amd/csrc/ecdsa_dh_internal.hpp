// ecdsa_dh_internal.hpp — types shared by the kernel TU and the C-ABI TU of
// liblcb_ecdsa_dh_gpu.so (include/lcb_ecdsa_dh_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ecdsa_dh_math.hpp"

namespace lcbec {

// Device-side description of one key agreement batch.
struct DhArgs {
    const uint8_t* pub = nullptr;        // npub x 2 kNumBytes: x || y
    const uint32_t* pub_idx = nullptr;   // nullptr: public key i for item i
    const uint8_t* priv = nullptr;       // npriv x kNumBytes
    const uint32_t* priv_idx = nullptr;  // nullptr: private key i for item i
    uint8_t* shared = nullptr;           // count x kNumBytes
    int32_t* status = nullptr;           // count
    uint64_t count = 0, npub = 0, npriv = 0;
    uint32_t le = 0;
};

// The per-curve constant block travels as a kernel argument (scalar loads).
void launch_ecdsa_dh(const DhArgs& a, const Curve<kLimbs>& c, hipStream_t s);

}  // namespace lcbec
