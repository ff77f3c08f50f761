// ecdsa_kernels.hip — batched ECDSA / GOST R 34.10 signature verification
// for gfx950 (include/lcb_ecdsa_gpu.h).  One lane verifies one signature
// with verify_one() of ecdsa_math.hpp: no cross-lane traffic, no LDS, no
// atomics, no scratch.  The work is integer multiply-add (v_mad_u64_u32) in
// a serial dependency chain per lane, so throughput comes from waves per
// SIMD; one wave per workgroup lets the dispatcher spread a small batch over
// every SIMD.  A lane whose item is rejected early idles under the mask
// until its wave is done.
#include <hip/hip_runtime.h>

#include "ecdsa_internal.hpp"

namespace lcbec {

constexpr int kBlock = 64;
// 187 VGPRs without a spill; asking for three waves per SIMD (168 registers)
// spills to scratch memory, and two waves already fill the multiplier
// (DESIGN.md 5g).
constexpr int kWavesPerSimd = 2;

__global__ __launch_bounds__(kBlock, kWavesPerSimd) void ecdsa_verify_kernel(const EcArgs a, const Curve<kLimbs> c) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.count) return;
    uint64_t k = i;
    if (a.key_idx) {
        k = a.key_idx[i];
        if (k >= a.nkeys) {  // no key is read
            a.status[i] = kEinval;
            return;
        }
    }
    const uint8_t* sig = a.sigs + i * (2 * kNumBytes);
    const uint8_t* key = a.keys + k * (2 * kNumBytes);
    a.status[i] = verify_one<kLimbs>(c, a.hashes + i * a.hash_size, a.hash_size, sig, sig + kNumBytes, key,
                                     key + kNumBytes, a.le != 0);
}

void launch_ecdsa_verify(const EcArgs& a, const Curve<kLimbs>& c, hipStream_t s) {
    if (a.count == 0) return;
    const uint64_t blocks = (a.count + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(ecdsa_verify_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, a, c);
}

}  // namespace lcbec
