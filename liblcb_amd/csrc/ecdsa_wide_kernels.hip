// ecdsa_wide_kernels.hip — batched ECDSA / GOST R 34.10 signature
// verification on 384- and 512-bit curves for gfx950
// (include/lcb_ecdsa_wide_gpu.h).  One lane verifies one signature with
// verify_one() of ecdsa_math.hpp over the inlined multiply-reduce, one wave
// per workgroup, one kernel per limb count: no cross-lane traffic, no LDS, no
// atomics, no scratch.  A lane whose item is rejected early idles under the
// mask until its wave is done.
#include <hip/hip_runtime.h>

#include "ecdsa_wide_internal.hpp"

namespace lcbec {

constexpr int kWideBlock = 64;
// One wave per SIMD: the lane's live numbers (the point, the three table
// points, two scalars, the operands of a product) pass 256 registers at 16
// limbs, and the register file gives a single wave 512.
constexpr int kWideWavesPerSimd = 1;

template <int L>
__device__ __forceinline__ void wide_verify_item(const EcWideArgs& a, const Curve<L>& c) {
    const uint64_t i = (uint64_t)blockIdx.x * kWideBlock + threadIdx.x;
    if (i >= a.count) return;
    uint64_t k = i;
    if (a.key_idx) {
        k = a.key_idx[i];
        if (k >= a.nkeys) {  // no key is read
            a.status[i] = kEinval;
            return;
        }
    }
    const uint8_t* sig = a.sigs + i * (8 * L);
    const uint8_t* key = a.keys + k * (8 * L);
    a.status[i] = verify_one<L, MulInline>(c, a.hashes + i * a.hash_size, a.hash_size, sig, sig + 4 * L, key,
                                           key + 4 * L, a.le != 0);
}

__global__ __launch_bounds__(kWideBlock, kWideWavesPerSimd) void ecdsa_wide_verify_kernel_384(
    const EcWideArgs a, const Curve<kLimbs384> c) {
    wide_verify_item<kLimbs384>(a, c);
}

__global__ __launch_bounds__(kWideBlock, kWideWavesPerSimd) void ecdsa_wide_verify_kernel_512(
    const EcWideArgs a, const Curve<kLimbs512> c) {
    wide_verify_item<kLimbs512>(a, c);
}

void launch_ecdsa_wide_verify(const EcWideArgs& a, const Curve<kLimbs384>& c, hipStream_t s) {
    if (a.count == 0) return;
    const uint64_t blocks = (a.count + kWideBlock - 1) / kWideBlock;
    hipLaunchKernelGGL(ecdsa_wide_verify_kernel_384, dim3((unsigned)blocks), dim3(kWideBlock), 0, s, a, c);
}

void launch_ecdsa_wide_verify(const EcWideArgs& a, const Curve<kLimbs512>& c, hipStream_t s) {
    if (a.count == 0) return;
    const uint64_t blocks = (a.count + kWideBlock - 1) / kWideBlock;
    hipLaunchKernelGGL(ecdsa_wide_verify_kernel_512, dim3((unsigned)blocks), dim3(kWideBlock), 0, s, a, c);
}

}  // namespace lcbec
