// ecdsa_wide_sign_kernels.hip — batched ECDSA / GOST R 34.10-2012 signing, key
// generation and public keys from private keys on 384- and 512-bit curves for
// gfx950 (include/lcb_ecdsa_wide_sign_gpu.h).  One lane serves one item with
// sign_item() / keys_item() of ecdsa_sign_items.hpp, the bodies of the 256-bit
// kernels at 12 and 16 limbs, one wave per workgroup, one sign and one keys
// kernel per limb count: no cross-lane traffic, no LDS, no atomics.  A lane
// whose item is rejected idles under the mask until its wave is done.
//
// The window table of G is read through addresses that are the same in every
// lane (the window index is the loop counter), all 15 entries of a window, and
// the entry is chosen with selects: no address depends on a secret.
#include <hip/hip_runtime.h>

#include "ecdsa_sign_items.hpp"
#include "ecdsa_wide_sign_internal.hpp"

namespace lcbec {

// One wave per SIMD, as the wide verification: with 256 registers per lane the
// same code spills (DESIGN.md 5l has the figures of the two-wave compile).
constexpr int kWideSignWavesPerSimd = 1;

__global__ __launch_bounds__(kSignBlock, kWideSignWavesPerSimd) void ecdsa_wide_sign_kernel_384(
    const SignArgs a, const Curve<kLimbs384> c, const BaseTable<kLimbs384>* __restrict__ t) {
    sign_item<kLimbs384>(a, c, t);
}

__global__ __launch_bounds__(kSignBlock, kWideSignWavesPerSimd) void ecdsa_wide_sign_kernel_512(
    const SignArgs a, const Curve<kLimbs512> c, const BaseTable<kLimbs512>* __restrict__ t) {
    sign_item<kLimbs512>(a, c, t);
}

__global__ __launch_bounds__(kSignBlock, kWideSignWavesPerSimd) void ecdsa_wide_keys_kernel_384(
    const KeyArgs a, const Curve<kLimbs384> c, const BaseTable<kLimbs384>* __restrict__ t) {
    keys_item<kLimbs384>(a, c, t);
}

__global__ __launch_bounds__(kSignBlock, kWideSignWavesPerSimd) void ecdsa_wide_keys_kernel_512(
    const KeyArgs a, const Curve<kLimbs512> c, const BaseTable<kLimbs512>* __restrict__ t) {
    keys_item<kLimbs512>(a, c, t);
}

void launch_ecdsa_wide_sign(const SignArgs& a, const Curve<kLimbs384>& c, const BaseTable<kLimbs384>* t,
                            hipStream_t s) {
    if (a.count == 0) return;
    hipLaunchKernelGGL(ecdsa_wide_sign_kernel_384, dim3(sign_blocks(a.count)), dim3(kSignBlock), 0, s, a, c, t);
}

void launch_ecdsa_wide_sign(const SignArgs& a, const Curve<kLimbs512>& c, const BaseTable<kLimbs512>* t,
                            hipStream_t s) {
    if (a.count == 0) return;
    hipLaunchKernelGGL(ecdsa_wide_sign_kernel_512, dim3(sign_blocks(a.count)), dim3(kSignBlock), 0, s, a, c, t);
}

void launch_ecdsa_wide_keys(const KeyArgs& a, const Curve<kLimbs384>& c, const BaseTable<kLimbs384>* t,
                            hipStream_t s) {
    if (a.count == 0) return;
    hipLaunchKernelGGL(ecdsa_wide_keys_kernel_384, dim3(sign_blocks(a.count)), dim3(kSignBlock), 0, s, a, c, t);
}

void launch_ecdsa_wide_keys(const KeyArgs& a, const Curve<kLimbs512>& c, const BaseTable<kLimbs512>* t,
                            hipStream_t s) {
    if (a.count == 0) return;
    hipLaunchKernelGGL(ecdsa_wide_keys_kernel_512, dim3(sign_blocks(a.count)), dim3(kSignBlock), 0, s, a, c, t);
}

}  // namespace lcbec
