// ecdsa_sign_kernels.hip — batched ECDSA / GOST R 34.10 signing, key
// generation and public keys from private keys for gfx950
// (include/lcb_ecdsa_sign_gpu.h).  One lane serves one item with sign_item() /
// keys_item() of ecdsa_sign_items.hpp, which call sign_one() / key_one() of
// ecdsa_sign_math.hpp: no cross-lane traffic, no LDS, no atomics, no scratch.
// As in the verification kernel the work is v_mad_u64_u32 in a serial chain
// per lane, so one wave per workgroup spreads a small batch over every SIMD; a
// lane whose item is rejected idles under the mask.
//
// The window table of G is read through addresses that are the same in every
// lane (the window index is the loop counter), all 15 entries of a window, and
// the entry is chosen with selects: no address depends on a secret.
#include <hip/hip_runtime.h>

#include "ecdsa_sign_internal.hpp"
#include "ecdsa_sign_items.hpp"

namespace lcbec {

constexpr int kWavesPerSimd = 2;  // as the verification kernel

__global__ __launch_bounds__(kSignBlock, kWavesPerSimd) void ecdsa_sign_kernel(const SignArgs a, const Curve<kLimbs> c,
                                                                               const Table* __restrict__ t) {
    sign_item<kLimbs>(a, c, t);
}

__global__ __launch_bounds__(kSignBlock, kWavesPerSimd) void ecdsa_keys_kernel(const KeyArgs a, const Curve<kLimbs> c,
                                                                               const Table* __restrict__ t) {
    keys_item<kLimbs>(a, c, t);
}

void launch_ecdsa_sign(const SignArgs& a, const Curve<kLimbs>& c, const Table* t, hipStream_t s) {
    if (a.count == 0) return;
    hipLaunchKernelGGL(ecdsa_sign_kernel, dim3(sign_blocks(a.count)), dim3(kSignBlock), 0, s, a, c, t);
}

void launch_ecdsa_keys(const KeyArgs& a, const Curve<kLimbs>& c, const Table* t, hipStream_t s) {
    if (a.count == 0) return;
    hipLaunchKernelGGL(ecdsa_keys_kernel, dim3(sign_blocks(a.count)), dim3(kSignBlock), 0, s, a, c, t);
}

}  // namespace lcbec
