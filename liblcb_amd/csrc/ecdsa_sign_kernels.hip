// ecdsa_sign_kernels.hip — batched ECDSA / GOST R 34.10 signing, key
// generation and public keys from private keys for gfx950
// (include/lcb_ecdsa_sign_gpu.h).  One lane serves one item with sign_one() /
// key_one() of ecdsa_sign_math.hpp: no cross-lane traffic, no LDS, no atomics,
// no scratch.  As in the verification kernel the work is v_mad_u64_u32 in a
// serial chain per lane, so one wave per workgroup spreads a small batch over
// every SIMD; a lane whose item is rejected idles under the mask.
//
// The window table of G is read through addresses that are the same in every
// lane (the window index is the loop counter), all 15 entries of a window, and
// the entry is chosen with selects: no address depends on a secret.
#include <hip/hip_runtime.h>

#include "ecdsa_sign_internal.hpp"

namespace lcbec {

constexpr int kBlock = 64;
constexpr int kWavesPerSimd = 2;  // as the verification kernel

__global__ __launch_bounds__(kBlock, kWavesPerSimd) void ecdsa_sign_kernel(const SignArgs a, const Curve<kLimbs> c,
                                                                           const Table* __restrict__ t) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.count) return;
    uint8_t* sig = a.sigs + i * (2 * kNumBytes);
    Num<kLimbs> r = small<kLimbs>(0), s = small<kLimbs>(0);
    int st = kEinval;
    uint64_t k = i;
    if (a.key_idx) k = a.key_idx[i];
    if (k < a.nkeys)  // else no key is read
        st = sign_one<kLimbs>(c, t, a.hashes + i * a.hash_size, a.hash_size, a.priv + k * kNumBytes,
                              a.rnd + i * kNumBytes, a.le != 0, r, s);
    store_num<kLimbs>(sig, r, a.le != 0);
    store_num<kLimbs>(sig + kNumBytes, s, a.le != 0);
    a.status[i] = st;
}

__global__ __launch_bounds__(kBlock, kWavesPerSimd) void ecdsa_keys_kernel(const KeyArgs a, const Curve<kLimbs> c,
                                                                           const Table* __restrict__ t) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.count) return;
    Num<kLimbs> d, x, y;
    const int st = key_one<kLimbs>(c, t, a.in + i * kNumBytes, a.from_rnd != 0, a.le != 0, d, x, y);
    if (a.priv) store_num<kLimbs>(a.priv + i * kNumBytes, d, a.le != 0);
    uint8_t* pub = a.pub + i * (2 * kNumBytes);
    store_num<kLimbs>(pub, x, a.le != 0);
    store_num<kLimbs>(pub + kNumBytes, y, a.le != 0);
    a.status[i] = st;
}

void launch_ecdsa_sign(const SignArgs& a, const Curve<kLimbs>& c, const Table* t, hipStream_t s) {
    if (a.count == 0) return;
    const uint64_t blocks = (a.count + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(ecdsa_sign_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, a, c, t);
}

void launch_ecdsa_keys(const KeyArgs& a, const Curve<kLimbs>& c, const Table* t, hipStream_t s) {
    if (a.count == 0) return;
    const uint64_t blocks = (a.count + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(ecdsa_keys_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, a, c, t);
}

}  // namespace lcbec
