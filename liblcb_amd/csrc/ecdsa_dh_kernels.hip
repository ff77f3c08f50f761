// ecdsa_dh_kernels.hip — batched ECDH key agreement for gfx950
// (include/lcb_ecdsa_dh_gpu.h).  One lane serves one item with dh_one() of
// ecdsa_dh_math.hpp: no cross-lane traffic, no LDS, no atomics, no scratch.
// As in the verification kernel the work is v_mad_u64_u32 in a serial chain
// per lane, so one wave per workgroup spreads a small batch over every SIMD;
// a lane whose item is rejected idles under the mask.
//
// Both indices are checked before anything else: an item whose index is past
// its table reads no key and gets EINVAL and zeros.
#include <hip/hip_runtime.h>

#include "ecdsa_dh_internal.hpp"

namespace lcbec {

constexpr int kBlock = 64;
constexpr int kWavesPerSimd = 2;  // as the verification kernel

__global__ __launch_bounds__(kBlock, kWavesPerSimd) void ecdsa_dh_kernel(const DhArgs a, const Curve<kLimbs> c) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.count) return;
    uint8_t* out = a.shared + i * kNumBytes;
    uint64_t kq = i, kd = i;
    if (a.pub_idx) kq = a.pub_idx[i];
    if (a.priv_idx) kd = a.priv_idx[i];
    int st = kEinval;
    if (kq < a.npub && kd < a.npriv) {  // else no key is read
        const uint8_t* q = a.pub + kq * (2 * kNumBytes);
        st = dh_one<kLimbs>(c, q, q + kNumBytes, a.priv + kd * kNumBytes, a.le != 0, out);
    } else {
        store_num<kLimbs>(out, small<kLimbs>(0), false);
    }
    a.status[i] = st;
}

void launch_ecdsa_dh(const DhArgs& a, const Curve<kLimbs>& c, hipStream_t s) {
    if (a.count == 0) return;
    const uint64_t blocks = (a.count + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(ecdsa_dh_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, a, c);
}

}  // namespace lcbec
