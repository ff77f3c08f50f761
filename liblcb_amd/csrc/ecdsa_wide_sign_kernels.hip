// ecdsa_wide_sign_kernels.hip — batched ECDSA / GOST R 34.10-2012 signing, key
// generation and public keys from private keys on 384- and 512-bit curves for
// gfx950 (include/lcb_ecdsa_wide_sign_gpu.h).  One lane serves one item with
// wide_sign_one() / wide_key_one() of ecdsa_wide_sign_math.hpp, one wave per
// workgroup, one sign and one keys kernel per limb count: no cross-lane
// traffic, no LDS, no atomics.  A lane whose item is rejected idles under the
// mask until its wave is done.
//
// The window table of G is read through addresses that are the same in every
// lane (the window index is the loop counter), all 15 entries of a window, and
// the entry is chosen with selects: no address depends on a secret.
#include <hip/hip_runtime.h>

#include "ecdsa_wide_sign_internal.hpp"
#include "ecdsa_wide_sign_math.hpp"

namespace lcbec {

constexpr int kWideSignBlock = 64;
// One wave per SIMD, as the wide verification: with 256 registers per lane the
// same code spills (DESIGN.md 5l has the figures of the two-wave compile).
constexpr int kWideSignWavesPerSimd = 1;

template <int L>
__device__ __forceinline__ void wide_sign_item(const WideSignArgs& a, const Curve<L>& c, const BaseTable<L>* t) {
    const uint64_t i = (uint64_t)blockIdx.x * kWideSignBlock + threadIdx.x;
    if (i >= a.count) return;
    uint8_t* sig = a.sigs + i * (8 * L);
    Num<L> r = small<L>(0), s = small<L>(0);
    int st = kEinval;
    uint64_t k = i;
    if (a.key_idx) k = a.key_idx[i];
    if (k < a.nkeys)  // else no key is read
        st = wide_sign_one<L>(c, t, a.hashes + i * a.hash_size, a.hash_size, a.priv + k * (4 * L), a.rnd + i * (4 * L),
                              a.le != 0, r, s);
    store_num<L>(sig, r, a.le != 0);
    store_num<L>(sig + 4 * L, s, a.le != 0);
    a.status[i] = st;
}

template <int L>
__device__ __forceinline__ void wide_keys_item(const WideKeyArgs& a, const Curve<L>& c, const BaseTable<L>* t) {
    const uint64_t i = (uint64_t)blockIdx.x * kWideSignBlock + threadIdx.x;
    if (i >= a.count) return;
    Num<L> d, x, y;
    const int st = wide_key_one<L>(c, t, a.in + i * (4 * L), a.from_rnd != 0, a.le != 0, d, x, y);
    if (a.priv) store_num<L>(a.priv + i * (4 * L), d, a.le != 0);
    uint8_t* pub = a.pub + i * (8 * L);
    store_num<L>(pub, x, a.le != 0);
    store_num<L>(pub + 4 * L, y, a.le != 0);
    a.status[i] = st;
}

__global__ __launch_bounds__(kWideSignBlock, kWideSignWavesPerSimd) void ecdsa_wide_sign_kernel_384(
    const WideSignArgs a, const Curve<kLimbs384> c, const BaseTable<kLimbs384>* __restrict__ t) {
    wide_sign_item<kLimbs384>(a, c, t);
}

__global__ __launch_bounds__(kWideSignBlock, kWideSignWavesPerSimd) void ecdsa_wide_sign_kernel_512(
    const WideSignArgs a, const Curve<kLimbs512> c, const BaseTable<kLimbs512>* __restrict__ t) {
    wide_sign_item<kLimbs512>(a, c, t);
}

__global__ __launch_bounds__(kWideSignBlock, kWideSignWavesPerSimd) void ecdsa_wide_keys_kernel_384(
    const WideKeyArgs a, const Curve<kLimbs384> c, const BaseTable<kLimbs384>* __restrict__ t) {
    wide_keys_item<kLimbs384>(a, c, t);
}

__global__ __launch_bounds__(kWideSignBlock, kWideSignWavesPerSimd) void ecdsa_wide_keys_kernel_512(
    const WideKeyArgs a, const Curve<kLimbs512> c, const BaseTable<kLimbs512>* __restrict__ t) {
    wide_keys_item<kLimbs512>(a, c, t);
}

static unsigned wide_sign_blocks(uint64_t count) { return (unsigned)((count + kWideSignBlock - 1) / kWideSignBlock); }

void launch_ecdsa_wide_sign(const WideSignArgs& a, const Curve<kLimbs384>& c, const BaseTable<kLimbs384>* t,
                            hipStream_t s) {
    if (a.count == 0) return;
    hipLaunchKernelGGL(ecdsa_wide_sign_kernel_384, dim3(wide_sign_blocks(a.count)), dim3(kWideSignBlock), 0, s, a, c,
                       t);
}

void launch_ecdsa_wide_sign(const WideSignArgs& a, const Curve<kLimbs512>& c, const BaseTable<kLimbs512>* t,
                            hipStream_t s) {
    if (a.count == 0) return;
    hipLaunchKernelGGL(ecdsa_wide_sign_kernel_512, dim3(wide_sign_blocks(a.count)), dim3(kWideSignBlock), 0, s, a, c,
                       t);
}

void launch_ecdsa_wide_keys(const WideKeyArgs& a, const Curve<kLimbs384>& c, const BaseTable<kLimbs384>* t,
                            hipStream_t s) {
    if (a.count == 0) return;
    hipLaunchKernelGGL(ecdsa_wide_keys_kernel_384, dim3(wide_sign_blocks(a.count)), dim3(kWideSignBlock), 0, s, a, c,
                       t);
}

void launch_ecdsa_wide_keys(const WideKeyArgs& a, const Curve<kLimbs512>& c, const BaseTable<kLimbs512>* t,
                            hipStream_t s) {
    if (a.count == 0) return;
    hipLaunchKernelGGL(ecdsa_wide_keys_kernel_512, dim3(wide_sign_blocks(a.count)), dim3(kWideSignBlock), 0, s, a, c,
                       t);
}

}  // namespace lcbec
