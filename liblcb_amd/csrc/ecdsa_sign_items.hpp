// ecdsa_sign_items.hpp — what one lane does in the signing and the key
// kernels, at every limb count: included by ecdsa_sign_kernels.hip (8 limbs)
// and ecdsa_wide_sign_kernels.hip (12 and 16), which wrap these bodies in
// their __global__ entry points with their own launch bounds.  Device code
// only.
#pragma once
#include <hip/hip_runtime.h>

#include "ecdsa_sign_args.hpp"
#include "ecdsa_sign_math.hpp"

namespace lcbec {

constexpr int kSignBlock = 64;  // one wave per workgroup

template <int L>
__device__ __forceinline__ void sign_item(const SignArgs& a, const Curve<L>& c, const BaseTable<L>* t) {
    const uint64_t i = (uint64_t)blockIdx.x * kSignBlock + threadIdx.x;
    if (i >= a.count) return;
    uint8_t* sig = a.sigs + i * (8 * L);
    Num<L> r = small<L>(0), s = small<L>(0);
    int st = kEinval;
    uint64_t k = i;
    if (a.key_idx) k = a.key_idx[i];
    if (k < a.nkeys)  // else no key is read
        st = sign_one<L>(c, t, a.hashes + i * a.hash_size, a.hash_size, a.priv + k * (4 * L), a.rnd + i * (4 * L),
                         a.le != 0, r, s);
    store_num<L>(sig, r, a.le != 0);
    store_num<L>(sig + 4 * L, s, a.le != 0);
    a.status[i] = st;
}

template <int L>
__device__ __forceinline__ void keys_item(const KeyArgs& a, const Curve<L>& c, const BaseTable<L>* t) {
    const uint64_t i = (uint64_t)blockIdx.x * kSignBlock + threadIdx.x;
    if (i >= a.count) return;
    Num<L> d, x, y;
    const int st = key_one<L>(c, t, a.in + i * (4 * L), a.from_rnd != 0, a.le != 0, d, x, y);
    if (a.priv) store_num<L>(a.priv + i * (4 * L), d, a.le != 0);
    uint8_t* pub = a.pub + i * (8 * L);
    store_num<L>(pub, x, a.le != 0);
    store_num<L>(pub + 4 * L, y, a.le != 0);
    a.status[i] = st;
}

inline unsigned sign_blocks(uint64_t count) { return (unsigned)((count + kSignBlock - 1) / kSignBlock); }

}  // namespace lcbec
