// ecdsa_wide_sign_math.hpp — the arithmetic of batched ECDSA / GOST R
// 34.10-2012 signing, key generation and public-key recovery on 384- and
// 512-bit curves (include/lcb_ecdsa_wide_sign_gpu.h), in plain C++ for the
// host as well as for the device.  The formulas are those of
// ecdsa_sign_math.hpp (base_mult, sign_one, key_one) and of jac_to_affine,
// restated over the multiply-reduce of ecdsa_wide_math.hpp, which has no call
// boundary: at L = 12 and 16 a call of ecdsa_math.hpp's mont_mul puts its
// operands on the stack.  The window table and its host-side
// derivation (BaseTable<L>, base_table_setup<L>), shr4 and bn_mod_reduce are
// ecdsa_sign_math.hpp's, used as they are.
//
// The kernels (ecdsa_wide_sign_kernels.hip) call these once per lane; the host
// test (tests/c/ecdsa_wide_sign_host.cpp) calls the same code under the
// sanitizers.
//
// Secrets: the rule of ecdsa_sign_math.hpp.  No load address depends on the
// scalar: every window reads all 15 entries through addresses that are the
// same in every lane, copies an entry to a local and picks with selects;
// digit 0 adds an entry and drops the sum with a select.  Trip counts are
// fixed.  NOT constant-time beyond that: rejected items return early and
// wide_jac_add_affine branches on its exceptional cases.
#pragma once
#include <stdint.h>

#include "ecdsa_sign_math.hpp"
#include "ecdsa_wide_math.hpp"

namespace lcbec {

template <int L>
EC_HD EC_INLINE Num<L> wide_from_mont(const Num<L>& a, const Mod<L>& M) {
    return wide_mont_mul(a, small<L>(1), M);
}

// Affine x (and y where wanted) of R, Z != 0, as plain numbers below p: as
// jac_to_affine.
template <int L>
EC_HD EC_INLINE void wide_jac_to_affine(const Jac<L>& R, const Mod<L>& F, Num<L>& x, Num<L>* y) {
    const Num<L> zi = wide_mont_inv(R.Z, F);
    const Num<L> zi2 = wide_mont_mul(zi, zi, F);
    x = wide_from_mont(wide_mont_mul(R.X, zi2, F), F);
    if (y) *y = wide_from_mont(wide_mont_mul(R.Y, wide_mont_mul(zi2, zi, F), F), F);
}

// ------------------------------------------------------ fixed-base multiple
// k G for k < 16^(8 L) over T[j][v - 1] = v 16^j G; the point at infinity
// (Z = 0) for k = 0.  As base_mult: 8 L mixed additions, no doubling.
template <int L>
EC_HD EC_INLINE Jac<L> wide_base_mult(const Curve<L>& C, const BaseTable<L>* T, Num<L> k) {
    Jac<L> R;
    R.X = C.p.one;
    R.Y = C.p.one;
    R.Z = small<L>(0);
    EC_NOUNROLL
    for (int j = 0; j < 8 * L; ++j) {
        const uint32_t v = shr4(k);
        const Aff<L>* row = T->t[j];  // the same address in every lane
        Num<L> tx = row[0].x, ty = row[0].y;
        EC_UNROLL
        for (int e = 1; e < kWinEntries; ++e) {
            // A copy first: select(hit, row[e].x, tx) would read the entry
            // only where hit is true, a load that depends on the digit.
            const Aff<L> ent = row[e];
            const bool hit = v == (uint32_t)(e + 1);
            tx = select(hit, ent.x, tx);
            ty = select(hit, ent.y, ty);
        }
        const Jac<L> S = wide_jac_add_affine(R, tx, ty, C);
        const bool take = v != 0;  // digit 0: the sum is dropped
        R.X = select(take, S.X, R.X);
        R.Y = select(take, S.Y, R.Y);
        R.Z = select(take, S.Z, R.Z);
    }
    return R;
}

// --------------------------------------------------------------------- sign
// What the reference's ecdsa_sign_be / ecdsa_sign_le return for numbers of
// 4 L bytes, and on 0 the r and s they export: sign_one, line for line.  r and
// s are zero on every other status.
template <int L>
EC_HD EC_INLINE int wide_sign_one(const Curve<L>& C, const BaseTable<L>* T, const uint8_t* hash, uint32_t hash_size,
                                  const uint8_t* priv, const uint8_t* rnd, bool le, Num<L>& r, Num<L>& s) {
    const Mod<L>& N = C.n;
    r = small<L>(0);
    s = small<L>(0);
    const Num<L> d = load_num<L>(priv, 4 * L, le);
    if (geq(d, N.m)) return kEinval;  // the key check comes first
    const Num<L> k = bn_mod_reduce(load_num<L>(rnd, 4 * L, le), N.m);
    if (is_zero(k)) return kBadPoint;  // k G = O
    const Jac<L> R = wide_base_mult(C, T, k);
    if (is_zero(R.Z)) return kBadPoint;
    Num<L> x;
    wide_jac_to_affine<L>(R, C.p, x, nullptr);
    const Num<L> rr = reduce_small(x, N.m, 3);  // x < p < 2^(32 L) < 4 n
    if (is_zero(rr)) return kBadPoint;
    Num<L> e = bn_mod_reduce(load_num<L>(hash, hash_size < 4u * L ? hash_size : 4u * L, le), N.m);
    const Num<L> rd = wide_mont_mul(wide_to_mont(rr, N), d, N);  // r d
    Num<L> ss;
    if (C.algo == kAlgoEcdsa) {
        const Num<L> ki = wide_mont_inv(wide_to_mont(k, N), N);  // k^-1 R
        ss = wide_mont_mul(ki, mod_add(e, rd, N.m), N);
    } else {
        e = select(is_zero(e), small<L>(1), e);
        ss = mod_add(wide_mont_mul(wide_to_mont(k, N), e, N), rd, N.m);
    }
    if (is_zero(ss)) return kBadPoint;
    r = rr;
    s = ss;
    return 0;
}

// ------------------------------------------------------------ key generation
// ecdsa_key_gen_be / _le: d = bn_mod_reduce(rnd), Q = d G.  from_rnd = false
// is ecdsa_recover_pub_key_from_priv_key_be / _le: d as given, EINVAL for
// d >= n.  d = 0 is -1 in both (Q = O is no public key).  d, x, y are zero on
// every status but 0.  As key_one.
template <int L>
EC_HD EC_INLINE int wide_key_one(const Curve<L>& C, const BaseTable<L>* T, const uint8_t* in, bool from_rnd, bool le,
                                 Num<L>& d, Num<L>& x, Num<L>& y) {
    const Mod<L>& N = C.n;
    d = small<L>(0);
    x = small<L>(0);
    y = small<L>(0);
    Num<L> v = load_num<L>(in, 4 * L, le);
    if (from_rnd)
        v = bn_mod_reduce(v, N.m);
    else if (geq(v, N.m))
        return kEinval;
    if (is_zero(v)) return kBadPoint;
    const Jac<L> R = wide_base_mult(C, T, v);
    if (is_zero(R.Z)) return kBadPoint;
    wide_jac_to_affine<L>(R, C.p, x, &y);
    d = v;
    return 0;
}

}  // namespace lcbec
