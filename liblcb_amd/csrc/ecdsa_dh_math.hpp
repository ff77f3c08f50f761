// ecdsa_dh_math.hpp — the arithmetic of batched ECDH key agreement
// (include/lcb_ecdsa_dh_gpu.h) on top of ecdsa_math.hpp, in plain C++ for the
// host as well as for the device: one variable-base multiple d Q per item and
// its affine x.
//
//   var_mult()  d Q, binary, most significant bit first: 32 L doublings and
//               32 L mixed additions, the sum kept or dropped with a select.
//   dh_one()    the per-item contract of ecdsa_dh_be / ecdsa_dh_le.
//
// The kernel (ecdsa_dh_kernels.hip) calls dh_one() once per lane; the host
// test (tests/c/ecdsa_dh_host.cpp) calls the same code under the sanitizers.
//
// Secrets: the trip count is fixed and no load address and no branch of
// var_mult() is taken on a bit of d (add-always, select).  NOT constant-time
// beyond that: rejected items return early and jac_add_affine branches on its
// exceptional cases.  For d < n and Q of order n those are reached only as
// R = O while the leading bits of d are zero, and R = -Q in the last step of
// d = n - 1, whose sum is dropped.
#pragma once
#include <stdint.h>

#include "ecdsa_math.hpp"

namespace lcbec {

// d (x, y) for an affine (x, y) on the curve, Montgomery form; the point at
// infinity (Z = 0) for d = 0.
template <int L>
EC_HD EC_INLINE Jac<L> var_mult(const Curve<L>& C, const Num<L>& x, const Num<L>& y, Num<L> d) {
    Jac<L> R;
    R.X = C.p.one;
    R.Y = C.p.one;
    R.Z = small<L>(0);
    EC_NOUNROLL
    for (int i = 0; i < 32 * L; ++i) {
        const bool bit = shl1(d) != 0;
        R = jac_dbl(R, C);
        const Jac<L> T = jac_add_affine(R, x, y, C);  // always; dropped where the bit is 0
        R.X = select(bit, T.X, R.X);
        R.Y = select(bit, T.Y, R.Y);
        R.Z = select(bit, T.Z, R.Z);
    }
    return R;
}

// What the reference's ecdsa_dh_be / ecdsa_dh_le return for numbers of 4 L
// bytes (ecdsa.h:1712-1824), and on 0 the 4 L bytes of the shared x they
// export to `out`; zeros on every other status.  The order of the checks is
// the reference's: the public key (-1), then d >= n (EINVAL), then d = 0 (-1).
// Every supported curve has cofactor 1, so use_cofactor changes nothing and
// is not a parameter.
template <int L>
EC_HD EC_INLINE int dh_one(const Curve<L>& C, const uint8_t* key_x, const uint8_t* key_y, const uint8_t* priv, bool le,
                           uint8_t* out) {
    const Mod<L>& F = C.p;
    store_num<L>(out, small<L>(0), le);
    const Num<L> qx = load_num<L>(key_x, 4 * L, le), qy = load_num<L>(key_y, 4 * L, le);
    if (geq(qx, F.m) || geq(qy, F.m)) return kBadPoint;
    const Num<L> x = to_mont(qx, F), y = to_mont(qy, F);
    {
        const Num<L> lhs = mont_mul(y, y, F);
        const Num<L> xxa = mod_add(mont_mul(x, x, F), C.a, F.m);
        const Num<L> rhs = mod_add(mont_mul(xxa, x, F), C.b, F.m);
        if (!equal(lhs, rhs)) return kBadPoint;
    }
    const Num<L> d = load_num<L>(priv, 4 * L, le);
    if (geq(d, C.n.m)) return kEinval;
    if (is_zero(d)) return kBadPoint;  // d Q = O
    const Jac<L> R = var_mult(C, x, y, d);
    if (is_zero(R.Z)) return kBadPoint;
    Num<L> sx;
    jac_to_affine<L>(R, F, sx, nullptr);
    store_num<L>(out, sx, le);
    return 0;
}

}  // namespace lcbec
