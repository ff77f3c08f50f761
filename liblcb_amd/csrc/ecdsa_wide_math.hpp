// ecdsa_wide_math.hpp — the arithmetic of the batched ECDSA / GOST R 34.10
// verification on 384- and 512-bit curves (include/lcb_ecdsa_wide_gpu.h), in
// plain C++ that compiles for the host as well as for the device.  Numbers,
// moduli, curve blocks, limb helpers, import and curve_setup are those of
// ecdsa_math.hpp at L = 12 and L = 16; what is restated here is everything
// that multiplies: wide_verify_one() is verify_one() formula for formula and
// exceptional case for exceptional case, over another multiply-reduce.
//
// Why another one: ecdsa_math.hpp's mont_mul_raw is one out-of-line body per
// translation unit that takes both operands and the modulus by value, 3 L + 1
// argument registers.  The device calling convention has 32; at L = 12 and
// L = 16 the rest goes to the stack, which is scratch memory, at every call
// of the point loop.  wide_mont_mul has no call boundary: it is inlined at
// every site (72 per kernel), and so that each site stays a loop the
// instruction cache holds, its outer loop over the limbs of b stays rolled.
// A rolled loop cannot index a register array by its counter, so b is rotated
// one limb down per step and the step always reads b.w[0]: L moves beside
// 2 L multiply-adds.  Resources and timings: DESIGN.md 5k.
#pragma once
#include <stdint.h>

#include "ecdsa_math.hpp"

namespace lcbec {

// a b R^-1 mod m for a, b < m: the CIOS steps of mont_mul_raw, one limb of b
// per trip of a rolled loop.
template <int L>
EC_HD EC_INLINE Num<L> wide_mont_mul(const Num<L>& a, Num<L> b, const Mod<L>& M) {
    uint32_t t[L + 1];
    EC_UNROLL
    for (int j = 0; j < L + 1; ++j) t[j] = 0;
    EC_NOUNROLL
    for (int i = 0; i < L; ++i) {
        const uint32_t bi = b.w[0];
        EC_UNROLL
        for (int j = 0; j + 1 < L; ++j) b.w[j] = b.w[j + 1];
        uint64_t c = 0;
        EC_UNROLL
        for (int j = 0; j < L; ++j) {
            c += (uint64_t)a.w[j] * bi + t[j];
            t[j] = (uint32_t)c;
            c >>= 32;
        }
        c += t[L];
        const uint32_t tl = (uint32_t)c, tl1 = (uint32_t)(c >> 32);
        const uint32_t q = t[0] * M.m0inv;
        c = (uint64_t)q * M.m.w[0] + t[0];
        c >>= 32;
        EC_UNROLL
        for (int j = 1; j < L; ++j) {
            c += (uint64_t)q * M.m.w[j] + t[j];
            t[j - 1] = (uint32_t)c;
            c >>= 32;
        }
        c += tl;
        t[L - 1] = (uint32_t)c;
        t[L] = tl1 + (uint32_t)(c >> 32);
    }
    Num<L> r, d;
    EC_UNROLL
    for (int j = 0; j < L; ++j) r.w[j] = t[j];
    const uint32_t br = sub_to(d, r, M.m);
    return select(t[L] != 0 || br == 0, d, r);
}

template <int L>
EC_HD EC_INLINE Num<L> wide_to_mont(const Num<L>& a, const Mod<L>& M) {
    return wide_mont_mul(a, M.rr, M);
}

// x^-1 in Montgomery form (x^(m-2), m prime); 0 for x = 0.
template <int L>
EC_HD EC_INLINE Num<L> wide_mont_inv(const Num<L>& x, const Mod<L>& M) {
    Num<L> r = M.one, e = M.exp;
    EC_NOUNROLL
    for (int i = 0; i < 32 * L; ++i) {
        r = wide_mont_mul(r, r, M);
        if (shl1(e)) r = wide_mont_mul(r, x, M);
    }
    return r;
}

// 2 P, as jac_dbl.
template <int L>
EC_HD EC_INLINE Jac<L> wide_jac_dbl(const Jac<L>& P, const Curve<L>& C) {
    const Mod<L>& F = C.p;
    const Num<L> yy = wide_mont_mul(P.Y, P.Y, F);
    const Num<L> yyyy = wide_mont_mul(yy, yy, F);
    Num<L> s = wide_mont_mul(P.X, yy, F);
    s = mod_add(s, s, F.m);
    s = mod_add(s, s, F.m);  // 4 X Y^2
    Num<L> m;
    if (C.a_kind == kAMinus3) {
        const Num<L> zz = wide_mont_mul(P.Z, P.Z, F);
        m = wide_mont_mul(mod_sub(P.X, zz, F.m), mod_add(P.X, zz, F.m), F);
        m = mod_add(mod_add(m, m, F.m), m, F.m);
    } else {
        const Num<L> xx = wide_mont_mul(P.X, P.X, F);
        m = mod_add(mod_add(xx, xx, F.m), xx, F.m);
        if (C.a_kind != kAZero) {
            const Num<L> zz = wide_mont_mul(P.Z, P.Z, F);
            m = mod_add(m, wide_mont_mul(C.a, wide_mont_mul(zz, zz, F), F), F.m);
        }
    }
    Jac<L> R;
    R.X = mod_sub(wide_mont_mul(m, m, F), mod_add(s, s, F.m), F.m);
    Num<L> y8 = mod_add(yyyy, yyyy, F.m);
    y8 = mod_add(y8, y8, F.m);
    y8 = mod_add(y8, y8, F.m);
    const Num<L> yz = wide_mont_mul(P.Y, P.Z, F);
    R.Y = mod_sub(wide_mont_mul(m, mod_sub(s, R.X, F.m), F), y8, F.m);
    R.Z = mod_add(yz, yz, F.m);
    return R;
}

// P + (x2, y2) for an affine (x2, y2) on the curve, as jac_add_affine: P = O
// gives the affine point, P = (x2, y2) the doubling, P = -(x2, y2) the point
// at infinity.
template <int L>
EC_HD EC_INLINE Jac<L> wide_jac_add_affine(const Jac<L>& P, const Num<L>& x2, const Num<L>& y2, const Curve<L>& C) {
    const Mod<L>& F = C.p;
    Jac<L> R;
    if (is_zero(P.Z)) {
        R.X = x2;
        R.Y = y2;
        R.Z = F.one;
        return R;
    }
    const Num<L> zz = wide_mont_mul(P.Z, P.Z, F);
    const Num<L> u2 = wide_mont_mul(x2, zz, F);
    const Num<L> s2 = wide_mont_mul(y2, wide_mont_mul(P.Z, zz, F), F);
    const Num<L> h = mod_sub(u2, P.X, F.m);
    const Num<L> r = mod_sub(s2, P.Y, F.m);
    if (is_zero(h)) {
        if (is_zero(r)) {
            R.X = x2;
            R.Y = y2;
            R.Z = F.one;
            return wide_jac_dbl(R, C);
        }
        R.X = F.one;
        R.Y = F.one;
        R.Z = small<L>(0);
        return R;
    }
    const Num<L> hh = wide_mont_mul(h, h, F);
    const Num<L> hhh = wide_mont_mul(h, hh, F);
    const Num<L> v = wide_mont_mul(P.X, hh, F);
    R.X = mod_sub(mod_sub(wide_mont_mul(r, r, F), hhh, F.m), mod_add(v, v, F.m), F.m);
    R.Y = mod_sub(wide_mont_mul(r, mod_sub(v, R.X, F.m), F), wide_mont_mul(P.Y, hhh, F), F.m);
    R.Z = wide_mont_mul(P.Z, h, F);
    return R;
}

// What the reference's ecdsa_verify_be / ecdsa_verify_le return for numbers
// of 4 L bytes: verify_one() of ecdsa_math.hpp, line for line.
template <int L>
EC_HD EC_INLINE int wide_verify_one(const Curve<L>& C, const uint8_t* hash, uint32_t hash_size, const uint8_t* sig_r,
                                    const uint8_t* sig_s, const uint8_t* key_x, const uint8_t* key_y, bool le) {
    const Mod<L>& F = C.p;
    const Mod<L>& N = C.n;
    const Num<L> qx = load_num<L>(key_x, 4 * L, le), qy = load_num<L>(key_y, 4 * L, le);
    if (geq(qx, F.m) || geq(qy, F.m)) return kBadPoint;
    const Num<L> x = wide_to_mont(qx, F), y = wide_to_mont(qy, F);
    {
        const Num<L> lhs = wide_mont_mul(y, y, F);
        const Num<L> xxa = mod_add(wide_mont_mul(x, x, F), C.a, F.m);
        const Num<L> rhs = mod_add(wide_mont_mul(xxa, x, F), C.b, F.m);
        if (!equal(lhs, rhs)) return kBadPoint;
    }
    const Num<L> r = load_num<L>(sig_r, 4 * L, le), s = load_num<L>(sig_s, 4 * L, le);
    if (geq(r, N.m) || geq(s, N.m)) return kEinval;
    // bn_mod_reduce: e itself below n, else (e mod (n - 1)) + 1; n > 2^(32 L - 2)
    // (curve_setup), so three subtractions do.
    Num<L> e = load_num<L>(hash, hash_size < 4u * L ? hash_size : 4u * L, le);
    if (geq(e, N.m)) {
        Num<L> nm1, t;
        sub_to(nm1, N.m, small<L>(1));
        e = reduce_small(e, nm1, 3);
        add_to(t, e, small<L>(1));
        e = t;
    }
    Num<L> u1, u2;
    if (C.algo == kAlgoEcdsa) {
        if (is_zero(s)) return kEinval;  // no inverse of 0
        const Num<L> w = wide_mont_inv(wide_to_mont(s, N), N);  // s^-1 R
        u1 = wide_mont_mul(e, w, N);
        u2 = wide_mont_mul(r, w, N);
    } else {
        if (is_zero(e)) e = small<L>(1);
        const Num<L> w = wide_mont_inv(wide_to_mont(e, N), N);  // e^-1 R
        u1 = wide_mont_mul(s, w, N);
        const Num<L> t = wide_mont_mul(r, w, N);
        u2 = mod_sub(small<L>(0), t, N.m);  // -(r e^-1)
    }
    // G + Q in affine form for Shamir's trick over {G, Q, G + Q}; it may be a
    // doubling (Q = G) or the point at infinity (Q = -G).
    Jac<L> R;
    R.X = C.gx;
    R.Y = C.gy;
    R.Z = F.one;
    R = wide_jac_add_affine(R, x, y, C);
    const bool gq_inf = is_zero(R.Z);
    Num<L> gqx, gqy;
    {
        const Num<L> zi = wide_mont_inv(R.Z, F);
        const Num<L> zi2 = wide_mont_mul(zi, zi, F);
        gqx = wide_mont_mul(R.X, zi2, F);
        gqy = wide_mont_mul(R.Y, wide_mont_mul(zi2, zi, F), F);
    }
    R.X = F.one;
    R.Y = F.one;
    R.Z = small<L>(0);
    EC_NOUNROLL
    for (int i = 0; i < 32 * L; ++i) {
        const bool b1 = shl1(u1) != 0, b2 = shl1(u2) != 0;
        R = wide_jac_dbl(R, C);
        if ((b1 || b2) && !(b1 && b2 && gq_inf)) {
            const Num<L> tx = select(b2, select(b1, gqx, x), C.gx);
            const Num<L> ty = select(b2, select(b1, gqy, y), C.gy);
            R = wide_jac_add_affine(R, tx, ty, C);
        }
    }
    if (is_zero(R.Z)) return kBadPoint;
    // R.x mod n = r without inverting Z: X = (r + k n) Z^2 for one k in 0..3
    // with r + k n < p, as in verify_one.
    const Num<L> zz = wide_mont_mul(R.Z, R.Z, F);
    Num<L> t = r;
    bool live = true, ok = false;
    for (int k = 0; k < 4; ++k) {
        if (live && !geq(t, F.m)) ok = ok || equal(wide_mont_mul(wide_to_mont(t, F), zz, F), R.X);
        Num<L> u;
        if (add_to(u, t, N.m)) live = false;  // past 2^(32 L), so past p
        t = u;
    }
    return ok ? 0 : kBadSign;
}

}  // namespace lcbec
