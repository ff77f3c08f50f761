// ecdsa_sign_math.hpp — the arithmetic of batched ECDSA / GOST R 34.10
// signing, key generation and public-key recovery
// (include/lcb_ecdsa_sign_gpu.h) on top of ecdsa_math.hpp, in plain C++ for
// the host as well as for the device.  All three are a secret scalar times
// the base point G and a little arithmetic mod n:
//
//   base_mult()   k G over a 4-bit window table of G, T[j][v - 1] = v 16^j G
//                 (j = 0 .. 8 L - 1, v = 1 .. 15, affine, Montgomery form):
//                 8 L mixed additions, no doubling.
//   sign_one(), keygen_one(), pubkey_one()   the per-item contracts.
//
// The kernels (ecdsa_sign_kernels.hip at 8 limbs, ecdsa_wide_sign_kernels.hip
// at 12 and 16, through ecdsa_sign_items.hpp) call these once per lane; the
// host tests (tests/c/ecdsa_sign_host.cpp, tests/c/ecdsa_wide_sign_host.cpp)
// call the same code under the sanitizers, and the host build derives the
// table (base_table_setup).  K is the multiply-reduce policy of
// ecdsa_math.hpp.
//
// Secrets: no load address depends on the scalar.  Every window reads all 15
// entries through addresses that are the same in every lane and picks one with
// selects; digit 0 adds an entry and drops the sum with a select.  Trip counts
// are fixed.  NOT constant-time beyond that: rejected items return early and
// jac_add_affine branches on its exceptional cases.
#pragma once
#include <stdint.h>

#include "ecdsa_math.hpp"

namespace lcbec {

constexpr int kWinBits = 4;
constexpr int kWinEntries = (1 << kWinBits) - 1;  // v = 1 .. 15

template <int L>
struct Aff {  // affine, Montgomery form
    Num<L> x, y;
};

// 8 L windows x 15 entries (L = 8: 960 points, 60 KiB; 135 KiB at 12 limbs,
// 240 KiB at 16).
template <int L>
struct BaseTable {
    Aff<L> t[8 * L][kWinEntries];
};

// ------------------------------------------------------------- small helpers
// Shifts a right by four bits and returns the four bits that fell out.
template <int L>
EC_HD EC_INLINE uint32_t shr4(Num<L>& a) {
    const uint32_t low = a.w[0] & 15u;
    EC_UNROLL
    for (int j = 0; j < L - 1; ++j) a.w[j] = (a.w[j] >> 4) | (a.w[j + 1] << 28);
    a.w[L - 1] >>= 4;
    return low;
}

// The reference's bn_mod_reduce: v itself below m, else (v mod (m - 1)) + 1.
// m > 2^(32 L - 2) (curve_setup), so three subtractions of m - 1 do.  No
// branch on v.
template <int L>
EC_HD EC_INLINE Num<L> bn_mod_reduce(const Num<L>& v, const Num<L>& m) {
    Num<L> m1, t;
    sub_to(m1, m, small<L>(1));
    add_to(t, reduce_small(v, m1, 3), small<L>(1));
    return select(geq(v, m), t, v);
}

// ------------------------------------------------------ fixed-base multiple
// k G for k < 16^(8 L); the point at infinity (Z = 0) for k = 0.
template <int L, class K = DefaultMul<L>>
EC_HD EC_INLINE Jac<L> base_mult(const Curve<L>& C, const BaseTable<L>* T, Num<L> k) {
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
        const Jac<L> S = jac_add_affine<L, K>(R, tx, ty, C);
        const bool take = v != 0;  // digit 0: the sum is dropped
        R.X = select(take, S.X, R.X);
        R.Y = select(take, S.Y, R.Y);
        R.Z = select(take, S.Z, R.Z);
    }
    return R;
}

// --------------------------------------------------------------------- sign
// What the reference's ecdsa_sign_be / ecdsa_sign_le return for numbers of
// 4 L bytes (ecdsa.h:1192-1351), and on 0 the r and s they export.  r and s
// are zero on every other status.
template <int L, class K = DefaultMul<L>>
EC_HD EC_INLINE int sign_one(const Curve<L>& C, const BaseTable<L>* T, const uint8_t* hash, uint32_t hash_size,
                             const uint8_t* priv, const uint8_t* rnd, bool le, Num<L>& r, Num<L>& s) {
    const Mod<L>& N = C.n;
    r = small<L>(0);
    s = small<L>(0);
    const Num<L> d = load_num<L>(priv, 4 * L, le);
    if (geq(d, N.m)) return kEinval;  // the key check comes first
    const Num<L> k = bn_mod_reduce(load_num<L>(rnd, 4 * L, le), N.m);
    if (is_zero(k)) return kBadPoint;  // k G = O
    const Jac<L> R = base_mult<L, K>(C, T, k);
    if (is_zero(R.Z)) return kBadPoint;
    Num<L> x;
    jac_to_affine<L, K>(R, C.p, x, nullptr);
    const Num<L> rr = reduce_small(x, N.m, 3);  // x < p < 2^(32 L) < 4 n
    if (is_zero(rr)) return kBadPoint;
    Num<L> e = bn_mod_reduce(load_num<L>(hash, hash_size < 4u * L ? hash_size : 4u * L, le), N.m);
    const Num<L> rd = K::mul(to_mont<L, K>(rr, N), d, N);  // r d
    Num<L> ss;
    if (C.algo == kAlgoEcdsa) {
        const Num<L> ki = mont_inv<L, K>(to_mont<L, K>(k, N), N);  // k^-1 R
        ss = K::mul(ki, mod_add(e, rd, N.m), N);
    } else {
        e = select(is_zero(e), small<L>(1), e);
        ss = mod_add(K::mul(to_mont<L, K>(k, N), e, N), rd, N.m);
    }
    if (is_zero(ss)) return kBadPoint;
    r = rr;
    s = ss;
    return 0;
}

// ------------------------------------------------------------ key generation
// ecdsa_key_gen_be / _le (ecdsa.h:1083-1177): d = bn_mod_reduce(rnd), Q = d G.
// from_rnd = false is ecdsa_recover_pub_key_from_priv_key_be / _le
// (ecdsa.h:1839-1905): d as given, EINVAL for d >= n.  d = 0 is -1 in both
// (Q = O is no public key).  d, x, y are zero on every status but 0.
template <int L, class K = DefaultMul<L>>
EC_HD EC_INLINE int key_one(const Curve<L>& C, const BaseTable<L>* T, const uint8_t* in, bool from_rnd, bool le,
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
    const Jac<L> R = base_mult<L, K>(C, T, v);
    if (is_zero(R.Z)) return kBadPoint;
    jac_to_affine<L, K>(R, C.p, x, &y);
    d = v;
    return 0;
}

template <int L, class K = DefaultMul<L>>
EC_HD EC_INLINE int keygen_one(const Curve<L>& C, const BaseTable<L>* T, const uint8_t* rnd, bool le, Num<L>& d,
                               Num<L>& x, Num<L>& y) {
    return key_one<L, K>(C, T, rnd, true, le, d, x, y);
}

template <int L, class K = DefaultMul<L>>
EC_HD EC_INLINE int pubkey_one(const Curve<L>& C, const BaseTable<L>* T, const uint8_t* priv, bool le, Num<L>& x,
                               Num<L>& y) {
    Num<L> d;
    return key_one<L, K>(C, T, priv, false, le, d, x, y);
}

// ------------------------------------------------------- the table (host side)
// P + Q for two Jacobian points, every exceptional case included.
template <int L>
inline Jac<L> jac_add(const Jac<L>& P, const Jac<L>& Q, const Curve<L>& C) {
    const Mod<L>& F = C.p;
    if (is_zero(P.Z)) return Q;
    if (is_zero(Q.Z)) return P;
    const Num<L> z1z1 = mont_mul(P.Z, P.Z, F), z2z2 = mont_mul(Q.Z, Q.Z, F);
    const Num<L> u1 = mont_mul(P.X, z2z2, F), u2 = mont_mul(Q.X, z1z1, F);
    const Num<L> s1 = mont_mul(P.Y, mont_mul(Q.Z, z2z2, F), F), s2 = mont_mul(Q.Y, mont_mul(P.Z, z1z1, F), F);
    const Num<L> h = mod_sub(u2, u1, F.m), r = mod_sub(s2, s1, F.m);
    Jac<L> R;
    if (is_zero(h)) {
        if (is_zero(r)) return jac_dbl(P, C);
        R.X = F.one;
        R.Y = F.one;
        R.Z = small<L>(0);
        return R;
    }
    const Num<L> hh = mont_mul(h, h, F), hhh = mont_mul(h, hh, F), v = mont_mul(u1, hh, F);
    R.X = mod_sub(mod_sub(mont_mul(r, r, F), hhh, F.m), mod_add(v, v, F.m), F.m);
    R.Y = mod_sub(mont_mul(r, mod_sub(v, R.X, F.m), F), mont_mul(s1, hhh, F), F.m);
    R.Z = mont_mul(mont_mul(P.Z, Q.Z, F), h, F);
    return R;
}

// Derives T from G: 960 Jacobian points by doublings and additions, then one
// field inversion for all of them (Montgomery's simultaneous inversion).
// `work` holds 8 L * 15 Jacobian points and as many numbers.  False if an
// entry came out as the point at infinity (n would divide v 16^j).
template <int L>
inline bool base_table_setup(BaseTable<L>& T, const Curve<L>& C, Jac<L>* pts, Num<L>* pre) {
    const Mod<L>& F = C.p;
    const int W = 8 * L, E = kWinEntries;
    Jac<L> B;
    B.X = C.gx;
    B.Y = C.gy;
    B.Z = F.one;
    for (int j = 0; j < W; ++j) {
        pts[j * E] = B;
        pts[j * E + 1] = jac_dbl(B, C);
        for (int e = 2; e < E; ++e) pts[j * E + e] = jac_add(pts[j * E + e - 1], B, C);
        B = jac_dbl(pts[j * E + E - 1 - 7], C);  // 16 B = 2 (8 B)
    }
    // pre[i] = Z_0 ... Z_i; one inverse; walk back.
    Num<L> acc = F.one;
    for (int i = 0; i < W * E; ++i) {
        if (is_zero(pts[i].Z)) return false;
        acc = mont_mul(acc, pts[i].Z, F);
        pre[i] = acc;
    }
    Num<L> inv = mont_inv(acc, F);
    for (int i = W * E - 1; i >= 0; --i) {
        const Num<L> zi = i ? mont_mul(inv, pre[i - 1], F) : inv;
        inv = mont_mul(inv, pts[i].Z, F);
        const Num<L> zi2 = mont_mul(zi, zi, F);
        Aff<L>& a = T.t[i / E][i % E];
        a.x = mont_mul(pts[i].X, zi2, F);
        a.y = mont_mul(pts[i].Y, mont_mul(zi2, zi, F), F);
    }
    return true;
}

}  // namespace lcbec
