// ecdsa_key_math.hpp — the arithmetic of batched public-key import and export
// (include/lcb_ecdsa_key_gpu.h) on top of ecdsa_math.hpp, in plain C++ for the
// host as well as for the device.
//
//   key_setup()       per-curve constants of the square root, host side, once
//   mont_sqrt()       a square root candidate mod p, fixed trip counts
//   key_import_one()  the per-item contract of ecdsa_pub_key_import_be / _le
//   key_export_one()  the per-item contract of ecdsa_pub_key_export_be / _le
//
// The kernels (ecdsa_key_kernels.hip) call the last two once per lane; the
// host test (tests/c/ecdsa_key_host.cpp) calls the same code under the
// sanitizers.
//
// The square root.  p - 1 = 2^s q with q odd.  w = v^((q - 1) / 2) gives the
// candidate r = v w = v^((q + 1) / 2) and t = r w = v^q with r^2 = v t.  Where
// s = 1 (p = 3 mod 4: eight of the ten curves) r = v^((p + 1) / 4) and that is
// all.  Where s > 1 (the two curves with p = 1 mod 8, s = 4 and s = 3)
// Tonelli-Shanks runs its s - 1 correction steps, every one of them always:
// with c of order 2^i and t^(2^(i - 1)) = 1, u = t^(2^(i - 2)) is 1 or -1, and
// where it is -1 r takes a factor c and t a factor c^2, kept or dropped with a
// select.  The exponent and s are the same in every lane, so no branch of the
// root diverges.  For a non-residue (or anything else) the candidate is not a
// root; the caller's r^2 = v check is the only test of that, and it also
// serves v = 0.
#pragma once
#include <stdint.h>

#include "ecdsa_math.hpp"

namespace lcbec {

constexpr int kKeyMaxSize = 2 * kNumBytes + 1;  // the packed form

// Per-curve constants of the square root mod p (key_setup).
template <int L>
struct KeyConsts {
    Num<L> exp;   // (q - 1) / 2
    Num<L> c;     // z^q in Montgomery form, z the smallest non-residue: order 2^s
    uint32_t s;   // p - 1 = 2^s q, q odd
};

// x^e in Montgomery form, all 32 L bits of e, most significant first.  The
// exponent is the same in every lane, so its branch does not diverge.
template <int L>
EC_HD EC_INLINE Num<L> mont_pow(const Num<L>& x, Num<L> e, const Mod<L>& M) {
    Num<L> r = M.one;
    EC_NOUNROLL
    for (int i = 0; i < 32 * L; ++i) {
        r = mont_mul(r, r, M);
        if (shl1(e)) r = mont_mul(r, x, M);
    }
    return r;
}

// a >> 1.
template <int L>
EC_HD EC_INLINE void shr1(Num<L>& a) {
    EC_UNROLL
    for (int j = 0; j < L - 1; ++j) a.w[j] = (a.w[j] >> 1) | (a.w[j + 1] << 31);
    a.w[L - 1] >>= 1;
}

// Host side, once per curve.  False where no non-residue below 256 exists
// (never, for a prime p).
template <int L>
EC_HD inline bool key_setup(KeyConsts<L>& K, const Curve<L>& C) {
    const Mod<L>& F = C.p;
    Num<L> q, half;
    sub_to(q, F.m, small<L>(1));
    half = q;
    shr1(half);  // (p - 1) / 2, Euler's exponent
    K.s = 0;
    while (!(q.w[0] & 1u)) {
        shr1(q);
        ++K.s;
    }
    K.exp = q;
    shr1(K.exp);  // (q - 1) / 2
    Num<L> minus_one = mod_sub(small<L>(0), F.one, F.m);
    for (uint32_t z = 2; z < 256; ++z) {
        const Num<L> zm = to_mont(small<L>(z), F);
        if (!equal(mont_pow(zm, half, F), minus_one)) continue;
        K.c = mont_pow(zm, q, F);
        return true;
    }
    return false;
}

// A square root candidate of v (Montgomery form in, Montgomery form out): a
// root where v is a square, anything otherwise.
template <int L>
EC_HD EC_INLINE Num<L> mont_sqrt(const Num<L>& v, const KeyConsts<L>& K, const Mod<L>& F) {
    const Num<L> w = mont_pow(v, K.exp, F);
    Num<L> r = mont_mul(v, w, F);
    if (K.s > 1) {  // the same in every lane
        Num<L> t = mont_mul(r, w, F), c = K.c;
        EC_NOUNROLL
        for (uint32_t i = K.s; i > 1; --i) {
            Num<L> u = t;
            EC_NOUNROLL
            for (uint32_t j = 0; j + 2 < i; ++j) u = mont_mul(u, u, F);
            const bool fix = !equal(u, F.one);
            const Num<L> rc = mont_mul(r, c, F);
            c = mont_mul(c, c, F);
            const Num<L> tc = mont_mul(t, c, F);
            r = select(fix, rc, r);
            t = select(fix, tc, t);
        }
    }
    return r;
}

// x^3 + a x + b in Montgomery form; a = -3 and a = 0 are scalar branches
// (a_kind is the same in every lane).
template <int L>
EC_HD EC_INLINE Num<L> curve_rhs(const Curve<L>& C, const Num<L>& x) {
    const Mod<L>& F = C.p;
    Num<L> t = mont_mul(x, x, F);
    if (C.a_kind == kAMinus3) {
        t = mod_sub(t, mod_add(mod_add(F.one, F.one, F.m), F.one, F.m), F.m);
    } else if (C.a_kind != kAZero) {
        t = mod_add(t, C.a, F.m);
    }
    return mod_add(mont_mul(t, x, F), C.b, F.m);
}

// The coordinates of one key as plain numbers below p.  Returns the status of
// ecdsa_pub_key_import_be / _le (ecdsa.h:939-1071) for numbers of 4 L bytes;
// *inf is set where the key is the point at infinity (status 0, x and y
// untouched).  key_y counts only where size = 4 L.  No byte outside
// key[0 .. size) and key_y[0 .. 4 L) is read.
template <int L>
EC_HD EC_INLINE int key_parse(const Curve<L>& C, const KeyConsts<L>& K, const uint8_t* key, uint32_t size,
                              const uint8_t* key_y, bool le, Num<L>& x, Num<L>& y, bool& inf) {
    constexpr uint32_t B = 4 * L;
    const Mod<L>& F = C.p;
    inf = false;
    if (size == 0) return kEinval;
    if (size == 1) {
        if (key[0] != 0) return kEinval;
        inf = true;
        return 0;
    }
    const uint8_t *xp = key, *yp = key_y;
    bool compressed = false;
    if (size == B) {
        if (!key_y) return kEinval;
    } else if (size == B + 1) {
        if (key[0] != 2 && key[0] != 3) return kBadPoint;
        compressed = true;
        xp = key + 1;
    } else if (size == 2 * B + 1) {
        if (key[0] != 4 && key[0] != 6 && key[0] != 7) return kBadPoint;  // 6 / 7: the parity is not compared
        xp = key + 1;
        yp = key + 1 + B;
    } else if (size == 2 * B) {
        yp = key + B;
    } else {
        return kBadPoint;
    }
    x = load_num<L>(xp, B, le);
    if (geq(x, F.m)) return kBadPoint;
    const Num<L> xm = to_mont(x, F);
    const Num<L> rhs = curve_rhs(C, xm);
    if (compressed) {
        const Num<L> r = mont_sqrt(rhs, K, F);
        if (!equal(mont_mul(r, r, F), rhs)) return kBadPoint;  // no root
        const Num<L> yr = from_mont(r, F);
        const bool flip = (yr.w[0] & 1u) != (uint32_t)(key[0] & 1u);
        y = select(flip, mod_sub(small<L>(0), yr, F.m), yr);
        return 0;
    }
    y = load_num<L>(yp, B, le);
    if (geq(y, F.m)) return kBadPoint;
    const Num<L> ym = to_mont(y, F);
    if (!equal(mont_mul(ym, ym, F), rhs)) return kBadPoint;
    return 0;
}

// One item of the import: the status, and at out the 2 x 4 L bytes x || y in
// the form's byte order on 0, zeros on every other status and for the point
// at infinity; *infinity (where given) 1 for the point at infinity, else 0.
template <int L>
EC_HD EC_INLINE int key_import_one(const Curve<L>& C, const KeyConsts<L>& K, const uint8_t* key, uint32_t size,
                                   const uint8_t* key_y, bool le, uint8_t* out, uint8_t* infinity) {
    Num<L> x = small<L>(0), y = small<L>(0);
    bool inf = false;
    const int st = key_parse(C, K, key, size, key_y, le, x, y, inf);
    const bool ok = st == 0 && !inf;
    store_num<L>(out, select(ok, x, small<L>(0)), le);
    store_num<L>(out + 4 * L, select(ok, y, small<L>(0)), le);
    if (infinity) *infinity = inf ? 1 : 0;
    return st;
}

// One item of the export (ecdsa.h:837-924; nothing is validated): pub is
// x || y, 2 x 4 L bytes in the form's byte order.  Writes the key form at out
// and returns its size: 1 (a zero byte) for the point at infinity, 4 L + 1
// compressed, 8 L + 1 packed.  No byte past that size is written.
template <int L>
EC_HD EC_INLINE uint32_t key_export_one(const uint8_t* pub, bool inf, bool compress, bool le, uint8_t* out) {
    constexpr uint32_t B = 4 * L;
    if (inf) {
        out[0] = 0;
        return 1;
    }
    const uint32_t n = compress ? B : 2 * B;
    out[0] = compress ? (uint8_t)(2u | (pub[le ? B : 2 * B - 1] & 1u)) : (uint8_t)4;
    for (uint32_t k = 0; k < n; ++k) out[1 + k] = pub[k];
    return n + 1;
}

}  // namespace lcbec
