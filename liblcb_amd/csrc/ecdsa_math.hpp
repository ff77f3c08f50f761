// ecdsa_math.hpp — the arithmetic of the batched ECDSA / GOST R 34.10
// verification (include/lcb_ecdsa_gpu.h), in plain C++ that compiles for the
// host as well as for the device: numbers of L 32-bit limbs, Montgomery
// multiplication over an odd modulus (serves the field p and the group order
// n alike), Fermat inversion, Jacobian point arithmetic with every
// exceptional case, and verify_one(), the whole per-item contract.  The
// kernels (ecdsa_kernels.hip at 8 limbs, ecdsa_wide_kernels.hip at 12 and 16)
// call verify_one() once per lane; the host tests
// (tests/c/ecdsa_verify_host.cpp, tests/c/ecdsa_wide_host.cpp) call the same
// code under the sanitizers.
//
// There is one set of formulas and two multiply-reduces under it.  Everything
// that multiplies is a template over <L, K>, K a policy type with one static
// mul(a, b, M): MulCall is the out-of-line body (mont_mul), MulInline the
// rolled, inlined one (mont_mul_rolled).  DefaultMul<L> picks by limb count,
// and a call that names no policy gets it.
//
// Every array here is indexed with compile-time constants once the limb
// loops are unrolled: scalar bits are read by shifting the scalar, table
// entries are chosen with selects, so nothing lands in scratch memory.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EC_HD __host__ __device__
#define EC_UNROLL _Pragma("unroll")
#define EC_NOUNROLL _Pragma("nounroll")
#else
#define EC_HD
#define EC_UNROLL
#define EC_NOUNROLL
#endif
// One body of the 8 x 8 limb multiply-reduce per translation unit: inlining
// it at every call site multiplies the compile time (host and device) and
// overflows the instruction cache of the point loop.
#define EC_NOINLINE __attribute__((noinline))
#define EC_INLINE inline __attribute__((always_inline))

namespace lcbec {

constexpr int kEinval = 22;  // EINVAL of the reference's platforms
constexpr int kBadPoint = -1;
constexpr int kBadSign = -2;
constexpr int kLimbs = 8;  // 256-bit curves; a 384-bit build is kLimbs = 12
constexpr int kNumBytes = 4 * kLimbs;
enum { kAlgoEcdsa = 0, kAlgoGost = 1 };
enum { kAGeneral = 0, kAZero = 1, kAMinus3 = 2 };  // Curve::a_kind

// A number of L limbs, least significant first.
template <int L>
struct Num {
    uint32_t w[L];
};

// An odd modulus with its Montgomery constants (R = 2^(32 L)).
template <int L>
struct Mod {
    Num<L> m;
    Num<L> one;      // R mod m
    Num<L> rr;       // R^2 mod m
    Num<L> exp;      // m - 2, the Fermat exponent
    uint32_t m0inv;  // -m^-1 mod 2^32
};

// Per-curve constant block; a, b, gx, gy in Montgomery form mod p.
template <int L>
struct Curve {
    Mod<L> p, n;
    Num<L> a, b, gx, gy;
    uint32_t algo;
    uint32_t a_kind;  // a = 0 and a = p - 3 save two of the doubling's ten products
};

template <int L>
struct Jac {  // x = X / Z^2, y = Y / Z^3, Montgomery form; Z = 0: the point at infinity
    Num<L> X, Y, Z;
};

// 0 .. L-1 as a parameter pack (std::make_integer_sequence without <utility>).
template <int... I>
struct Seq {};
template <int N, int... I>
struct MakeSeq : MakeSeq<N - 1, N - 1, I...> {};
template <int... I>
struct MakeSeq<0, I...> {
    typedef Seq<I...> type;
};

// ------------------------------------------------------------ limb helpers
template <int L>
EC_HD EC_INLINE bool is_zero(const Num<L>& a) {
    uint32_t v = 0;
    EC_UNROLL
    for (int j = 0; j < L; ++j) v |= a.w[j];
    return v == 0;
}

template <int L>
EC_HD EC_INLINE bool equal(const Num<L>& a, const Num<L>& b) {
    uint32_t v = 0;
    EC_UNROLL
    for (int j = 0; j < L; ++j) v |= a.w[j] ^ b.w[j];
    return v == 0;
}

// r = a + b, returns the carry.
template <int L>
EC_HD EC_INLINE uint32_t add_to(Num<L>& r, const Num<L>& a, const Num<L>& b) {
    uint64_t c = 0;
    EC_UNROLL
    for (int j = 0; j < L; ++j) {
        c += (uint64_t)a.w[j] + b.w[j];
        r.w[j] = (uint32_t)c;
        c >>= 32;
    }
    return (uint32_t)c;
}

// r = a - b, returns the borrow.
template <int L>
EC_HD EC_INLINE uint32_t sub_to(Num<L>& r, const Num<L>& a, const Num<L>& b) {
    uint64_t br = 0;
    EC_UNROLL
    for (int j = 0; j < L; ++j) {
        const uint64_t t = (uint64_t)a.w[j] - b.w[j] - br;
        r.w[j] = (uint32_t)t;
        br = (t >> 32) & 1u;
    }
    return (uint32_t)br;
}

template <int L>
EC_HD EC_INLINE bool geq(const Num<L>& a, const Num<L>& b) {
    Num<L> t;
    return sub_to(t, a, b) == 0;
}

template <int L>
EC_HD EC_INLINE Num<L> select(bool c, const Num<L>& a, const Num<L>& b) {
    Num<L> r;
    EC_UNROLL
    for (int j = 0; j < L; ++j) r.w[j] = c ? a.w[j] : b.w[j];
    return r;
}

template <int L>
EC_HD EC_INLINE Num<L> small(uint32_t v) {
    Num<L> r;
    EC_UNROLL
    for (int j = 0; j < L; ++j) r.w[j] = j ? 0u : v;
    return r;
}

// Shifts a left by one bit and returns the bit that fell out.
template <int L>
EC_HD EC_INLINE uint32_t shl1(Num<L>& a) {
    const uint32_t top = a.w[L - 1] >> 31;
    EC_UNROLL
    for (int j = L - 1; j > 0; --j) a.w[j] = (a.w[j] << 1) | (a.w[j - 1] >> 31);
    a.w[0] <<= 1;
    return top;
}

// (a + b) mod m and (a - b) mod m for a, b < m.
template <int L>
EC_HD EC_INLINE Num<L> mod_add(const Num<L>& a, const Num<L>& b, const Num<L>& m) {
    Num<L> s, d;
    const uint32_t c = add_to(s, a, b);
    const uint32_t br = sub_to(d, s, m);
    return select(c != 0 || br == 0, d, s);
}

template <int L>
EC_HD EC_INLINE Num<L> mod_sub(const Num<L>& a, const Num<L>& b, const Num<L>& m) {
    Num<L> d, e;
    const uint32_t br = sub_to(d, a, b);
    add_to(e, d, m);
    return select(br != 0, e, d);
}

// a mod m by at most `steps` subtractions (the caller knows a < (steps + 1) m).
template <int L>
EC_HD EC_INLINE Num<L> reduce_small(Num<L> a, const Num<L>& m, int steps) {
    for (int k = 0; k < steps; ++k) {
        Num<L> d;
        const uint32_t br = sub_to(d, a, m);
        a = select(br == 0, d, a);
    }
    return a;
}

// ------------------------------------------------- Montgomery multiplication
// a b R^-1 mod m for a, b < m (CIOS, one 32 x 32 + 32 + 32 -> 64 multiply-add
// per limb pair: v_mad_u64_u32 on the device).
//
// The modulus arrives as L scalar arguments, not as a third Num: the device
// calling convention passes at most 16 registers of aggregates by value and
// puts the next aggregate on the stack, which would be scratch memory.
template <int L, typename... Limb>
EC_HD EC_NOINLINE Num<L> mont_mul_raw(Num<L> a, Num<L> b, uint32_t m0inv, Limb... limbs) {
    static_assert(sizeof...(Limb) == L, "one argument per limb of the modulus");
    Num<L> m = {{limbs...}};
    uint32_t t[L + 2];
    EC_UNROLL
    for (int j = 0; j < L + 2; ++j) t[j] = 0;
    EC_UNROLL
    for (int i = 0; i < L; ++i) {
        uint64_t c = 0;
        EC_UNROLL
        for (int j = 0; j < L; ++j) {
            c += (uint64_t)a.w[j] * b.w[i] + t[j];
            t[j] = (uint32_t)c;
            c >>= 32;
        }
        c += t[L];
        t[L] = (uint32_t)c;
        t[L + 1] = (uint32_t)(c >> 32);
        const uint32_t q = t[0] * m0inv;
        c = (uint64_t)q * m.w[0] + t[0];
        c >>= 32;
        EC_UNROLL
        for (int j = 1; j < L; ++j) {
            c += (uint64_t)q * m.w[j] + t[j];
            t[j - 1] = (uint32_t)c;
            c >>= 32;
        }
        c += t[L];
        t[L - 1] = (uint32_t)c;
        t[L] = t[L + 1] + (uint32_t)(c >> 32);
    }
    Num<L> r, d;
    EC_UNROLL
    for (int j = 0; j < L; ++j) r.w[j] = t[j];
    const uint32_t br = sub_to(d, r, m);
    return select(t[L] != 0 || br == 0, d, r);
}

template <int L, int... I>
EC_HD EC_INLINE Num<L> mont_mul_seq(const Num<L>& a, const Num<L>& b, const Mod<L>& M, Seq<I...>) {
    return mont_mul_raw<L>(a, b, M.m0inv, M.m.w[I]...);
}

template <int L>
EC_HD EC_INLINE Num<L> mont_mul(const Num<L>& a, const Num<L>& b, const Mod<L>& M) {
    return mont_mul_seq<L>(a, b, M, typename MakeSeq<L>::type());
}

// The same product with no call boundary.  mont_mul_raw is one out-of-line
// body per translation unit that takes both operands and the modulus by value,
// 3 L + 1 argument registers.  The device calling convention has 32; at L = 12
// and L = 16 the rest goes to the stack, which is scratch memory, at every call
// of the point loop.  mont_mul_rolled is inlined at every site (72 per kernel),
// and so that each site stays a loop the instruction cache holds, its outer
// loop over the limbs of b stays rolled.  A rolled loop cannot index a register
// array by its counter, so b is rotated one limb down per step and the step
// always reads b.w[0]: L moves beside 2 L multiply-adds.  Resources and
// timings: DESIGN.md 5k.
//
// a b R^-1 mod m for a, b < m: the CIOS steps of mont_mul_raw, one limb of b
// per trip of a rolled loop.
template <int L>
EC_HD EC_INLINE Num<L> mont_mul_rolled(const Num<L>& a, Num<L> b, const Mod<L>& M) {
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

// The multiply-reduce as a policy of the formulas below.
struct MulCall {  // one out-of-line body per translation unit
    template <int L>
    static EC_HD EC_INLINE Num<L> mul(const Num<L>& a, const Num<L>& b, const Mod<L>& M) {
        return mont_mul(a, b, M);
    }
};
// b by value, as mont_mul_rolled takes it: with a reference here and the copy
// one level down, the 16-limb kernels place their spilled SGPRs differently
// (DESIGN.md 5k).
struct MulInline {  // no call boundary, rolled
    template <int L>
    static EC_HD EC_INLINE Num<L> mul(const Num<L>& a, Num<L> b, const Mod<L>& M) {
        return mont_mul_rolled(a, b, M);
    }
};

// 8 limbs fit the calling convention; 12 and 16 do not.
template <int L>
struct DefaultMulOf {
    typedef MulInline type;
};
template <>
struct DefaultMulOf<8> {
    typedef MulCall type;
};
template <int L>
using DefaultMul = typename DefaultMulOf<L>::type;

template <int L, class K = DefaultMul<L>>
EC_HD EC_INLINE Num<L> to_mont(const Num<L>& a, const Mod<L>& M) {
    return K::mul(a, M.rr, M);
}

template <int L, class K = DefaultMul<L>>
EC_HD EC_INLINE Num<L> from_mont(const Num<L>& a, const Mod<L>& M) {
    return K::mul(a, small<L>(1), M);
}

// x^-1 in Montgomery form (x^(m-2), m prime); 0 for x = 0.  The exponent is
// the same in every lane, so its branch does not diverge.
template <int L, class K = DefaultMul<L>>
EC_HD EC_INLINE Num<L> mont_inv(const Num<L>& x, const Mod<L>& M) {
    Num<L> r = M.one, e = M.exp;
    EC_NOUNROLL
    for (int i = 0; i < 32 * L; ++i) {
        r = K::mul(r, r, M);
        if (shl1(e)) r = K::mul(r, x, M);
    }
    return r;
}

// ---------------------------------------------------------- point arithmetic
// 2 P (dbl-1998-cmo-2): also right for P = O and for a point of order two
// (Y = 0), both of which give Z = 0.  M = 3 X^2 + a Z^4 costs three products
// for a general a, one for a = 0 and two for a = -3 (3 (X - Z^2) (X + Z^2));
// a_kind is the same in every lane.
template <int L, class K = DefaultMul<L>>
EC_HD EC_INLINE Jac<L> jac_dbl(const Jac<L>& P, const Curve<L>& C) {
    const Mod<L>& F = C.p;
    const Num<L> yy = K::mul(P.Y, P.Y, F);
    const Num<L> yyyy = K::mul(yy, yy, F);
    Num<L> s = K::mul(P.X, yy, F);
    s = mod_add(s, s, F.m);
    s = mod_add(s, s, F.m);  // 4 X Y^2
    Num<L> m;
    if (C.a_kind == kAMinus3) {
        const Num<L> zz = K::mul(P.Z, P.Z, F);
        m = K::mul(mod_sub(P.X, zz, F.m), mod_add(P.X, zz, F.m), F);
        m = mod_add(mod_add(m, m, F.m), m, F.m);
    } else {
        const Num<L> xx = K::mul(P.X, P.X, F);
        m = mod_add(mod_add(xx, xx, F.m), xx, F.m);
        if (C.a_kind != kAZero) {
            const Num<L> zz = K::mul(P.Z, P.Z, F);
            m = mod_add(m, K::mul(C.a, K::mul(zz, zz, F), F), F.m);
        }
    }
    Jac<L> R;
    R.X = mod_sub(K::mul(m, m, F), mod_add(s, s, F.m), F.m);
    Num<L> y8 = mod_add(yyyy, yyyy, F.m);
    y8 = mod_add(y8, y8, F.m);
    y8 = mod_add(y8, y8, F.m);
    const Num<L> yz = K::mul(P.Y, P.Z, F);
    R.Y = mod_sub(K::mul(m, mod_sub(s, R.X, F.m), F), y8, F.m);
    R.Z = mod_add(yz, yz, F.m);
    return R;
}

// P + (x2, y2) for an affine (x2, y2) on the curve (madd).  P = O gives the
// affine point, P = (x2, y2) the doubling, P = -(x2, y2) the point at
// infinity.
template <int L, class K = DefaultMul<L>>
EC_HD EC_INLINE Jac<L> jac_add_affine(const Jac<L>& P, const Num<L>& x2, const Num<L>& y2, const Curve<L>& C) {
    const Mod<L>& F = C.p;
    Jac<L> R;
    if (is_zero(P.Z)) {
        R.X = x2;
        R.Y = y2;
        R.Z = F.one;
        return R;
    }
    const Num<L> zz = K::mul(P.Z, P.Z, F);
    const Num<L> u2 = K::mul(x2, zz, F);
    const Num<L> s2 = K::mul(y2, K::mul(P.Z, zz, F), F);
    const Num<L> h = mod_sub(u2, P.X, F.m);
    const Num<L> r = mod_sub(s2, P.Y, F.m);
    if (is_zero(h)) {
        if (is_zero(r)) {
            R.X = x2;
            R.Y = y2;
            R.Z = F.one;
            return jac_dbl<L, K>(R, C);
        }
        R.X = F.one;
        R.Y = F.one;
        R.Z = small<L>(0);
        return R;
    }
    const Num<L> hh = K::mul(h, h, F);
    const Num<L> hhh = K::mul(h, hh, F);
    const Num<L> v = K::mul(P.X, hh, F);
    R.X = mod_sub(mod_sub(K::mul(r, r, F), hhh, F.m), mod_add(v, v, F.m), F.m);
    R.Y = mod_sub(K::mul(r, mod_sub(v, R.X, F.m), F), K::mul(P.Y, hhh, F), F.m);
    R.Z = K::mul(P.Z, h, F);
    return R;
}

// Affine x (and y where wanted) of R, Z != 0, as plain numbers below p.
template <int L, class K = DefaultMul<L>>
EC_HD EC_INLINE void jac_to_affine(const Jac<L>& R, const Mod<L>& F, Num<L>& x, Num<L>* y) {
    const Num<L> zi = mont_inv<L, K>(R.Z, F);
    const Num<L> zi2 = K::mul(zi, zi, F);
    x = from_mont<L, K>(K::mul(R.X, zi2, F), F);
    if (y) *y = from_mont<L, K>(K::mul(R.Y, K::mul(zi2, zi, F), F), F);
}

// ------------------------------------------------------------------- import
// The number in p[0 .. nbytes), nbytes <= 4 L, big-endian or little-endian.
// No byte outside p[0 .. nbytes) is read.
template <int L>
EC_HD EC_INLINE Num<L> load_num(const uint8_t* p, uint32_t nbytes, bool le) {
    Num<L> r;
    EC_UNROLL
    for (int j = 0; j < L; ++j) {
        uint32_t v = 0;
        EC_UNROLL
        for (int k = 0; k < 4; ++k) {
            const uint32_t q = 4u * j + k;  // byte of significance 256^q
            if (q < nbytes) v |= (uint32_t)p[le ? q : nbytes - 1 - q] << (8 * k);
        }
        r.w[j] = v;
    }
    return r;
}

// The number a as 4 L bytes at p, big-endian or little-endian.
template <int L>
EC_HD EC_INLINE void store_num(uint8_t* p, const Num<L>& a, bool le) {
    EC_UNROLL
    for (int j = 0; j < L; ++j) {
        EC_UNROLL
        for (int k = 0; k < 4; ++k) {
            const int q = 4 * j + k;  // byte of significance 256^q
            p[le ? q : 4 * L - 1 - q] = (uint8_t)(a.w[j] >> (8 * k));
        }
    }
}

// ------------------------------------------------------------------- verify
// What the reference's ecdsa_verify_be / ecdsa_verify_le return for numbers
// of 4 L bytes (ecdsa.h:1366-1523): the public key check, the range check of
// r and s, the hash import and its reduction, u1 G + u2 Q, R.x mod n = r.
template <int L, class K = DefaultMul<L>>
EC_HD EC_INLINE int verify_one(const Curve<L>& C, const uint8_t* hash, uint32_t hash_size, const uint8_t* sig_r,
                               const uint8_t* sig_s, const uint8_t* key_x, const uint8_t* key_y, bool le) {
    const Mod<L>& F = C.p;
    const Mod<L>& N = C.n;
    // Public key: coordinates below p, on the curve.  Every supported curve
    // has cofactor 1, so n Q = O follows and is not computed.
    const Num<L> qx = load_num<L>(key_x, 4 * L, le), qy = load_num<L>(key_y, 4 * L, le);
    if (geq(qx, F.m) || geq(qy, F.m)) return kBadPoint;
    const Num<L> x = to_mont<L, K>(qx, F), y = to_mont<L, K>(qy, F);
    {
        const Num<L> lhs = K::mul(y, y, F);
        const Num<L> xxa = mod_add(K::mul(x, x, F), C.a, F.m);
        const Num<L> rhs = mod_add(K::mul(xxa, x, F), C.b, F.m);
        if (!equal(lhs, rhs)) return kBadPoint;
    }
    const Num<L> r = load_num<L>(sig_r, 4 * L, le), s = load_num<L>(sig_s, 4 * L, le);
    if (geq(r, N.m) || geq(s, N.m)) return kEinval;
    // The reference's bn_mod_reduce: e itself below n, else (e mod (n - 1)) + 1.
    // n > 2^(32 L - 2) (checked by curve_setup), so three subtractions do.
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
        const Num<L> w = mont_inv<L, K>(to_mont<L, K>(s, N), N);  // s^-1 R
        u1 = K::mul(e, w, N);
        u2 = K::mul(r, w, N);
    } else {
        if (is_zero(e)) e = small<L>(1);
        const Num<L> w = mont_inv<L, K>(to_mont<L, K>(e, N), N);  // e^-1 R
        u1 = K::mul(s, w, N);
        const Num<L> t = K::mul(r, w, N);
        u2 = mod_sub(small<L>(0), t, N.m);  // -(r e^-1)
    }
    // G + Q in affine form for Shamir's trick over {G, Q, G + Q}; it may be a
    // doubling (Q = G) or the point at infinity (Q = -G).
    Jac<L> R;
    R.X = C.gx;
    R.Y = C.gy;
    R.Z = F.one;
    R = jac_add_affine<L, K>(R, x, y, C);
    const bool gq_inf = is_zero(R.Z);
    Num<L> gqx, gqy;
    {
        const Num<L> zi = mont_inv<L, K>(R.Z, F);
        const Num<L> zi2 = K::mul(zi, zi, F);
        gqx = K::mul(R.X, zi2, F);
        gqy = K::mul(R.Y, K::mul(zi2, zi, F), F);
    }
    R.X = F.one;
    R.Y = F.one;
    R.Z = small<L>(0);
    EC_NOUNROLL
    for (int i = 0; i < 32 * L; ++i) {
        const bool b1 = shl1(u1) != 0, b2 = shl1(u2) != 0;
        R = jac_dbl<L, K>(R, C);
        if ((b1 || b2) && !(b1 && b2 && gq_inf)) {
            const Num<L> tx = select(b2, select(b1, gqx, x), C.gx);
            const Num<L> ty = select(b2, select(b1, gqy, y), C.gy);
            R = jac_add_affine<L, K>(R, tx, ty, C);
        }
    }
    if (is_zero(R.Z)) return kBadPoint;
    // R.x mod n = r without inverting Z: R.x = X / Z^2 < p < 2^(32 L) < 4 n, so
    // R.x mod n = r exactly when X = (r + k n) Z^2 for one k in 0..3 with
    // r + k n < p.  k > 0 is live only where p is well above n.
    const Num<L> zz = K::mul(R.Z, R.Z, F);
    Num<L> t = r;
    bool live = true, ok = false;
    for (int k = 0; k < 4; ++k) {
        if (live && !geq(t, F.m)) ok = ok || equal(K::mul(to_mont<L, K>(t, F), zz, F), R.X);
        Num<L> u;
        if (add_to(u, t, N.m)) live = false;  // past 2^(32 L), so past p
        t = u;
    }
    return ok ? 0 : kBadSign;
}

// ------------------------------------------------------------ per-curve setup
// Montgomery constants of the odd modulus m > 1 (host side, once per curve).
template <int L>
EC_HD inline void mod_setup(Mod<L>& M, const Num<L>& m) {
    M.m = m;
    uint32_t inv = 1;  // Newton: inv = m^-1 mod 2^32
    for (int k = 0; k < 5; ++k) inv *= 2u - m.w[0] * inv;
    M.m0inv = 0u - inv;
    Num<L> v = small<L>(1);
    for (int k = 0; k < 32 * L; ++k) v = mod_add(v, v, m);
    M.one = v;
    for (int k = 0; k < 32 * L; ++k) v = mod_add(v, v, m);
    M.rr = v;
    sub_to(M.exp, m, small<L>(2));
}

// raw: p, a, b, Gx, Gy, n as 6 x 4 L big-endian bytes.  False where the
// numbers do not fit verify_one's bounds (odd p and n above 2^(32 L - 2),
// a, b, Gx, Gy below p).
template <int L>
EC_HD inline bool curve_setup(Curve<L>& C, const uint8_t* raw, uint32_t algo) {
    Num<L> v[6];
    for (int k = 0; k < 6; ++k) v[k] = load_num<L>(raw + 4 * L * k, 4 * L, false);
    const Num<L>&p = v[0], &n = v[5];
    if (!(p.w[0] & 1u) || !(n.w[0] & 1u) || (p.w[L - 1] >> 30) == 0 || (n.w[L - 1] >> 30) == 0) return false;
    if (algo != kAlgoEcdsa && algo != kAlgoGost) return false;
    for (int k = 1; k < 5; ++k)
        if (geq(v[k], p)) return false;
    mod_setup(C.p, p);
    mod_setup(C.n, n);
    C.a = to_mont(v[1], C.p);
    C.b = to_mont(v[2], C.p);
    C.gx = to_mont(v[3], C.p);
    C.gy = to_mont(v[4], C.p);
    C.algo = algo;
    Num<L> pm3;
    sub_to(pm3, p, small<L>(3));
    C.a_kind = is_zero(v[1]) ? kAZero : (equal(v[1], pm3) ? kAMinus3 : kAGeneral);
    return true;
}

}  // namespace lcbec
