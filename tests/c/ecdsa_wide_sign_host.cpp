// ecdsa_wide_sign_host.cpp — liblcb_amd/csrc/ecdsa_sign_math.hpp at 12 and 16
// limbs compiled for the host (tests/test_ecdsa_wide_sign_host.py builds it
// with AddressSanitizer and UBSan): the same table, the same base_mult() and
// the same sign_one<L, MulInline>() and key_one<L, MulInline>() the wide
// kernels run per lane, beside sign_one<L, MulCall>() / key_one<L, MulCall>(),
// the same formulas over the other multiply-reduce, and
// verify_one<L, MulInline>() of ecdsa_math.hpp.
//
// Reads lines of hex words on stdin and answers one line each:
//   C algo p a b Gx Gy n       set the curve (B = 48 or 64 big-endian bytes
//                              each, B picks the limb count) and derive its
//                              window table -> "C ok" | "C bad"
//   T j v                      -> "x y" of the table entry v 16^j G (v = 1 .. 15),
//                                 out of Montgomery form, big-endian
//   S le hash_size hash d rnd  -> "status r s same verify": r, s the B bytes
//                                 written; same = 1 where MulCall gave the
//                                 same status and numbers; verify = the status
//                                 of verify_one for (hash, r, s) under
//                                 key_one's key of d, or "-" where that
//                                 does not apply (status != 0 or d = 0)
//   K le rnd                   -> "status d Qx Qy same"
//   P le d                     -> "status Qx Qy same"
// Every buffer handed to the *_one functions is a heap block of exactly its
// size, the table included, so a read past any of them is an error here.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../liblcb_amd/csrc/ecdsa_sign_math.hpp"

using namespace lcbec;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out(s.size() / 2);
    for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return out;
}

static std::string hex(const uint8_t* p, size_t n) {
    std::string s(2 * n, '0');
    for (size_t i = 0; i < n; ++i) snprintf(&s[2 * i], 3, "%02x", p[i]);
    return s;
}

// An exact-size heap copy of a byte string.
static std::unique_ptr<uint8_t[]> exact(const std::string& h, size_t size) {
    const std::vector<uint8_t> b = unhex(h);
    if (b.size() != size) exit(4);
    std::unique_ptr<uint8_t[]> p(new uint8_t[size]);
    memcpy(p.get(), b.data(), size);
    return p;
}

template <int L>
static std::unique_ptr<uint8_t[]> bytes_of(const Num<L>& a, bool le) {
    std::unique_ptr<uint8_t[]> b(new uint8_t[4 * L]);
    store_num<L>(b.get(), a, le);
    return b;
}

template <int L>
static std::string hex_num(const Num<L>& a, bool le) {
    return hex(bytes_of<L>(a, le).get(), 4 * L);
}

template <int L>
struct Bench {
    Curve<L> C;
    std::unique_ptr<BaseTable<L>> T;

    bool setup(const std::vector<uint8_t>& raw, uint32_t algo) {
        T.reset();
        if (!curve_setup(C, raw.data(), algo)) return false;
        T.reset(new BaseTable<L>);
        std::vector<Jac<L>> pts(8 * L * kWinEntries);
        std::vector<Num<L>> pre(8 * L * kWinEntries);
        if (!base_table_setup(*T, C, pts.data(), pre.data())) T.reset();
        return (bool)T;
    }

    int line(const std::string& op, std::istringstream& in) {
        if (!T) return 3;
        int le = 0;
        if (op == "T") {
            int j, v;
            in >> j >> v;
            if (j < 0 || j >= 8 * L || v < 1 || v > kWinEntries) return 6;
            const Aff<L>& a = T->t[j][v - 1];
            printf("%s %s\n", hex_num<L>(from_mont<L, MulInline>(a.x, C.p), false).c_str(),
                   hex_num<L>(from_mont<L, MulInline>(a.y, C.p), false).c_str());
        } else if (op == "S") {
            uint32_t hash_size;
            std::string h, d, k;
            in >> le >> hash_size >> h >> d >> k;
            const auto hb = exact(h, hash_size), db = exact(d, 4 * L), kb = exact(k, 4 * L);
            Num<L> r, s, r2, s2;
            const int st = sign_one<L, MulInline>(C, T.get(), hb.get(), hash_size, db.get(), kb.get(), le != 0, r, s);
            const int st2 = sign_one<L, MulCall>(C, T.get(), hb.get(), hash_size, db.get(), kb.get(), le != 0, r2, s2);
            const bool same = st == st2 && equal(r, r2) && equal(s, s2);
            std::string ver = "-";
            if (st == 0) {
                Num<L> dd, x, y;
                if (key_one<L, MulInline>(C, T.get(), db.get(), false, le != 0, dd, x, y) == 0) {
                    const auto rb = bytes_of<L>(r, le != 0), sb = bytes_of<L>(s, le != 0);
                    const auto xb = bytes_of<L>(x, le != 0), yb = bytes_of<L>(y, le != 0);
                    ver = std::to_string(verify_one<L, MulInline>(C, hb.get(), hash_size, rb.get(), sb.get(), xb.get(),
                                                                  yb.get(), le != 0));
                }
            }
            printf("%d %s %s %d %s\n", st, hex_num<L>(r, le != 0).c_str(), hex_num<L>(s, le != 0).c_str(), (int)same,
                   ver.c_str());
        } else if (op == "K" || op == "P") {
            const bool gen = op == "K";
            std::string k;
            in >> le >> k;
            const auto kb = exact(k, 4 * L);
            Num<L> d, x, y, d2, x2, y2;
            const int st = key_one<L, MulInline>(C, T.get(), kb.get(), gen, le != 0, d, x, y);
            const int st2 = key_one<L, MulCall>(C, T.get(), kb.get(), gen, le != 0, d2, x2, y2);
            const bool same = st == st2 && equal(d, d2) && equal(x, x2) && equal(y, y2);
            if (gen)
                printf("%d %s %s %s %d\n", st, hex_num<L>(d, le != 0).c_str(), hex_num<L>(x, le != 0).c_str(),
                       hex_num<L>(y, le != 0).c_str(), (int)same);
            else
                printf("%d %s %s %d\n", st, hex_num<L>(x, le != 0).c_str(), hex_num<L>(y, le != 0).c_str(), (int)same);
        } else {
            return 5;
        }
        return 0;
    }
};

int main() {
    Bench<12> b12;
    Bench<16> b16;
    int limbs = 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        in >> op;
        if (op.empty()) continue;
        if (op == "C") {
            uint32_t algo;
            in >> algo;
            std::vector<uint8_t> raw;
            size_t B = 0;
            for (int k = 0; k < 6; ++k) {
                std::string h;
                in >> h;
                const std::vector<uint8_t> b = unhex(h);
                if (k == 0) B = b.size();
                if ((B != 48 && B != 64) || b.size() != B) return 2;
                raw.insert(raw.end(), b.begin(), b.end());
            }
            limbs = (int)(B / 4);
            const bool ok = limbs == 12 ? b12.setup(raw, algo) : b16.setup(raw, algo);
            printf(ok ? "C ok\n" : "C bad\n");
            continue;
        }
        const int rc = limbs == 12 ? b12.line(op, in) : limbs == 16 ? b16.line(op, in) : 3;
        if (rc) return rc;
    }
    return 0;
}
