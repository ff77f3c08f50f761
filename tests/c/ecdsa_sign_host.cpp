// ecdsa_sign_host.cpp — liblcb_amd/csrc/ecdsa_sign_math.hpp compiled for the
// host (tests/test_ecdsa_sign_host.py builds it with AddressSanitizer and
// UBSan): the same table, the same base_mult() and the same sign_one(),
// keygen_one() and pubkey_one() the kernels run per lane.
//
// Reads lines of hex words on stdin and answers one line each:
//   C algo p a b Gx Gy n       set the curve (32 big-endian bytes each) and
//                              derive its window table -> "C ok" | "C bad"
//   T j v                      -> "x y" of the table entry v 16^j G (v = 1 .. 15),
//                                 out of Montgomery form, big-endian
//   S le hash_size hash d rnd  -> "status r s"    (r, s: the 32 bytes written)
//   K le rnd                   -> "status d Qx Qy"
//   P le d                     -> "status Qx Qy"
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
constexpr int L = 8;

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

static std::string hex_num(const Num<L>& a, bool le) {
    std::unique_ptr<uint8_t[]> b(new uint8_t[4 * L]);
    store_num<L>(b.get(), a, le);
    return hex(b.get(), 4 * L);
}

// An exact-size heap copy of a number of 4 L bytes.
static std::unique_ptr<uint8_t[]> exact(const std::string& h, size_t size) {
    const std::vector<uint8_t> b = unhex(h);
    if (b.size() != size) exit(4);
    std::unique_ptr<uint8_t[]> p(new uint8_t[size]);
    memcpy(p.get(), b.data(), size);
    return p;
}

int main() {
    Curve<L> C;
    std::unique_ptr<BaseTable<L>> T;
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
            for (int k = 0; k < 6; ++k) {
                std::string h;
                in >> h;
                const std::vector<uint8_t> b = unhex(h);
                if (b.size() != 4 * L) return 2;
                raw.insert(raw.end(), b.begin(), b.end());
            }
            T.reset();
            if (curve_setup(C, raw.data(), algo)) {
                T.reset(new BaseTable<L>);
                std::vector<Jac<L>> pts(8 * L * kWinEntries);
                std::vector<Num<L>> pre(8 * L * kWinEntries);
                if (!base_table_setup(*T, C, pts.data(), pre.data())) T.reset();
            }
            printf(T ? "C ok\n" : "C bad\n");
            continue;
        }
        if (!T) return 3;
        int le = 0;
        if (op == "T") {
            int j, v;
            in >> j >> v;
            if (j < 0 || j >= 8 * L || v < 1 || v > kWinEntries) return 6;
            const Aff<L>& a = T->t[j][v - 1];
            printf("%s %s\n", hex_num(from_mont(a.x, C.p), false).c_str(), hex_num(from_mont(a.y, C.p), false).c_str());
        } else if (op == "S") {
            uint32_t hash_size;
            std::string h, d, k;
            in >> le >> hash_size >> h >> d >> k;
            const auto hb = exact(h, hash_size), db = exact(d, 4 * L), kb = exact(k, 4 * L);
            Num<L> r, s;
            const int st = sign_one<L>(C, T.get(), hb.get(), hash_size, db.get(), kb.get(), le != 0, r, s);
            printf("%d %s %s\n", st, hex_num(r, le != 0).c_str(), hex_num(s, le != 0).c_str());
        } else if (op == "K") {
            std::string k;
            in >> le >> k;
            const auto kb = exact(k, 4 * L);
            Num<L> d, x, y;
            const int st = keygen_one<L>(C, T.get(), kb.get(), le != 0, d, x, y);
            printf("%d %s %s %s\n", st, hex_num(d, le != 0).c_str(), hex_num(x, le != 0).c_str(),
                   hex_num(y, le != 0).c_str());
        } else if (op == "P") {
            std::string d;
            in >> le >> d;
            const auto db = exact(d, 4 * L);
            Num<L> x, y;
            const int st = pubkey_one<L>(C, T.get(), db.get(), le != 0, x, y);
            printf("%d %s %s\n", st, hex_num(x, le != 0).c_str(), hex_num(y, le != 0).c_str());
        } else {
            return 5;
        }
    }
    return 0;
}
