// ecdsa_verify_host.cpp — liblcb_amd/csrc/ecdsa_math.hpp compiled for the
// host (tests/test_ecdsa_host.py builds it with AddressSanitizer and UBSan):
// the same arithmetic and the same verify_one() the kernel runs per lane.
//
// Reads lines of hex words on stdin and answers one line each:
//   C algo p a b Gx Gy n          set the curve (32 big-endian bytes each)
//                                 -> "C ok m0inv_p one_p rr_p m0inv_n one_n rr_n" | "C bad"
//   M p|n a b                     -> the Montgomery product a b R^-1 mod m, two words:
//                                    MulCall::mul(a, b) and MulInline::mul(a, b)
//   I p|n a                       -> a^-1 mod m (through to_mont, mont_inv, from_mont)
//   V le hash_size hash r s Qx Qy -> the status of verify_one
// Every buffer handed to verify_one is a heap block of exactly its size, so a
// read past hash_size or past a number's 32 bytes is an error here.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../liblcb_amd/csrc/ecdsa_math.hpp"

using namespace lcbec;
constexpr int L = 8;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out(s.size() / 2);
    for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return out;
}

static Num<L> num_be(const std::string& s) {
    const std::vector<uint8_t> b = unhex(s);
    return load_num<L>(b.data(), (uint32_t)b.size(), false);
}

static std::string hex_be(const Num<L>& a) {
    char buf[8 * L + 1];
    for (int j = 0; j < L; ++j) snprintf(buf + 8 * j, 9, "%08x", a.w[L - 1 - j]);
    return buf;
}

int main() {
    Curve<L> C;
    bool have = false;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        in >> op;
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
            have = curve_setup(C, raw.data(), algo);
            if (!have) {
                printf("C bad\n");
                continue;
            }
            printf("C ok %08x %s %s %08x %s %s\n", C.p.m0inv, hex_be(C.p.one).c_str(), hex_be(C.p.rr).c_str(),
                   C.n.m0inv, hex_be(C.n.one).c_str(), hex_be(C.n.rr).c_str());
        } else if (op == "M" || op == "I") {
            if (!have) return 3;
            std::string which, a, b;
            in >> which >> a;
            const Mod<L>& M = which == "p" ? C.p : C.n;
            if (op == "M") {
                in >> b;
                printf("%s %s\n", hex_be(MulCall::mul(num_be(a), num_be(b), M)).c_str(),
                       hex_be(MulInline::mul(num_be(a), num_be(b), M)).c_str());
            } else {
                printf("%s\n", hex_be(from_mont(mont_inv(to_mont(num_be(a), M), M), M)).c_str());
            }
        } else if (op == "V") {
            if (!have) return 3;
            int le;
            uint32_t hash_size;
            std::string h, r, s, qx, qy;
            in >> le >> hash_size >> h >> r >> s >> qx >> qy;
            // exact-size heap copies: the hash holds hash_size bytes only
            std::vector<uint8_t> hb = unhex(h), rb = unhex(r), sb = unhex(s), xb = unhex(qx), yb = unhex(qy);
            if (hb.size() < hash_size || rb.size() != 4 * L || sb.size() != 4 * L || xb.size() != 4 * L ||
                yb.size() != 4 * L)
                return 4;
            hb.resize(hash_size);
            hb.shrink_to_fit();
            printf("%d\n", verify_one(C, hb.data(), hash_size, rb.data(), sb.data(), xb.data(), yb.data(), le != 0));
        } else if (!op.empty()) {
            return 5;
        }
    }
    return 0;
}
