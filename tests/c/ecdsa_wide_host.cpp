// ecdsa_wide_host.cpp — liblcb_amd/csrc/ecdsa_math.hpp at 12 and 16 limbs
// compiled for the host (tests/test_ecdsa_wide_host.py builds it with
// AddressSanitizer and UBSan): the same arithmetic and the same
// verify_one<L, MulInline>() the wide kernels run per lane, over the library's
// own curve table (ecdsa_wide_host.hpp), side by side with the same formulas
// over the other multiply-reduce, verify_one<L, MulCall>().
//
// Reads lines of hex words on stdin and answers one line each:
//   K id                             -> "K B m0inv_p one_p rr_p m0inv_n one_n rr_n" | "K bad"
//   M id p|n a b                     -> MulInline::mul(a, b) and MulCall::mul(a, b), two words
//   I id p|n a                       -> a^-1 mod m through to_mont, mont_inv over MulInline
//   V id le hash_size hash r s Qx Qy -> the statuses of verify_one over MulInline and over MulCall, two words
// Every buffer handed to the verification is a heap block of exactly its
// size, so a read past hash_size or past a number's B bytes is an error here.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../liblcb_amd/csrc/ecdsa_wide_host.hpp"

using namespace lcbec;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out(s.size() / 2);
    for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return out;
}

template <int L>
static Num<L> num_be(const std::string& s) {
    const std::vector<uint8_t> b = unhex(s);
    return load_num<L>(b.data(), (uint32_t)b.size(), false);
}

template <int L>
static std::string hex_be(const Num<L>& a) {
    char buf[8 * L + 1];
    for (int j = 0; j < L; ++j) snprintf(buf + 8 * j, 9, "%08x", a.w[L - 1 - j]);
    return buf;
}

template <int L>
static int serve(const Curve<L>& C, const std::string& op, std::istringstream& in) {
    if (op == "K") {
        printf("K %d %08x %s %s %08x %s %s\n", 4 * L, C.p.m0inv, hex_be(C.p.one).c_str(), hex_be(C.p.rr).c_str(),
               C.n.m0inv, hex_be(C.n.one).c_str(), hex_be(C.n.rr).c_str());
    } else if (op == "M" || op == "I") {
        std::string which, a, b;
        in >> which >> a;
        const Mod<L>& M = which == "p" ? C.p : C.n;
        if (op == "M") {
            in >> b;
            printf("%s %s\n", hex_be(MulInline::mul(num_be<L>(a), num_be<L>(b), M)).c_str(),
                   hex_be(MulCall::mul(num_be<L>(a), num_be<L>(b), M)).c_str());
        } else {
            const Num<L> inv = mont_inv<L, MulInline>(to_mont<L, MulInline>(num_be<L>(a), M), M);
            printf("%s\n", hex_be(MulInline::mul(inv, small<L>(1), M)).c_str());
        }
    } else if (op == "V") {
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
        printf("%d %d\n",
               verify_one<L, MulInline>(C, hb.data(), hash_size, rb.data(), sb.data(), xb.data(), yb.data(), le != 0),
               verify_one<L, MulCall>(C, hb.data(), hash_size, rb.data(), sb.data(), xb.data(), yb.data(), le != 0));
    } else {
        return 5;
    }
    return 0;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        int id = -1;
        in >> op;
        if (op.empty()) continue;
        in >> id;
        if (!wide_known(id)) {
            if (op != "K") return 3;
            printf("K bad\n");
            continue;
        }
        const int rc = kWideCurves[id].bytes == 48 ? serve(wide_table().c12[id], op, in)
                                                   : serve(wide_table().c16[id], op, in);
        if (rc) return rc;
    }
    return 0;
}
