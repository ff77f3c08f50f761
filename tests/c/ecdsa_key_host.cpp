// ecdsa_key_host.cpp — liblcb_amd/csrc/ecdsa_key_math.hpp compiled for the
// host (tests/test_ecdsa_key_host.py builds it with AddressSanitizer and
// UBSan): the same key_import_one() and key_export_one() the kernels run per
// lane, and key_setup() as the library runs it once per curve.
//
// Reads lines of words on stdin and answers one line each:
//   C algo p a b Gx Gy n    set the curve (32 big-endian bytes each)
//                           -> "C ok s exp c" (key_setup's constants, exp and
//                           the plain value of c as big-endian hex) | "C bad"
//   I le size key key_y     key, key_y: hex or "-" (empty / NULL)
//                           -> "status infinity xy"  (xy: the 64 bytes written)
//   E le compress inf xy    -> "size out"   (out: the `size` bytes written)
//   S v                     v: 32 big-endian bytes below p
//                           -> "r ok"  (the root candidate, ok = r^2 == v)
// Every buffer handed over is a heap block of exactly its size, so a read
// past any of them is an error here.  Outputs sit between two canary blocks
// inside one heap block; the export's block ends right after the item's size.
// A canary that changed ends the program with exit code 7.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../liblcb_amd/csrc/ecdsa_key_math.hpp"

using namespace lcbec;
constexpr int L = 8;
constexpr size_t kGuard = 16;
constexpr uint8_t kCanary = 0xC7;

static std::vector<uint8_t> unhex(const std::string& s) {
    if (s == "-") return {};
    std::vector<uint8_t> out(s.size() / 2);
    for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return out;
}

static std::string hex(const uint8_t* p, size_t n) {
    std::string s(2 * n, '0');
    for (size_t i = 0; i < n; ++i) snprintf(&s[2 * i], 3, "%02x", p[i]);
    return s;
}

static std::string hex_num(const Num<L>& a) {
    uint8_t b[4 * L];
    store_num<L>(b, a, false);
    return hex(b, sizeof b);
}

// An exact-size heap copy.
static std::unique_ptr<uint8_t[]> exact(const std::vector<uint8_t>& b) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[b.size()]);
    if (!b.empty()) memcpy(p.get(), b.data(), b.size());
    return p;
}

// `size` bytes between two canary blocks.
struct Box {
    std::unique_ptr<uint8_t[]> mem;
    size_t size;
    explicit Box(size_t n) : mem(new uint8_t[kGuard + n + kGuard]), size(n) { memset(mem.get(), kCanary, kGuard + n + kGuard); }
    uint8_t* out() { return mem.get() + kGuard; }
    bool intact(size_t written) const {
        for (size_t i = 0; i < kGuard; ++i)
            if (mem[i] != kCanary) return false;
        for (size_t i = kGuard + written; i < kGuard + size + kGuard; ++i)
            if (mem[i] != kCanary) return false;
        return true;
    }
};

int main() {
    Curve<L> C;
    KeyConsts<L> K;
    bool have = false;
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
            have = curve_setup(C, raw.data(), algo) && key_setup(K, C);
            if (have)
                printf("C ok %u %s %s\n", K.s, hex_num(K.exp).c_str(), hex_num(from_mont(K.c, C.p)).c_str());
            else
                printf("C bad\n");
        } else if (op == "I") {
            if (!have) return 3;
            int le = 0;
            unsigned size = 0;
            std::string kh, yh;
            in >> le >> size >> kh >> yh;
            const std::vector<uint8_t> kb = unhex(kh), yb = unhex(yh);
            if (kb.size() != size || (yh != "-" && yb.size() != 4 * L)) return 4;
            const auto key = exact(kb), key_y = exact(yb);
            Box xy(2 * 4 * L), inf(1);
            const int st =
                key_import_one<L>(C, K, key.get(), size, yh == "-" ? nullptr : key_y.get(), le != 0, xy.out(), inf.out());
            if (!xy.intact(2 * 4 * L) || !inf.intact(1)) return 7;
            if ((size && memcmp(key.get(), kb.data(), size)) || (yh != "-" && memcmp(key_y.get(), yb.data(), 4 * L)))
                return 8;  // an input changed
            // without the flag: the same status and bytes
            Box xy2(2 * 4 * L);
            if (key_import_one<L>(C, K, key.get(), size, yh == "-" ? nullptr : key_y.get(), le != 0, xy2.out(),
                                  nullptr) != st ||
                !xy2.intact(2 * 4 * L) || memcmp(xy.out(), xy2.out(), 2 * 4 * L))
                return 9;
            printf("%d %u %s\n", st, (unsigned)*inf.out(), hex(xy.out(), 2 * 4 * L).c_str());
        } else if (op == "E") {
            int le = 0, compress = 0, inf = 0;
            std::string ph;
            in >> le >> compress >> inf >> ph;
            const std::vector<uint8_t> pb = unhex(ph);
            if (pb.size() != 2 * 4 * L) return 4;
            const auto pub = exact(pb);
            const size_t want = inf ? 1 : (compress ? 4 * L + 1 : 2 * 4 * L + 1);
            Box out(want);  // a byte past the item's size lands in the canary
            const uint32_t size = key_export_one<L>(pub.get(), inf != 0, compress != 0, le != 0, out.out());
            if (size != want || !out.intact(size)) return 7;
            if (memcmp(pub.get(), pb.data(), pb.size())) return 8;
            printf("%u %s\n", size, hex(out.out(), size).c_str());
        } else if (op == "S") {
            if (!have) return 3;
            std::string vh;
            in >> vh;
            const std::vector<uint8_t> vb = unhex(vh);
            if (vb.size() != 4 * L) return 4;
            const Num<L> v = load_num<L>(vb.data(), 4 * L, false);
            if (geq(v, C.p.m)) return 6;
            const Num<L> vm = to_mont(v, C.p);
            const Num<L> r = mont_sqrt(vm, K, C.p);
            printf("%s %d\n", hex_num(from_mont(r, C.p)).c_str(), equal(mont_mul(r, r, C.p), vm) ? 1 : 0);
        } else {
            return 5;
        }
    }
    return 0;
}
