// ecdsa_dh_host.cpp — liblcb_amd/csrc/ecdsa_dh_math.hpp compiled for the host
// (tests/test_ecdsa_dh_host.py builds it with AddressSanitizer and UBSan):
// the same dh_one() the kernel runs per lane.
//
// Reads lines of hex words on stdin and answers one line each:
//   C algo p a b Gx Gy n   set the curve (32 big-endian bytes each) -> "C ok" | "C bad"
//   D le Qx Qy d           -> "status shared"   (shared: the 32 bytes written)
// Every buffer handed to dh_one() is a heap block of exactly its size, so a
// read past any of them is an error here.  The output sits between two canary
// blocks inside one heap block; a canary that changed ends the program with
// exit code 7.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../liblcb_amd/csrc/ecdsa_dh_math.hpp"

using namespace lcbec;
constexpr int L = 8;
constexpr size_t kGuard = 16;
constexpr uint8_t kCanary = 0xC7;

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
            have = curve_setup(C, raw.data(), algo);
            printf(have ? "C ok\n" : "C bad\n");
        } else if (op == "D") {
            if (!have) return 3;
            int le = 0;
            std::string qx, qy, d;
            in >> le >> qx >> qy >> d;
            const auto xb = exact(qx, 4 * L), yb = exact(qy, 4 * L), db = exact(d, 4 * L);
            const std::vector<uint8_t> keep_x(xb.get(), xb.get() + 4 * L), keep_y(yb.get(), yb.get() + 4 * L),
                keep_d(db.get(), db.get() + 4 * L);
            std::unique_ptr<uint8_t[]> box(new uint8_t[kGuard + 4 * L + kGuard]);
            memset(box.get(), kCanary, kGuard + 4 * L + kGuard);
            uint8_t* out = box.get() + kGuard;
            const int st = dh_one<L>(C, xb.get(), yb.get(), db.get(), le != 0, out);
            for (size_t i = 0; i < kGuard; ++i)
                if (box[i] != kCanary || box[kGuard + 4 * L + i] != kCanary) return 7;
            if (memcmp(xb.get(), keep_x.data(), 4 * L) || memcmp(yb.get(), keep_y.data(), 4 * L) ||
                memcmp(db.get(), keep_d.data(), 4 * L))
                return 8;  // an input changed
            printf("%d %s\n", st, hex(out, 4 * L).c_str());
        } else {
            return 5;
        }
    }
    return 0;
}
