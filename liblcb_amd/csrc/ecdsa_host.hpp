// ecdsa_host.hpp — what the C-ABI units of the three ECDSA libraries
// (verification, signing, key agreement) share on the host: the curve table
// of ecdsa_curves.hpp parsed once per library, with the Montgomery constants
// of every curve.  Host only; internal linkage, so every library has its own.
#pragma once
#include <errno.h>
#include <stdint.h>

#include "ecdsa_curves.hpp"
#include "ecdsa_math.hpp"

namespace lcbec {
namespace {

static_assert(kEinval == EINVAL, "the kernel's EINVAL is the host's");

// The curve table parsed and its Montgomery constants derived, once.  `raw`
// is p, a, b, Gx, Gy, n as big-endian bytes (lcb_ecdsa_curve_params).
struct CurveTable {
    uint8_t raw[kCurveCount][6 * kNumBytes];
    Curve<kLimbs> c[kCurveCount];
    bool ok[kCurveCount];
    CurveTable() {
        for (int id = 0; id < kCurveCount; ++id) {
            for (int k = 0; k < 6; ++k)
                for (int i = 0; i < kNumBytes; ++i) {
                    auto nib = [](char ch) { return (uint8_t)(ch <= '9' ? ch - '0' : ch - 'a' + 10); };
                    const char* h = kCurves[id].num[k] + 2 * i;
                    raw[id][kNumBytes * k + i] = (uint8_t)(nib(h[0]) << 4 | nib(h[1]));
                }
            ok[id] = curve_setup(c[id], raw[id], kCurves[id].algo);
        }
    }
};

const CurveTable& table() {
    static const CurveTable t;
    return t;
}

bool known(int id) { return id >= 0 && id < kCurveCount && table().ok[id]; }

}  // namespace
}  // namespace lcbec
