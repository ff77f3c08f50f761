// ecdsa_wide_host.hpp — the curve table of ecdsa_wide_curves.hpp parsed once,
// with the Montgomery constants of every curve at its own limb count (12 or
// 16), for the C-ABI unit of liblcb_ecdsa_wide_gpu.so and the host test.
// Host only; internal linkage.
#pragma once
#include <errno.h>
#include <stdint.h>

#include "ecdsa_math.hpp"
#include "ecdsa_wide_curves.hpp"

namespace lcbec {
namespace {

static_assert(kEinval == EINVAL, "the kernel's EINVAL is the host's");

constexpr int kWideMaxBytes = 64;

// `raw` is p, a, b, Gx, Gy, n as 6 x B big-endian bytes
// (lcb_ecdsa_wide_curve_params); a curve has its block in c12 or in c16.
struct WideCurveTable {
    uint8_t raw[kWideCurveCount][6 * kWideMaxBytes];
    Curve<12> c12[kWideCurveCount];
    Curve<16> c16[kWideCurveCount];
    bool ok[kWideCurveCount];
    WideCurveTable() {
        for (int id = 0; id < kWideCurveCount; ++id) {
            const uint32_t B = kWideCurves[id].bytes;
            for (int k = 0; k < 6; ++k)
                for (uint32_t i = 0; i < B; ++i) {
                    auto nib = [](char ch) { return (uint8_t)(ch <= '9' ? ch - '0' : ch - 'a' + 10); };
                    const char* h = kWideCurves[id].num[k] + 2 * i;
                    raw[id][B * k + i] = (uint8_t)(nib(h[0]) << 4 | nib(h[1]));
                }
            ok[id] = B == 48   ? curve_setup(c12[id], raw[id], kWideCurves[id].algo)
                     : B == 64 ? curve_setup(c16[id], raw[id], kWideCurves[id].algo)
                               : false;
        }
    }
};

const WideCurveTable& wide_table() {
    static const WideCurveTable t;
    return t;
}

bool wide_known(int id) { return id >= 0 && id < kWideCurveCount && wide_table().ok[id]; }

}  // namespace
}  // namespace lcbec
