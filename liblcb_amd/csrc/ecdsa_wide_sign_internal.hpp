// ecdsa_wide_sign_internal.hpp — types shared by the kernel TU and the C-ABI
// TU of liblcb_ecdsa_wide_sign_gpu.so (include/lcb_ecdsa_wide_sign_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ecdsa_sign_args.hpp"
#include "ecdsa_sign_math.hpp"

namespace lcbec {

constexpr int kLimbs384 = 12, kLimbs512 = 16;

// One sign and one keys kernel per limb count.  The per-curve constant block
// travels as a kernel argument (scalar loads); `t` is the curve's window
// table in device memory.
void launch_ecdsa_wide_sign(const SignArgs& a, const Curve<kLimbs384>& c, const BaseTable<kLimbs384>* t,
                            hipStream_t s);
void launch_ecdsa_wide_sign(const SignArgs& a, const Curve<kLimbs512>& c, const BaseTable<kLimbs512>* t,
                            hipStream_t s);
void launch_ecdsa_wide_keys(const KeyArgs& a, const Curve<kLimbs384>& c, const BaseTable<kLimbs384>* t,
                            hipStream_t s);
void launch_ecdsa_wide_keys(const KeyArgs& a, const Curve<kLimbs512>& c, const BaseTable<kLimbs512>* t,
                            hipStream_t s);

}  // namespace lcbec
