// ecdsa_sign_internal.hpp — types shared by the kernel TU and the C-ABI TU of
// liblcb_ecdsa_sign_gpu.so (include/lcb_ecdsa_sign_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ecdsa_sign_args.hpp"
#include "ecdsa_sign_math.hpp"

namespace lcbec {

typedef BaseTable<kLimbs> Table;

// The per-curve constant block travels as a kernel argument (scalar loads);
// `t` is the curve's window table in device memory.
void launch_ecdsa_sign(const SignArgs& a, const Curve<kLimbs>& c, const Table* t, hipStream_t s);
void launch_ecdsa_keys(const KeyArgs& a, const Curve<kLimbs>& c, const Table* t, hipStream_t s);

}  // namespace lcbec
