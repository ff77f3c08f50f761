// radius_internal.hpp — types shared by the kernel TU and the C-ABI TU of
// liblcb_radius_gpu.so (include/lcb_radius_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "radius_parse.hpp"

namespace lcbrad {

// Device-side description of one RADIUS batch and its per-call side arrays
// (all `count` long; see rad_side_bytes for their layout in one allocation).
struct RadArgs {
    uint8_t* pkts = nullptr;
    const uint64_t* offsets = nullptr;    // nullptr: i * stride
    const uint32_t* buf_sizes = nullptr;  // nullptr: fixed_size
    uint64_t count = 0, stride = 0;
    uint32_t fixed_size = 0;
    uint32_t nkeys = 0;
    const uint32_t* key_index = nullptr;  // the caller's, nullptr: key 0
    const uint8_t* req_hdrs = nullptr;    // verify: count x 20, nullptr: no request
    int32_t* errors = nullptr;
    // side arrays
    RadRec* rec = nullptr;
    uint4* park = nullptr;     // verify: 2 per packet, the original authenticator and Message-Authenticator
    uint4* dig = nullptr;      // the digests of the keyed pass in flight
    uint32_t* len_ma = nullptr;  // lengths of the HMAC pass: Length, or 0 for a packet not in it
    uint32_t* len_au = nullptr;  // lengths of the suffix pass
    uint32_t* kidx = nullptr;    // key index of every packet, always < nkeys
    // the call's own key table (password kernel)
    const uint8_t* keys = nullptr;
    const uint32_t* key_off = nullptr;
    const uint32_t* key_len = nullptr;
};

void launch_radius_parse(const RadArgs& a, bool sign, hipStream_t s);
// sign: zero the Message-Authenticator and run the encode chain (before the
// HMAC pass); verify: decode where errors[i] == 0 (after the last step).
void launch_radius_password(const RadArgs& a, bool sign, hipStream_t s);
void launch_radius_mid(const RadArgs& a, bool sign, hipStream_t s);  // between the HMAC and the suffix pass
void launch_radius_fin(const RadArgs& a, bool sign, hipStream_t s);  // after the suffix pass: writes errors

}  // namespace lcbrad
