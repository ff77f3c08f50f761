// ecdsa_key_internal.hpp — types shared by the kernel TU and the C-ABI TU of
// liblcb_ecdsa_key_gpu.so (include/lcb_ecdsa_key_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ecdsa_key_math.hpp"

namespace lcbec {

// Device-side description of one import batch.
struct KeyImportArgs {
    const uint8_t* keys = nullptr;     // item i at keys + i * key_stride
    const uint32_t* sizes = nullptr;   // nullptr: every item key_size
    const uint8_t* keys_y = nullptr;   // nullptr, or count x kNumBytes
    uint8_t* pub = nullptr;            // count x 2 kNumBytes: x || y
    uint8_t* infinity = nullptr;       // nullptr, or count
    int32_t* status = nullptr;         // count
    uint64_t count = 0, key_stride = 0;
    uint32_t key_size = 0, le = 0;
};

// Device-side description of one export batch.
struct KeyExportArgs {
    const uint8_t* pub = nullptr;       // count x 2 kNumBytes: x || y
    const uint8_t* infinity = nullptr;  // nullptr: no item is the point at infinity
    uint8_t* out = nullptr;             // item i at out + i * out_stride
    uint32_t* out_sizes = nullptr;      // count
    int32_t* status = nullptr;          // count
    uint64_t count = 0, out_stride = 0;
    uint32_t compress = 0, le = 0;
};

// The per-curve constant blocks travel as kernel arguments (scalar loads).
void launch_ecdsa_key_import(const KeyImportArgs& a, const Curve<kLimbs>& c, const KeyConsts<kLimbs>& k,
                             hipStream_t s);
void launch_ecdsa_key_export(const KeyExportArgs& a, hipStream_t s);

}  // namespace lcbec
