// gost28147_internal.hpp — types shared by the kernel TU and the C-ABI TU of
// liblcb_gost28147_gpu.so (include/lcb_gost28147_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lcbgost {

// Device-side description of one GOST 28147-89 batch.
struct GostArgs {
    const uint8_t* src = nullptr;          // ECB input / MAC data
    uint8_t* dst = nullptr;                // ECB output / packed MACs
    const uint64_t* offsets = nullptr;     // nullptr: i * stride
    const uint32_t* lengths = nullptr;     // nullptr: fixed_len
    const uint64_t* pair_start = nullptr;  // ragged ECB: exclusive prefix of block pairs (count + 1)
    const uint32_t* table = nullptr;       // the 256 packed sbox words (device)
    uint64_t count = 0, stride = 0;
    uint64_t total_pairs = 0;              // fixed layout: count * ppb
    uint32_t fixed_len = 0, ppb = 1;       // ppb: 16-byte block pairs per buffer, the last may be half
    uint32_t be = 0;                       // the reference's *_be load/store byte order
    uint32_t copy_only = 0;                // measurement aid: skip the rounds
    uint32_t mac_size = 8;
    uint32_t ks[32] = {};                  // key words in round order (the MAC uses the first 16)
};

// The packed table travels to the device as a kernel argument, so the
// caller's sbox is free the moment the launch returns.
struct GostTable {
    uint32_t w[256];
};

// Block pairs of a buffer of `len` bytes: blocks_count = len / 8 (integer).
__host__ __device__ inline uint64_t gost_pairs_of(uint32_t len) { return ((uint64_t)(len >> 3) + 1u) >> 1; }

void launch_gost_table(const GostTable& t, uint32_t* dtable, hipStream_t s);
// Ragged batches: scan (parts: (count+1023)/1024 words, pair_start: count+1),
// then the block kernel.
void launch_gost_ecb(const GostArgs& a, uint64_t nparts, uint64_t* parts, uint64_t* pair_start, hipStream_t s);
void launch_gost_mac(const GostArgs& a, hipStream_t s);

}  // namespace lcbgost
