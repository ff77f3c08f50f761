// stream_state.hpp — host-only: the device context layout of a stream set
// (include/lcb_hash_stream_gpu.h), the validation of an imported record and
// the mapping record <-> context words.  No HIP here, so it builds and runs
// stand-alone (tests/c/stream_state_host.cpp, under the sanitizers).
//
// A context is kWords(alg) uint32 words, stored word-major on the device:
// word k of stream s at ctx[k * pitch + s].
//
//   MD5 / SHA            GOST R 34.11-2012
//   [ 0, 16)  h          [ 0, 16)  h
//   [16, 18)  count      [16, 32)  N
//   [18, 20)  count_hi   [32, 48)  Sigma
//   [20, 52)  buf        [48]      used
//                        [49, 65)  buf
//
// h, N, Sigma and buf are the little-endian memory images of the reference
// context's fields; bytes of buf at or past `used` are zero.  The MD family
// keeps no `used`: it is count % block, as in the reference.
#pragma once
#include <errno.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/lcb_hash_stream_gpu.h"

namespace lcbstream {

enum : uint32_t {
    kMdH = 0, kMdCount = 16, kMdCountHi = 18, kMdBuf = 20, kMdWords = 52,
    kGoH = 0, kGoN = 16, kGoSigma = 32, kGoUsed = 48, kGoBuf = 49, kGoWords = 65,
    kMaxWords = 65
};

inline bool alg_valid(int alg) { return alg >= LCB_HASH_MD5 && alg <= LCB_HASH_GOST512; }
inline bool alg_gost(int alg) { return alg == LCB_HASH_GOST256 || alg == LCB_HASH_GOST512; }
inline uint32_t alg_block(int alg) { return (alg == LCB_HASH_SHA384 || alg == LCB_HASH_SHA512) ? 128u : 64u; }
inline uint32_t alg_words(int alg) { return alg_gost(alg) ? kGoWords : kMdWords; }
// Bytes of `h` the algorithm uses (the reference ctx's state words).
inline uint32_t alg_state_bytes(int alg) {
    switch (alg) {
    case LCB_HASH_MD5: return 16;
    case LCB_HASH_SHA1: return 20;
    case LCB_HASH_SHA224:
    case LCB_HASH_SHA256: return 32;
    default: return 64;
    }
}

// 0, or EINVAL for a record a set of `alg` must refuse: another algorithm,
// used >= block, or (MD5 / SHA) used != count % block.
inline int state_check(int alg, const lcb_hash_stream_state_t& r) {
    if (!alg_valid(alg) || r.alg != (uint32_t)alg) return EINVAL;
    const uint32_t B = alg_block(alg);
    if (r.used >= B) return EINVAL;
    if (!alg_gost(alg) && r.used != (uint32_t)(r.count & (B - 1))) return EINVAL;
    return 0;
}

inline uint32_t le32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
inline void put_le32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

// The context words of a checked record; w: alg_words(alg) words.  Bytes of
// r.buf at or past r.used and h bytes the algorithm does not use are dropped.
inline void state_to_words(int alg, const lcb_hash_stream_state_t& r, uint32_t* w) {
    const uint32_t B = alg_block(alg), nw = alg_words(alg);
    for (uint32_t k = 0; k < nw; ++k) w[k] = 0;
    const uint32_t hb = alg_state_bytes(alg);
    for (uint32_t k = 0; k < hb / 4; ++k) w[k] = le32(r.h + 4 * k);
    uint8_t buf[128] = {0};
    memcpy(buf, r.buf, r.used);
    const uint32_t at = alg_gost(alg) ? kGoBuf : kMdBuf;
    for (uint32_t k = 0; k < B / 4; ++k) w[at + k] = le32(buf + 4 * k);
    if (alg_gost(alg)) {
        for (uint32_t k = 0; k < 16; ++k) {
            w[kGoN + k] = le32(r.n + 4 * k);
            w[kGoSigma + k] = le32(r.sigma + 4 * k);
        }
        w[kGoUsed] = r.used;
    } else {
        w[kMdCount] = (uint32_t)r.count;
        w[kMdCount + 1] = (uint32_t)(r.count >> 32);
        if (B == 128) {
            w[kMdCountHi] = (uint32_t)r.count_hi;
            w[kMdCountHi + 1] = (uint32_t)(r.count_hi >> 32);
        }
    }
}

// The record of a context's words.
inline void words_to_state(int alg, const uint32_t* w, lcb_hash_stream_state_t& r) {
    const uint32_t B = alg_block(alg);
    memset(&r, 0, sizeof(r));
    r.alg = (uint32_t)alg;
    const uint32_t hb = alg_state_bytes(alg);
    for (uint32_t k = 0; k < hb / 4; ++k) put_le32(r.h + 4 * k, w[k]);
    const uint32_t at = alg_gost(alg) ? kGoBuf : kMdBuf;
    if (alg_gost(alg)) {
        for (uint32_t k = 0; k < 16; ++k) {
            put_le32(r.n + 4 * k, w[kGoN + k]);
            put_le32(r.sigma + 4 * k, w[kGoSigma + k]);
        }
        r.used = w[kGoUsed] & 63u;
        const uint64_t n0 = (uint64_t)w[kGoN] | ((uint64_t)w[kGoN + 1] << 32);
        const uint64_t n1 = (uint64_t)w[kGoN + 2] | ((uint64_t)w[kGoN + 3] << 32);
        r.count = ((n0 >> 3) | (n1 << 61)) + r.used;   // N / 8 + used, low 64 bits
    } else {
        r.count = (uint64_t)w[kMdCount] | ((uint64_t)w[kMdCount + 1] << 32);
        r.count_hi = (uint64_t)w[kMdCountHi] | ((uint64_t)w[kMdCountHi + 1] << 32);
        r.used = (uint32_t)(r.count & (B - 1));
    }
    uint8_t buf[128];
    for (uint32_t k = 0; k < B / 4; ++k) put_le32(buf + 4 * k, w[at + k]);
    memcpy(r.buf, buf, r.used);
}

// 0, or EINVAL when a list of `count` stream indices (nullptr: 0 .. count-1)
// holds one >= nstreams or one twice.  seen: nstreams bytes of zeroes,
// zeroes again on return.
inline int index_check(const uint32_t* idx, size_t count, size_t nstreams, uint8_t* seen) {
    if (!idx) return count > nstreams ? EINVAL : 0;
    int rc = 0;
    size_t i = 0;
    for (; i < count; ++i) {
        if (idx[i] >= nstreams || seen[idx[i]]) { rc = EINVAL; break; }
        seen[idx[i]] = 1;
    }
    for (size_t k = 0; k < i; ++k) seen[idx[k]] = 0;
    return rc;
}

}  // namespace lcbstream
