// lcb_gost28147_gpu.cpp — exported C-ABI of the batched GOST 28147-89
// (include/lcb_gost28147_gpu.h), built into liblcb_gost28147_gpu.so and
// linked against liblcb_hash_gpu.so for the shared runtime pieces
// (ensure_init, map_err, stream-ordered scratch, parallel_copy).
//
// Device mode enqueues table upload, (ragged scan,) kernel on the caller's
// stream with stream-ordered scratch and never synchronises; key, sbox and
// the packed table travel as kernel arguments, so the caller's arrays are
// free when the call returns.  Host mode stages chunk by chunk through
// page-locked memory on a private stream: pack -> H2D -> kernel -> D2H ->
// scatter.  It is NOT pipelined (one chunk in flight); the staging context
// and the chunk size are host_stage.hpp's.  Nothing falls back to the CPU.
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/lcb_gost28147_gpu.h"
#include "../../include/lcb_hash_gpu.h"
#include "gost28147_internal.hpp"
#include "host_stage.hpp"
#include "lcb_internal.hpp"

using namespace lcbgpu;
using namespace lcbgost;

namespace {

// The six parameter sets of gost28147.h:74-139 (RFC 4357 section 11.1-11.2,
// GOST R 34.11-94 test set, TC26 "Z"), one string of 16 nibbles per row.
const char* const kSboxRows[6][8] = {
    // 0: id-GostR3411-94-TestParamSet 1.2.643.2.2.31.0
    {"4A92D80E6B1C7F53", "EB4C6DFA23810759", "581DA342EFC7609B", "7DA1089FE46CB253", "6C715FD84A9E03B2",
     "4BA0721D36859CFE", "DB413F590AE7682C", "1FD057A4923E6B8C"},
    // 1: id-Gost28147-89-CryptoPro-A-ParamSet 1.2.643.2.2.31.1
    {"96328B17A4EFC0D5", "37E98AF0526CB4D1", "E462B3D8CF5A0719", "E7ACD13902B4F856", "B5198DF0E423C7A6",
     "3ADC120B75948FE6", "1D297A608C45F3BE", "BAF50CE8623917D4"},
    // 2: id-Gost28147-89-CryptoPro-B-ParamSet 1.2.643.2.2.31.2
    {"84B135092EACD67F", "012A4D5C973FB86E", "EC0A92DB758F3614", "750DB6123ACF4E98", "27CF95AB140D68E3",
     "83264DEBC17FA095", "52AB91C374D06F8E", "04BE8371A296FD5C"},
    // 3: id-Gost28147-89-CryptoPro-C-ParamSet 1.2.643.2.2.31.3
    {"1BC29D0F458EA763", "017DB4528EFC9A63", "825049FA37CD6E1B", "36015DA8B297EFC4", "8DB0451293CE6FA7",
     "C9B18E247365A0FD", "A968DE20F35B41C7", "7405A2FEC61BD938"},
    // 4: id-Gost28147-89-CryptoPro-D-ParamSet 1.2.643.2.2.31.4
    {"FC2A645079ED1B83", "B634CFE27D805A91", "1CB0FE65AD489372", "15ECA70D62B493F8", "0C89D2AB73654EF1",
     "80F325EB1A47C9D6", "306F1E92D8C4BA57", "1A68FB04C3597D2E"},
    // 5: id-tc26-gost-28147-param-Z 1.2.643.7.1.2.5.1.1
    {"C462A5B9E8D703F1", "68239A5C1E47BD0F", "B3582FADE174C960", "C821D4F670A53E9B", "7F5A816D093EB42C",
     "5DF692CAB78143E0", "8E25691CF4B0DA37", "17ED05834FA69CB2"},
};

struct Sboxes {
    uint8_t b[6][128];
    Sboxes() {
        for (int id = 0; id < 6; ++id)
            for (int r = 0; r < 8; ++r)
                for (int c = 0; c < 16; ++c) {
                    const char ch = kSboxRows[id][r][c];
                    b[id][16 * r + c] = (uint8_t)(ch <= '9' ? ch - '0' : ch - 'A' + 10);
                }
    }
};

uint32_t rotl32(uint32_t v, int n) { return (v << n) | (v >> (32 - n)); }

// The four tables of gost28147.h:494-507 packed into one (see
// gost28147_kernels.hip); EINVAL for an sbox entry above 15.
int pack_table(const uint8_t* sbox, uint32_t* out) {
    for (int i = 0; i < 128; ++i)
        if (sbox[i] > 15) return EINVAL;
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; ++k)
            v |= ((uint32_t)sbox[32 * k + (i & 15)] | ((uint32_t)sbox[32 * k + 16 + (i >> 4)] << 4)) << (8 * k);
        out[i] = rotl32(v, 11);
    }
    return 0;
}

// Round keys in round order: gost28147.h:256-284 (ECB), 244-253 (MAC = the
// first 16 of encrypt); key words as gost28147_init / _init_be leave them.
void expand_key(const uint8_t* key, bool be, bool decrypt, uint32_t ks[32]) {
    uint32_t k[8];
    for (int i = 0; i < 8; ++i) {
        const uint8_t* p = key + 4 * i;
        k[i] = be ? ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]
                  : ((uint32_t)p[3] << 24) | ((uint32_t)p[2] << 16) | ((uint32_t)p[1] << 8) | p[0];
    }
    for (int r = 0; r < 32; ++r) {
        const bool direct = decrypt ? r < 8 : r < 24;
        ks[r] = k[direct ? (r & 7) : 7 - (r & 7)];
    }
}

struct Setup {
    GostArgs a;
    GostTable t;
};

int make_setup(Setup& su, bool be, bool decrypt, const uint8_t* key, size_t key_size, const uint8_t* sbox) {
    if (!key || !sbox || (key_size != 32 && key_size != 256)) return EINVAL;
    if (int rc = pack_table(sbox, su.t.w)) return rc;
    expand_key(key, be, decrypt, su.a.ks);
    su.a.be = be ? 1u : 0u;
    return 0;
}

// Enqueue one batch whose data pointers are on the device.  mac: a.dst holds
// the packed MACs.
int gost_enqueue(GostArgs a, const GostTable& t, bool mac, hipStream_t s) {
    if (a.count == 0) return 0;
    const bool scan = !mac && a.lengths;
    if (!mac && !a.lengths) {
        if (a.fixed_len < 8) return 0;
        a.ppb = (uint32_t)gost_pairs_of(a.fixed_len);
        a.total_pairs = a.count * a.ppb;
    }
    const uint64_t nparts = (a.count + 1023) / 1024;
    uint8_t* scratch = nullptr;
    LCB_HOST_TRY(scratch_alloc(reinterpret_cast<void**>(&scratch), 1024 + (scan ? (nparts + a.count + 1) * 8 : 0), s));
    uint32_t* dtable = reinterpret_cast<uint32_t*>(scratch);
    uint64_t* parts = reinterpret_cast<uint64_t*>(scratch + 1024);
    launch_gost_table(t, dtable, s);
    a.table = dtable;
    if (mac)
        launch_gost_mac(a, s);
    else
        launch_gost_ecb(a, nparts, scan ? parts : nullptr, scan ? parts + nparts : nullptr, s);
    hipError_t e = hipGetLastError();
    (void)scratch_free(scratch, s);
    return map_err(e);
}

// ------------------------------------------------------------ host mode
// h / d: the packed data of one chunk (the kernel runs in place).  h2 / d2:
// offsets | lengths, then MACs (8 per buffer).
size_t meta_bytes(size_t m) { return m * (8 + 4 + 8) + 16; }

thread_local HostStage g_stage;
constexpr size_t kChunkMsgs = 1u << 18;

// Overrides the staging bytes per chunk (tests force a batch across a chunk
// boundary with it).
constexpr const char* kChunkEnv = "LCB_GOST28147_CHUNK_BYTES";

int gost_host(const Setup& su, bool mac, const uint8_t* src, uint8_t* dst, const uint64_t* offsets,
              const uint32_t* lengths, size_t count, uint64_t stride, uint32_t fixed_len, size_t mac_size) {
    int dev = 0;
    LCB_HOST_TRY(hipGetDevice(&dev));
    auto off_of = [&](size_t i) -> uint64_t { return offsets ? offsets[i] : (uint64_t)i * stride; };
    // Only a buffer's whole blocks are staged: the tail is neither read nor written.
    auto used_of = [&](size_t i) -> size_t { return (size_t)((lengths ? lengths[i] : fixed_len) & ~7u); };
    size_t maxlen = fixed_len;
    if (lengths) {
        maxlen = 0;
        for (size_t i = 0; i < count; ++i) maxlen = std::max<size_t>(maxlen, lengths[i]);
    }
    // The chunk limit of THIS call (the staging buffers only ever grow).
    const size_t limit = std::max(chunk_bytes(kChunkEnv, 64), up16(maxlen));
    // Buffers per chunk: the stage's second pair is sized in bytes, so a chunk's
    // metadata has to fit meta_bytes(max_msgs).
    const size_t max_msgs = std::min(count, kChunkMsgs);
    if (int rc = g_stage.ensure(dev, limit, meta_bytes(max_msgs))) return rc;
    HostStage& S = g_stage;
    std::vector<Piece> pieces;
    size_t i = 0;
    while (i < count) {
        // Buffers [i, j), each packed at a 16-byte boundary, that fit one chunk.
        size_t j = i, total = 0;
        while (j < count && j - i < max_msgs) {
            const size_t n = up16(used_of(j));
            if (j > i && total + n > limit) break;
            total += n;
            ++j;
        }
        const size_t n = j - i;
        uint64_t* h_off = reinterpret_cast<uint64_t*>(S.h2);
        uint32_t* h_len = reinterpret_cast<uint32_t*>(S.h2 + n * 8);
        const size_t mac_at = up16(n * 12);
        pieces.clear();
        size_t pos = 0, bytes = 0;
        for (size_t k = 0; k < n; ++k) {
            const size_t u = used_of(i + k);
            if (u) pieces.push_back(Piece{S.h + pos, src + off_of(i + k), u});
            h_off[k] = pos;
            h_len[k] = (uint32_t)u;
            pos += up16(u);
            bytes += u;
        }
        parallel_copy(pieces, bytes);
        GostArgs a = su.a;
        a.count = n;
        a.src = S.d;
        a.dst = mac ? S.d2 + mac_at : S.d;
        a.mac_size = (uint32_t)mac_size;
        if (lengths) {
            a.offsets = reinterpret_cast<const uint64_t*>(S.d2);
            a.lengths = reinterpret_cast<const uint32_t*>(S.d2 + n * 8);
            LCB_HOST_TRY(hipMemcpyAsync(S.d2, S.h2, n * 12, hipMemcpyHostToDevice, S.st));
        } else {
            a.stride = up16(used_of(0));
            a.fixed_len = (uint32_t)used_of(0);
        }
        if (pos) LCB_HOST_TRY(hipMemcpyAsync(S.d, S.h, pos, hipMemcpyHostToDevice, S.st));
        if (int rc = gost_enqueue(a, su.t, mac, S.st)) return rc;
        if (mac)
            LCB_HOST_TRY(hipMemcpyAsync(S.h2 + mac_at, S.d2 + mac_at, n * mac_size, hipMemcpyDeviceToHost, S.st));
        else if (pos)
            LCB_HOST_TRY(hipMemcpyAsync(S.h, S.d, pos, hipMemcpyDeviceToHost, S.st));
        LCB_HOST_TRY(hipStreamSynchronize(S.st));
        if (mac) {
            memcpy(dst + i * mac_size, S.h2 + mac_at, n * mac_size);
        } else {
            pieces.clear();
            for (size_t k = 0; k < n; ++k)
                if (h_len[k]) pieces.push_back(Piece{dst + off_of(i + k), S.h + h_off[k], h_len[k]});
            parallel_copy(pieces, bytes);
        }
        i = j;
    }
    return 0;
}

int crypt_batch(int op, int be, bool copy_only, const uint8_t* key, size_t key_size, const uint8_t* sbox,
                const uint8_t* src, uint8_t* dst, const uint64_t* offsets, const uint32_t* lengths, size_t count,
                uint64_t stride, uint32_t fixed_len, uint32_t flags, void* stream) {
    if (flags & ~LCB_HASH_F_DEVICE) return EINVAL;
    if (op != 0 && op != 1) return EINVAL;
    Setup su;
    if (int rc = make_setup(su, be != 0, op == 1, key, key_size, sbox)) return rc;
    if (!lengths && fixed_len % 8u) return EINVAL;
    if (count == 0) return 0;
    if (!src || !dst) return EINVAL;
    if (int rc = ensure_init()) return rc;
    su.a.copy_only = copy_only ? 1u : 0u;
    if (flags & LCB_HASH_F_DEVICE) {
        su.a.src = src; su.a.dst = dst; su.a.offsets = offsets; su.a.lengths = lengths;
        su.a.count = count; su.a.stride = stride; su.a.fixed_len = fixed_len;
        return gost_enqueue(su.a, su.t, false, reinterpret_cast<hipStream_t>(stream));
    }
    return gost_host(su, false, src, dst, offsets, lengths, count, stride, fixed_len, 0);
}

}  // namespace

extern "C" {

const uint8_t* lcb_gost28147_sbox(int id) {
    static const Sboxes s;
    return (id >= 0 && id < 6) ? s.b[id] : nullptr;
}

int lcb_gost28147_gpu_table(const uint8_t* sbox, uint32_t* out) {
    if (!sbox || !out) return EINVAL;
    return pack_table(sbox, out);
}

int lcb_gost28147_crypt_batch(int op, int be, const uint8_t* key, size_t key_size, const uint8_t* sbox,
                              const uint8_t* src, uint8_t* dst, const uint64_t* offsets, const uint32_t* lengths,
                              size_t count, uint64_t stride, uint32_t fixed_len, uint32_t flags, void* stream) {
    return crypt_batch(op, be, false, key, key_size, sbox, src, dst, offsets, lengths, count, stride, fixed_len,
                       flags, stream);
}

int lcb_gost28147_gpu_copy_probe(const uint8_t* src, uint8_t* dst, const uint64_t* offsets, const uint32_t* lengths,
                                 size_t count, uint64_t stride, uint32_t fixed_len, uint32_t flags, void* stream) {
    static const uint8_t zero_key[32] = {};
    return crypt_batch(0, 0, true, zero_key, 32, lcb_gost28147_sbox(0), src, dst, offsets, lengths, count, stride,
                       fixed_len, flags, stream);
}

int lcb_gost28147_mac_batch(int be, const uint8_t* key, size_t key_size, const uint8_t* sbox, const uint8_t* data,
                            const uint64_t* offsets, const uint32_t* lengths, size_t count, uint64_t stride,
                            uint32_t fixed_len, uint8_t* macs, size_t mac_size, uint32_t flags, void* stream) {
    if (flags & ~LCB_HASH_F_DEVICE) return EINVAL;
    if (mac_size < 1 || mac_size > 8) return EINVAL;
    Setup su;
    if (int rc = make_setup(su, be != 0, false, key, key_size, sbox)) return rc;
    if (!lengths && fixed_len % 8u) return EINVAL;
    if (count == 0) return 0;
    if (!data || !macs) return EINVAL;
    if (int rc = ensure_init()) return rc;
    if (flags & LCB_HASH_F_DEVICE) {
        su.a.src = data; su.a.dst = macs; su.a.offsets = offsets; su.a.lengths = lengths;
        su.a.count = count; su.a.stride = stride; su.a.fixed_len = fixed_len;
        su.a.mac_size = (uint32_t)mac_size;
        return gost_enqueue(su.a, su.t, true, reinterpret_cast<hipStream_t>(stream));
    }
    return gost_host(su, true, data, macs, offsets, lengths, count, stride, fixed_len, mac_size);
}

#define GOST_ECB_WRAPPER(name, op, be)                                                                          \
    int name(const uint8_t* key, size_t key_size, const uint8_t* sbox, const uint8_t* src, uint8_t* dst,       \
             const uint64_t* offsets, const uint32_t* lengths, size_t count, uint64_t stride,                   \
             uint32_t fixed_len, uint32_t flags, void* stream) {                                                \
        return lcb_gost28147_crypt_batch(op, be, key, key_size, sbox, src, dst, offsets, lengths, count,        \
                                         stride, fixed_len, flags, stream);                                     \
    }
GOST_ECB_WRAPPER(gost28147_blocks_encrypt_batch, 0, 0)
GOST_ECB_WRAPPER(gost28147_blocks_encrypt_be_batch, 0, 1)
GOST_ECB_WRAPPER(gost28147_blocks_decrypt_batch, 1, 0)
GOST_ECB_WRAPPER(gost28147_blocks_decrypt_be_batch, 1, 1)
#undef GOST_ECB_WRAPPER

int gost28147_blocks_mac_batch(const uint8_t* key, size_t key_size, const uint8_t* sbox, const uint8_t* data,
                               const uint64_t* offsets, const uint32_t* lengths, size_t count, uint64_t stride,
                               uint32_t fixed_len, uint8_t* macs, size_t mac_size, uint32_t flags, void* stream) {
    return lcb_gost28147_mac_batch(0, key, key_size, sbox, data, offsets, lengths, count, stride, fixed_len, macs,
                                   mac_size, flags, stream);
}

int gost28147_blocks_mac_be_batch(const uint8_t* key, size_t key_size, const uint8_t* sbox, const uint8_t* data,
                                  const uint64_t* offsets, const uint32_t* lengths, size_t count, uint64_t stride,
                                  uint32_t fixed_len, uint8_t* macs, size_t mac_size, uint32_t flags,
                                  void* stream) {
    return lcb_gost28147_mac_batch(1, key, key_size, sbox, data, offsets, lengths, count, stride, fixed_len, macs,
                                   mac_size, flags, stream);
}

}  // extern "C"
