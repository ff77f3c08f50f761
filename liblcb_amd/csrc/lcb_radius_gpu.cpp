// lcb_radius_gpu.cpp — exported C-ABI of the batched RADIUS sign/verify
// (include/lcb_radius_gpu.h), built into liblcb_radius_gpu.so and linked
// against liblcb_hash_gpu.so for the shared runtime pieces (ensure_init,
// map_err, stream-ordered scratch, parallel_copy) and the keyed MD5 batches
// (lcb_hash_batch_keyed).
//
// One call is a fixed sequence on one stream, the same for every batch, so
// nothing is read back to decide what runs next:
//
//   sign    parse -> password encode (+ zero the Message-Authenticator)
//           -> HMAC pass -> store it -> suffix pass -> store the authenticator
//   verify  parse (+ substitute for the HMAC pass) -> HMAC pass -> compare,
//           restore, substitute for the suffix pass -> suffix pass -> compare,
//           restore, merge errors -> password decode
//
// Both keyed passes run over all `count` packets with a device-written length
// array that is 0 for a packet not in that pass.  Host mode stages chunk by
// chunk through page-locked memory on a private stream (the staging context
// and the chunk size are host_stage.hpp's) and runs the same sequence; it is
// NOT pipelined.  Nothing falls back to the CPU.
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/lcb_hash_gpu.h"
#include "../../include/lcb_radius_gpu.h"
#include "host_stage.hpp"
#include "lcb_internal.hpp"
#include "radius_internal.hpp"

using namespace lcbgpu;
using namespace lcbrad;

namespace {

// The caller's key table (host memory), checked once per call.
struct KeyTab {
    const uint8_t* keys;
    const uint64_t* key_offsets;
    const uint32_t* key_lengths;
    size_t nkeys;
    size_t total = 0;  // key bytes
};

int key_tab_check(KeyTab& kt) {
    if (!kt.keys || !kt.key_lengths || kt.nkeys == 0 || kt.nkeys > UINT32_MAX) return EINVAL;
    uint64_t total = 0;
    for (size_t k = 0; k < kt.nkeys; ++k) {
        total += kt.key_lengths[k];
        if (total > UINT32_MAX) return EINVAL;
    }
    kt.total = (size_t)total;
    return 0;
}

void wipe(std::vector<uint8_t>& v) {
    volatile uint8_t* p = v.data();
    for (size_t i = 0; i < v.size(); ++i) p[i] = 0;
}

// One batch whose packet pointers are on the device, enqueued on `s`.
int rad_enqueue(RadArgs a, bool sign, const KeyTab& kt, hipStream_t s) {
    const size_t n = a.count;
    // [rec | park | dig | len_ma | len_au | kidx | key bytes | key_off | key_len]
    const size_t side_b = n * (sizeof(RadRec) + 32 + 16) + up16(n * 12);
    const size_t blob_b = up16(kt.total + 4), tab_b = up16(kt.nkeys * 4);
    const size_t key_b = blob_b + 2 * tab_b;
    uint8_t* d = nullptr;
    LCB_HOST_TRY(scratch_alloc(reinterpret_cast<void**>(&d), side_b + key_b, s));
    a.rec = reinterpret_cast<RadRec*>(d);
    a.park = reinterpret_cast<uint4*>(d + n * sizeof(RadRec));
    a.dig = a.park + 2 * n;
    a.len_ma = reinterpret_cast<uint32_t*>(a.dig + n);
    a.len_au = a.len_ma + n;
    a.kidx = a.len_au + n;
    uint8_t* dkeys = d + side_b;
    a.keys = dkeys;
    a.key_off = reinterpret_cast<const uint32_t*>(dkeys + blob_b);
    a.key_len = reinterpret_cast<const uint32_t*>(dkeys + blob_b + tab_b);
    a.nkeys = (uint32_t)kt.nkeys;

    // The password kernel's key table: one host image, one copy.  Pageable
    // source: the copy returns once the bytes are staged.
    std::vector<uint8_t> img(key_b, 0);
    uint32_t* koff = reinterpret_cast<uint32_t*>(img.data() + blob_b);
    uint32_t* klen = reinterpret_cast<uint32_t*>(img.data() + blob_b + tab_b);
    uint32_t at = 0;
    for (size_t k = 0; k < kt.nkeys; ++k) {
        koff[k] = at;
        klen[k] = kt.key_lengths[k];
        if (klen[k]) memcpy(img.data() + at, kt.keys + (kt.key_offsets ? kt.key_offsets[k] : 0), klen[k]);
        at += klen[k];
    }
    hipError_t e = hipMemcpyAsync(dkeys, img.data(), key_b, hipMemcpyHostToDevice, s);
    wipe(img);

    int rc = map_err(e);
    bool parsed = false;
    auto keyed = [&](int mode, const uint32_t* lengths) {
        return lcb_hash_batch_keyed(LCB_HASH_MD5, mode, kt.keys, kt.key_offsets, kt.key_lengths, kt.nkeys,
                                    kt.nkeys == 1 ? nullptr : a.kidx, a.pkts, a.offsets, lengths, n, a.stride, 0,
                                    reinterpret_cast<uint8_t*>(a.dig), LCB_HASH_F_DEVICE, s);
    };
    auto launched = [&]() { return map_err(hipGetLastError()); };
    if (!rc) {
        launch_radius_parse(a, sign, s);
        rc = launched();
        parsed = !rc;
    }
    if (!rc && sign) {
        launch_radius_password(a, true, s);
        rc = launched();
    }
    if (!rc) rc = keyed(LCB_HASH_KEY_HMAC, a.len_ma);
    if (!rc || (parsed && !sign)) {  // a failed verify still puts the substituted fields back
        launch_radius_mid(a, sign, s);
        const int r2 = launched();
        if (!rc) rc = r2;
    }
    if (!rc) rc = keyed(LCB_HASH_KEY_SUFFIX, a.len_au);
    if (!rc || (parsed && !sign)) {
        launch_radius_fin(a, sign, s);
        const int r2 = launched();
        if (!rc) rc = r2;
    }
    if (!rc && !sign) {
        launch_radius_password(a, false, s);
        rc = launched();
    }
    // The call's copy of the secrets is zeroed before the buffer goes back.
    (void)hipMemsetAsync(dkeys, 0, key_b, s);
    (void)scratch_free(d, s);
    return rc;
}

// ------------------------------------------------------------ host mode
// h / d: the packed packets of one chunk.  h2 / d2: offsets | buf_sizes |
// key_index | errors | req_hdrs.
size_t meta_bytes(size_t m) { return m * (8 + 4 + 4 + 4 + 20) + 16; }

thread_local HostStage g_stage;
constexpr size_t kChunkMsgs = 1u << 18;

// Overrides the staging bytes per chunk (tests force a batch across a chunk
// boundary with it).
constexpr const char* kChunkEnv = "LCB_RADIUS_CHUNK_BYTES";

// The bytes of a host packet buffer that are staged: [0, Length) where the
// header can be read and Length fits, else just enough for the device guard
// to reach the verdict the whole buffer would get.
uint32_t staged_size(const uint8_t* p, uint32_t buf_size) {
    if (buf_size < kHdrSize) return std::min<uint32_t>(buf_size, 4u);  // EBADMSG either way; a short header is not read
    const uint32_t len = ((uint32_t)p[2] << 8) | p[3];
    if (len < kHdrSize) return 4;   // EBADMSG as a 4-byte buffer
    if (len > buf_size || len > kPktMax) return kHdrSize;  // still longer than the 20 staged bytes
    return len;
}

int rad_host(RadArgs u, bool sign, const KeyTab& kt) {
    int dev = 0;
    LCB_HOST_TRY(hipGetDevice(&dev));
    const size_t count = u.count;
    auto off_of = [&](size_t i) -> uint64_t { return u.offsets ? u.offsets[i] : (uint64_t)i * u.stride; };
    auto size_of = [&](size_t i) -> uint32_t { return u.buf_sizes ? u.buf_sizes[i] : u.fixed_size; };
    // The chunk limit of THIS call (the staging buffers only ever grow).
    const size_t limit =
        std::max<size_t>(std::min<uint64_t>(chunk_bytes(kChunkEnv, kPktMax), (uint64_t)count * kPktMax), kPktMax);
    // Packets per chunk: the stage's second pair is sized in bytes, so a chunk's
    // metadata has to fit meta_bytes(max_msgs).
    const size_t max_msgs = std::min(count, kChunkMsgs);
    if (int rc = g_stage.ensure(dev, limit, meta_bytes(max_msgs))) return rc;
    HostStage& S = g_stage;
    std::vector<Piece> pieces;
    std::vector<uint32_t> msz;  // staged bytes of the chunk's packets
    size_t i = 0;
    while (i < count) {
        // Packets [i, j), each packed at a 16-byte boundary, that fit one chunk.
        uint64_t* h_off = reinterpret_cast<uint64_t*>(S.h2);
        size_t j = i, pos = 0, bytes = 0;
        pieces.clear();
        msz.clear();
        while (j < count && j - i < max_msgs) {
            const uint32_t m = staged_size(u.pkts + off_of(j), size_of(j));
            if (j > i && pos + up16(m) > limit) break;
            h_off[j - i] = pos;
            msz.push_back(m);
            if (m) pieces.push_back(Piece{S.h + pos, u.pkts + off_of(j), m});
            pos += up16(m);
            bytes += m;
            ++j;
        }
        const size_t n = j - i;
        uint32_t* h_size = reinterpret_cast<uint32_t*>(S.h2 + n * 8);
        uint32_t* h_kidx = h_size + n;
        int32_t* h_err = reinterpret_cast<int32_t*>(h_kidx + n);
        uint8_t* h_req = reinterpret_cast<uint8_t*>(h_err + n);
        memcpy(h_size, msz.data(), n * 4);
        if (u.key_index) memcpy(h_kidx, u.key_index + i, n * 4);
        if (u.req_hdrs) memcpy(h_req, u.req_hdrs + 20 * i, n * 20);
        parallel_copy(pieces, bytes);
        RadArgs a;
        a.count = n;
        a.pkts = S.d;
        a.offsets = reinterpret_cast<const uint64_t*>(S.d2);
        a.buf_sizes = reinterpret_cast<const uint32_t*>(S.d2 + n * 8);
        a.key_index = u.key_index ? reinterpret_cast<const uint32_t*>(S.d2 + n * 12) : nullptr;
        a.errors = reinterpret_cast<int32_t*>(S.d2 + n * 16);
        a.req_hdrs = u.req_hdrs ? S.d2 + n * 20 : nullptr;
        LCB_HOST_TRY(hipMemcpyAsync(S.d2, S.h2, n * 40, hipMemcpyHostToDevice, S.st));
        if (pos) LCB_HOST_TRY(hipMemcpyAsync(S.d, S.h, pos, hipMemcpyHostToDevice, S.st));
        if (int rc = rad_enqueue(a, sign, kt, S.st)) {
            (void)hipStreamSynchronize(S.st);
            return rc;
        }
        LCB_HOST_TRY(hipMemcpyAsync(h_err, S.d2 + n * 16, n * 4, hipMemcpyDeviceToHost, S.st));
        if (pos) LCB_HOST_TRY(hipMemcpyAsync(S.h, S.d, pos, hipMemcpyDeviceToHost, S.st));
        LCB_HOST_TRY(hipStreamSynchronize(S.st));
        // Only [0, Length) of the packets that may have changed goes back.
        pieces.clear();
        bytes = 0;
        for (size_t k = 0; k < n; ++k) {
            u.errors[i + k] = h_err[k];
            if (h_err[k] == 0 && h_size[k]) {
                pieces.push_back(Piece{u.pkts + off_of(i + k), S.h + h_off[k], h_size[k]});
                bytes += h_size[k];
            }
        }
        parallel_copy(pieces, bytes);
        i = j;
    }
    return 0;
}

int rad_batch(bool sign, uint8_t* pkts, const uint64_t* offsets, const uint32_t* buf_sizes, size_t count,
              uint64_t stride, uint32_t fixed_size, const uint8_t* keys, const uint64_t* key_offsets,
              const uint32_t* key_lengths, size_t nkeys, const uint32_t* key_index, const uint8_t* req_hdrs,
              int32_t* errors, uint32_t flags, void* stream) {
    if (flags & ~LCB_HASH_F_DEVICE) return EINVAL;
    KeyTab kt{keys, key_offsets, key_lengths, nkeys};
    if (int rc = key_tab_check(kt)) return rc;
    if (!buf_sizes && fixed_size < kHdrSize) return EINVAL;
    if (!offsets && stride < fixed_size && count > 1) return EINVAL;
    if (count == 0) return 0;
    if (!pkts || !errors) return EINVAL;
    if (int rc = ensure_init()) return rc;
    RadArgs a;
    a.pkts = pkts; a.offsets = offsets; a.buf_sizes = buf_sizes; a.count = count; a.stride = stride;
    a.fixed_size = fixed_size; a.key_index = key_index; a.req_hdrs = sign ? nullptr : req_hdrs; a.errors = errors;
    if (flags & LCB_HASH_F_DEVICE) return rad_enqueue(a, sign, kt, reinterpret_cast<hipStream_t>(stream));
    return rad_host(a, sign, kt);
}

}  // namespace

extern "C" {

int radius_pkt_sign_batch(uint8_t* pkts, const uint64_t* offsets, const uint32_t* buf_sizes, size_t count,
                          uint64_t stride, uint32_t fixed_size, const uint8_t* keys, const uint64_t* key_offsets,
                          const uint32_t* key_lengths, size_t nkeys, const uint32_t* key_index, int32_t* errors,
                          uint32_t flags, void* stream) {
    return rad_batch(true, pkts, offsets, buf_sizes, count, stride, fixed_size, keys, key_offsets, key_lengths, nkeys,
                     key_index, nullptr, errors, flags, stream);
}

int radius_pkt_verify_batch(uint8_t* pkts, const uint64_t* offsets, const uint32_t* buf_sizes, size_t count,
                            uint64_t stride, uint32_t fixed_size, const uint8_t* keys, const uint64_t* key_offsets,
                            const uint32_t* key_lengths, size_t nkeys, const uint32_t* key_index,
                            const uint8_t* req_hdrs, int32_t* errors, uint32_t flags, void* stream) {
    return rad_batch(false, pkts, offsets, buf_sizes, count, stride, fixed_size, keys, key_offsets, key_lengths,
                     nkeys, key_index, req_hdrs, errors, flags, stream);
}

}  // extern "C"
