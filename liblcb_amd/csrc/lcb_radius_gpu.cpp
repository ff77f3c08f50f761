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
// chunk through page-locked memory on a private stream and runs the same
// sequence; it is NOT pipelined.  Nothing falls back to the CPU.
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/lcb_hash_gpu.h"
#include "../../include/lcb_radius_gpu.h"
#include "lcb_internal.hpp"
#include "radius_internal.hpp"

using namespace lcbgpu;
using namespace lcbrad;

namespace {

#define RAD_TRY(expr)                             \
    do {                                          \
        hipError_t _e = (expr);                   \
        if (_e != hipSuccess) return map_err(_e); \
    } while (0)

size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

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
    RAD_TRY(scratch_alloc(reinterpret_cast<void**>(&d), side_b + key_b, s));
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
struct RadStage {
    int device = -1;
    size_t cap = 0, mcap = 0;  // packet bytes / packets per chunk
    hipStream_t st = nullptr;
    uint8_t *h_data = nullptr, *d_data = nullptr;
    uint8_t *h_meta = nullptr, *d_meta = nullptr;  // offsets | buf_sizes | key_index | errors | req_hdrs

    static size_t meta_bytes(size_t m) { return m * (8 + 4 + 4 + 4 + 20) + 16; }

    void release() {
        if (h_data) (void)hipHostFree(h_data);
        if (h_meta) (void)hipHostFree(h_meta);
        if (d_data) (void)hipFree(d_data);
        if (d_meta) (void)hipFree(d_meta);
        if (st) (void)hipStreamDestroy(st);
        h_data = h_meta = d_data = d_meta = nullptr;
        st = nullptr;
        cap = mcap = 0;
        device = -1;
    }
    ~RadStage() { release(); }

    int ensure(int dev, size_t need_bytes, size_t need_msgs) {
        if (device == dev && cap >= need_bytes && mcap >= need_msgs) return 0;
        const size_t nb = std::max(need_bytes, cap), nm = std::max(need_msgs, mcap);
        release();
        device = dev;
        RAD_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        RAD_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_data), nb, hipHostMallocDefault));
        RAD_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_meta), meta_bytes(nm), hipHostMallocDefault));
        RAD_TRY(hipMalloc(reinterpret_cast<void**>(&d_data), nb));
        RAD_TRY(hipMalloc(reinterpret_cast<void**>(&d_meta), meta_bytes(nm)));
        cap = nb;
        mcap = nm;
        return 0;
    }
};

thread_local RadStage g_stage;
constexpr size_t kChunkMsgs = 1u << 18;

// Staging bytes per chunk; LCB_RADIUS_CHUNK_BYTES overrides it (tests force a
// batch across a chunk boundary with it).
size_t chunk_bytes() {
    size_t v = 64ull << 20;
    if (const char* e = getenv("LCB_RADIUS_CHUNK_BYTES")) {
        const unsigned long long x = strtoull(e, nullptr, 0);
        if (x) v = (size_t)x;
    }
    return std::max<size_t>(v, kPktMax);
}

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
    RAD_TRY(hipGetDevice(&dev));
    const size_t count = u.count;
    auto off_of = [&](size_t i) -> uint64_t { return u.offsets ? u.offsets[i] : (uint64_t)i * u.stride; };
    auto size_of = [&](size_t i) -> uint32_t { return u.buf_sizes ? u.buf_sizes[i] : u.fixed_size; };
    // The chunk limit of THIS call (the staging buffers only ever grow).
    const size_t limit = std::max<size_t>(std::min<uint64_t>(chunk_bytes(), (uint64_t)count * kPktMax), kPktMax);
    if (int rc = g_stage.ensure(dev, limit, std::min(count, kChunkMsgs))) return rc;
    RadStage& S = g_stage;
    std::vector<Piece> pieces;
    std::vector<uint32_t> msz;  // staged bytes of the chunk's packets
    size_t i = 0;
    while (i < count) {
        // Packets [i, j), each packed at a 16-byte boundary, that fit one chunk.
        uint64_t* h_off = reinterpret_cast<uint64_t*>(S.h_meta);
        size_t j = i, pos = 0, bytes = 0;
        pieces.clear();
        msz.clear();
        while (j < count && j - i < S.mcap) {
            const uint32_t m = staged_size(u.pkts + off_of(j), size_of(j));
            if (j > i && pos + up16(m) > limit) break;
            h_off[j - i] = pos;
            msz.push_back(m);
            if (m) pieces.push_back(Piece{S.h_data + pos, u.pkts + off_of(j), m});
            pos += up16(m);
            bytes += m;
            ++j;
        }
        const size_t n = j - i;
        uint32_t* h_size = reinterpret_cast<uint32_t*>(S.h_meta + n * 8);
        uint32_t* h_kidx = h_size + n;
        int32_t* h_err = reinterpret_cast<int32_t*>(h_kidx + n);
        uint8_t* h_req = reinterpret_cast<uint8_t*>(h_err + n);
        memcpy(h_size, msz.data(), n * 4);
        if (u.key_index) memcpy(h_kidx, u.key_index + i, n * 4);
        if (u.req_hdrs) memcpy(h_req, u.req_hdrs + 20 * i, n * 20);
        parallel_copy(pieces, bytes);
        RadArgs a;
        a.count = n;
        a.pkts = S.d_data;
        a.offsets = reinterpret_cast<const uint64_t*>(S.d_meta);
        a.buf_sizes = reinterpret_cast<const uint32_t*>(S.d_meta + n * 8);
        a.key_index = u.key_index ? reinterpret_cast<const uint32_t*>(S.d_meta + n * 12) : nullptr;
        a.errors = reinterpret_cast<int32_t*>(S.d_meta + n * 16);
        a.req_hdrs = u.req_hdrs ? S.d_meta + n * 20 : nullptr;
        RAD_TRY(hipMemcpyAsync(S.d_meta, S.h_meta, n * 40, hipMemcpyHostToDevice, S.st));
        if (pos) RAD_TRY(hipMemcpyAsync(S.d_data, S.h_data, pos, hipMemcpyHostToDevice, S.st));
        if (int rc = rad_enqueue(a, sign, kt, S.st)) {
            (void)hipStreamSynchronize(S.st);
            return rc;
        }
        RAD_TRY(hipMemcpyAsync(h_err, S.d_meta + n * 16, n * 4, hipMemcpyDeviceToHost, S.st));
        if (pos) RAD_TRY(hipMemcpyAsync(S.h_data, S.d_data, pos, hipMemcpyDeviceToHost, S.st));
        RAD_TRY(hipStreamSynchronize(S.st));
        // Only [0, Length) of the packets that may have changed goes back.
        pieces.clear();
        bytes = 0;
        for (size_t k = 0; k < n; ++k) {
            u.errors[i + k] = h_err[k];
            if (h_err[k] == 0 && h_size[k]) {
                pieces.push_back(Piece{u.pkts + off_of(i + k), S.h_data + h_off[k], h_size[k]});
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
