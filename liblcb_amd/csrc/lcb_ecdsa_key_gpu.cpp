// lcb_ecdsa_key_gpu.cpp — exported C-ABI of batched public-key import and
// export (include/lcb_ecdsa_key_gpu.h), built into liblcb_ecdsa_key_gpu.so
// and linked against liblcb_hash_gpu.so for the shared runtime pieces
// (ensure_init, map_err).  The curve table is ecdsa_curves.hpp, parsed here by
// ecdsa_host.hpp; the constants of the square root are derived beside it,
// once; none of the other three ECDSA libraries is linked.
//
// Device mode enqueues one kernel on the caller's stream and never
// synchronises.  Host mode stages chunk by chunk through page-locked memory on
// a private stream: copy -> H2D -> kernel -> D2H -> copy, one chunk in flight
// (the staging context is host_stage.hpp's).  Public keys are no secrets, so
// nothing is wiped.  Nothing falls back to the CPU.
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "../../include/lcb_ecdsa_key_gpu.h"
#include "../../include/lcb_hash_gpu.h"
#include "ecdsa_host.hpp"
#include "ecdsa_key_internal.hpp"
#include "host_stage.hpp"
#include "lcb_internal.hpp"

using namespace lcbgpu;
using namespace lcbec;

namespace {

// The constants of the square root of every curve of table(), derived once.
struct KeyTable {
    KeyConsts<kLimbs> k[kCurveCount];
    bool ok[kCurveCount];
    KeyTable() {
        for (int id = 0; id < kCurveCount; ++id) ok[id] = table().ok[id] && key_setup(k[id], table().c[id]);
    }
};

const KeyTable& key_table() {
    static const KeyTable t;
    return t;
}

// ------------------------------------------------------------ host mode
thread_local HostStage g_stage;
constexpr size_t kChunkItems = 1u << 18;
constexpr size_t kChunkBytes = 64ull << 20;  // of keys / of exported forms per chunk, one item at least
static_assert(sizeof(size_t) >= 8, "chunk * stride: at most max(2^26, 2^32 - 1), and the sums beside it, fit");

size_t chunk_items(size_t count, size_t stride) {
    return std::max<size_t>(1, std::min({count, kChunkItems, kChunkBytes / std::max<size_t>(stride, 1)}));
}

int import_host(const Curve<kLimbs>& c, const KeyConsts<kLimbs>& k, int le, const uint8_t* keys, size_t key_stride,
                const uint32_t* sizes, size_t key_size, const uint8_t* keys_y, size_t count, uint8_t* pub,
                uint8_t* infinity, int32_t* status) {
    int dev = 0;
    LCB_HOST_TRY(hipGetDevice(&dev));
    // One chunk: keys | sizes | keys_y | pub | infinity | status; a part that is not given is empty.
    const size_t chunk = chunk_items(count, key_stride);
    const size_t o_sizes = up16(chunk * key_stride);
    const size_t o_y = o_sizes + (sizes ? up16(chunk * 4) : 0);
    const size_t o_pub = o_y + (keys_y ? chunk * kNumBytes : 0);
    const size_t o_inf = o_pub + chunk * 2 * kNumBytes;
    const size_t o_st = o_inf + up16(chunk);
    const size_t bytes = o_st + chunk * 4;
    if (int rc = g_stage.ensure(dev, bytes, 0)) return rc;
    HostStage& S = g_stage;
    // The last item of the batch is read up to its size only: the caller's buffer may end there.
    const size_t last = sizes ? sizes[count - 1] : key_size;
    const size_t tail = last <= key_stride ? last : 0;
    for (size_t i = 0; i < count; i += chunk) {
        const size_t n = std::min(chunk, count - i);
        const size_t kb = i + n == count ? (n - 1) * key_stride + tail : n * key_stride;
        if (kb) memcpy(S.h, keys + i * key_stride, kb);
        if (sizes) memcpy(S.h + o_sizes, sizes + i, n * 4);
        if (keys_y) memcpy(S.h + o_y, keys_y + i * kNumBytes, n * kNumBytes);
        if (o_pub) LCB_HOST_TRY(hipMemcpyAsync(S.d, S.h, o_pub, hipMemcpyHostToDevice, S.st));
        KeyImportArgs a;
        a.keys = S.d;
        a.sizes = sizes ? reinterpret_cast<const uint32_t*>(S.d + o_sizes) : nullptr;
        a.keys_y = keys_y ? S.d + o_y : nullptr;
        a.pub = S.d + o_pub;
        a.infinity = S.d + o_inf;
        a.status = reinterpret_cast<int32_t*>(S.d + o_st);
        a.count = n;
        a.key_stride = key_stride;
        a.key_size = (uint32_t)std::min<size_t>(key_size, 0xffffffffu);
        a.le = le ? 1u : 0u;
        launch_ecdsa_key_import(a, c, k, S.st);
        LCB_HOST_TRY(hipGetLastError());
        LCB_HOST_TRY(hipMemcpyAsync(S.h + o_pub, S.d + o_pub, o_st - o_pub + n * 4, hipMemcpyDeviceToHost, S.st));
        LCB_HOST_TRY(hipStreamSynchronize(S.st));
        memcpy(pub + i * 2 * kNumBytes, S.h + o_pub, n * 2 * kNumBytes);
        if (infinity) memcpy(infinity + i, S.h + o_inf, n);
        memcpy(status + i, S.h + o_st, n * 4);
    }
    return 0;
}

int export_host(int le, int compress, const uint8_t* pub, const uint8_t* infinity, size_t count, uint8_t* out,
                size_t out_stride, uint32_t* out_sizes, int32_t* status) {
    int dev = 0;
    LCB_HOST_TRY(hipGetDevice(&dev));
    // One chunk: pub | infinity | out | out_sizes | status.  The forms are staged densely, kKeyMaxSize apart.
    const size_t chunk = chunk_items(count, kKeyMaxSize);
    const size_t o_inf = chunk * 2 * kNumBytes;
    const size_t o_out = o_inf + (infinity ? up16(chunk) : 0);
    const size_t o_sz = o_out + up16(chunk * kKeyMaxSize);
    const size_t o_st = o_sz + chunk * 4;
    const size_t bytes = o_st + chunk * 4;
    if (int rc = g_stage.ensure(dev, bytes, 0)) return rc;
    HostStage& S = g_stage;
    for (size_t i = 0; i < count; i += chunk) {
        const size_t n = std::min(chunk, count - i);
        memcpy(S.h, pub + i * 2 * kNumBytes, n * 2 * kNumBytes);
        if (infinity) memcpy(S.h + o_inf, infinity + i, n);
        LCB_HOST_TRY(hipMemcpyAsync(S.d, S.h, o_out, hipMemcpyHostToDevice, S.st));
        KeyExportArgs a;
        a.pub = S.d;
        a.infinity = infinity ? S.d + o_inf : nullptr;
        a.out = S.d + o_out;
        a.out_sizes = reinterpret_cast<uint32_t*>(S.d + o_sz);
        a.status = reinterpret_cast<int32_t*>(S.d + o_st);
        a.count = n;
        a.out_stride = kKeyMaxSize;
        a.compress = compress ? 1u : 0u;
        a.le = le ? 1u : 0u;
        launch_ecdsa_key_export(a, S.st);
        LCB_HOST_TRY(hipGetLastError());
        LCB_HOST_TRY(hipMemcpyAsync(S.h + o_out, S.d + o_out, o_st - o_out + n * 4, hipMemcpyDeviceToHost, S.st));
        LCB_HOST_TRY(hipStreamSynchronize(S.st));
        const uint32_t* sz = reinterpret_cast<const uint32_t*>(S.h + o_sz);
        for (size_t j = 0; j < n; ++j)  // no byte past an item's size is written
            memcpy(out + (i + j) * out_stride, S.h + o_out + j * kKeyMaxSize, std::min<size_t>(sz[j], kKeyMaxSize));
        memcpy(out_sizes + i, S.h + o_sz, n * 4);
        memcpy(status + i, S.h + o_st, n * 4);
    }
    return 0;
}

}  // namespace

extern "C" {

int lcb_ecdsa_key_import_batch(int curve, int le, const uint8_t* keys, size_t key_stride, const uint32_t* sizes,
                               size_t key_size, const uint8_t* keys_y, size_t count, uint8_t* pub_keys,
                               uint8_t* infinity, int32_t* status, uint32_t flags, void* stream) {
    if (flags & ~LCB_HASH_F_DEVICE) return EINVAL;
    if (!known(curve) || !key_table().ok[curve]) return EINVAL;
    if (count > 0xffffffffull || key_stride > 0xffffffffull) return EINVAL;  // no product of the two wraps
    if (count == 0) return 0;
    if (!keys || !pub_keys || !status) return EINVAL;
    if (int rc = ensure_init()) return rc;
    const Curve<kLimbs>& c = table().c[curve];
    const KeyConsts<kLimbs>& k = key_table().k[curve];
    if (flags & LCB_HASH_F_DEVICE) {
        KeyImportArgs a;
        a.keys = keys;
        a.sizes = sizes;
        a.keys_y = keys_y;
        a.pub = pub_keys;
        a.infinity = infinity;
        a.status = status;
        a.count = count;
        a.key_stride = key_stride;
        a.key_size = (uint32_t)std::min<size_t>(key_size, 0xffffffffu);  // any size past 65 is -1 or EINVAL alike
        a.le = le ? 1u : 0u;
        launch_ecdsa_key_import(a, c, k, reinterpret_cast<hipStream_t>(stream));
        return map_err(hipGetLastError());
    }
    return import_host(c, k, le, keys, key_stride, sizes, key_size, keys_y, count, pub_keys, infinity, status);
}

int lcb_ecdsa_key_export_batch(int curve, int le, int form, const uint8_t* pub_keys, const uint8_t* infinity,
                               size_t count, uint8_t* out, size_t out_stride, uint32_t* out_sizes, int32_t* status,
                               uint32_t flags, void* stream) {
    if (flags & ~LCB_HASH_F_DEVICE) return EINVAL;
    if (!known(curve)) return EINVAL;
    if (form != LCB_ECDSA_KEY_PACKED && form != LCB_ECDSA_KEY_COMPRESSED) return EINVAL;
    if (out_stride < (form == LCB_ECDSA_KEY_COMPRESSED ? (size_t)kNumBytes + 1 : (size_t)kKeyMaxSize)) return EINVAL;
    if (count > 0xffffffffull || out_stride > 0xffffffffull) return EINVAL;
    if (count == 0) return 0;
    if (!pub_keys || !out || !out_sizes || !status) return EINVAL;
    if (int rc = ensure_init()) return rc;
    if (flags & LCB_HASH_F_DEVICE) {
        KeyExportArgs a;
        a.pub = pub_keys;
        a.infinity = infinity;
        a.out = out;
        a.out_sizes = out_sizes;
        a.status = status;
        a.count = count;
        a.out_stride = out_stride;
        a.compress = form == LCB_ECDSA_KEY_COMPRESSED ? 1u : 0u;
        a.le = le ? 1u : 0u;
        launch_ecdsa_key_export(a, reinterpret_cast<hipStream_t>(stream));
        return map_err(hipGetLastError());
    }
    return export_host(le, form == LCB_ECDSA_KEY_COMPRESSED, pub_keys, infinity, count, out, out_stride, out_sizes,
                       status);
}

int ecdsa_pub_key_import_be_batch(int curve, const uint8_t* keys, size_t key_stride, const uint32_t* sizes,
                                  size_t key_size, const uint8_t* keys_y, size_t count, uint8_t* pub_keys,
                                  uint8_t* infinity, int32_t* status, uint32_t flags, void* stream) {
    return lcb_ecdsa_key_import_batch(curve, 0, keys, key_stride, sizes, key_size, keys_y, count, pub_keys, infinity,
                                      status, flags, stream);
}

int ecdsa_pub_key_import_le_batch(int curve, const uint8_t* keys, size_t key_stride, const uint32_t* sizes,
                                  size_t key_size, const uint8_t* keys_y, size_t count, uint8_t* pub_keys,
                                  uint8_t* infinity, int32_t* status, uint32_t flags, void* stream) {
    return lcb_ecdsa_key_import_batch(curve, 1, keys, key_stride, sizes, key_size, keys_y, count, pub_keys, infinity,
                                      status, flags, stream);
}

int ecdsa_pub_key_export_be_batch(int curve, int compress, const uint8_t* pub_keys, const uint8_t* infinity,
                                  size_t count, uint8_t* out, size_t out_stride, uint32_t* out_sizes, int32_t* status,
                                  uint32_t flags, void* stream) {
    return lcb_ecdsa_key_export_batch(curve, 0, compress ? LCB_ECDSA_KEY_COMPRESSED : LCB_ECDSA_KEY_PACKED, pub_keys,
                                      infinity, count, out, out_stride, out_sizes, status, flags, stream);
}

int ecdsa_pub_key_export_le_batch(int curve, int compress, const uint8_t* pub_keys, const uint8_t* infinity,
                                  size_t count, uint8_t* out, size_t out_stride, uint32_t* out_sizes, int32_t* status,
                                  uint32_t flags, void* stream) {
    return lcb_ecdsa_key_export_batch(curve, 1, compress ? LCB_ECDSA_KEY_COMPRESSED : LCB_ECDSA_KEY_PACKED, pub_keys,
                                      infinity, count, out, out_stride, out_sizes, status, flags, stream);
}

}  // extern "C"
