// lcb_hash_stream_gpu.cpp — exported C-ABI of the batched streaming digests
// (include/lcb_hash_stream_gpu.h), built into liblcb_hash_stream_gpu.so and
// linked against liblcb_hash_gpu.so for the shared runtime pieces
// (ensure_init, map_err, stream-ordered scratch, parallel_copy).
//
// A set owns one device allocation: [init | opad | bad | stamps | contexts]
// (stream_state.hpp: the context layout).  Device mode enqueues (index check,)
// kernel on the caller's stream; with an index list the call then waits for
// the check's 4-byte verdict, which the kernels were gated on.  Host mode
// waits for the device first (the set's earlier device-mode work, its
// creation included, may still be queued on the caller's streams), then
// stages chunk by chunk through page-locked memory on the set's own stream
// and waits; it is NOT pipelined.  The staging buffers belong to the set (not
// host_stage.hpp's per-thread context; the error macro, up16 and the chunk
// size are taken from there).  Nothing falls back to the CPU.
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/lcb_hash_gpu.h"
#include "../../include/lcb_hash_stream_gpu.h"
#include "host_stage.hpp"
#include "lcb_internal.hpp"
#include "stream_internal.hpp"
#include "stream_state.hpp"

using namespace lcbgpu;
using namespace lcbstream;

namespace {

constexpr size_t kInitWords = 128;   // init image (<= kMaxWords), padded
constexpr size_t kOpadWords = 64;    // opad state (<= 48)
constexpr size_t kBadWords = 64;     // the check's flag word, in a line of its own
constexpr size_t kChunkMsgs = 1u << 18;

// Overrides the staging bytes per chunk (tests force an update across a chunk
// boundary with it).
constexpr const char* kChunkEnv = "LCB_HASH_STREAM_CHUNK_BYTES";

// The current device set to a set's for one call.
struct DevGuard {
    int prev = -1;
    bool switched = false;
    explicit DevGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DevGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};

}  // namespace

struct lcb_hash_stream_set_s {
    int alg = 0, device = -1;
    size_t nstreams = 0;
    bool keyed = false;
    uint32_t words = 0;
    uint64_t pitch = 0;
    uint32_t* dmem = nullptr;        // [init | opad | bad | stamps | contexts]
    uint32_t *init = nullptr, *opad = nullptr, *bad = nullptr, *stamp = nullptr, *ctx = nullptr;
    uint32_t* bad_host = nullptr;    // page-locked copy of *bad
    hipEvent_t ev = nullptr;
    uint32_t epoch = 0;
    std::vector<uint8_t> seen;       // host-side index check
    // host mode and export / import.  Not the HostStage of host_stage.hpp:
    // this staging belongs to a set, not to a thread, its stream outlives the
    // buffers, and its sizes are clamped to non-zero.
    hipStream_t st = nullptr;
    size_t cap = 0, mcap = 0;        // staged data bytes / entries
    uint8_t *h_data = nullptr, *d_data = nullptr;
    uint8_t *h_meta = nullptr, *d_meta = nullptr;   // offsets | lengths | index | digests or context images

    static size_t meta_bytes(size_t m) { return m * (8 + 4 + 4) + m * (kMaxWords * 4) + 64; }

    StreamArgs args() const {
        StreamArgs a;
        a.ctx = ctx; a.pitch = pitch; a.nstreams = (uint32_t)nstreams; a.words = words;
        a.init = init; a.opad = keyed ? opad : nullptr; a.stamp = stamp;
        return a;
    }

    void stage_release() {
        if (h_data) (void)hipHostFree(h_data);
        if (h_meta) (void)hipHostFree(h_meta);
        if (d_data) (void)hipFree(d_data);
        if (d_meta) (void)hipFree(d_meta);
        h_data = h_meta = d_data = d_meta = nullptr;
        cap = mcap = 0;
    }

    int stage_ensure(size_t need_bytes, size_t need_msgs) {
        if (!st) LCB_HOST_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        if (cap >= need_bytes && mcap >= need_msgs && h_meta) return 0;
        const size_t nb = std::max<size_t>(std::max(need_bytes, cap), 64), nm = std::max<size_t>(std::max(need_msgs, mcap), 1);
        stage_release();
        LCB_HOST_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_data), nb, hipHostMallocDefault));
        LCB_HOST_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_meta), meta_bytes(nm), hipHostMallocDefault));
        LCB_HOST_TRY(hipMalloc(reinterpret_cast<void**>(&d_data), nb));
        LCB_HOST_TRY(hipMalloc(reinterpret_cast<void**>(&d_meta), meta_bytes(nm)));
        cap = nb;
        mcap = nm;
        return 0;
    }

    void release() {
        stage_release();
        if (st) (void)hipStreamDestroy(st);
        if (ev) (void)hipEventDestroy(ev);
        if (bad_host) (void)hipHostFree(bad_host);
        if (dmem) {
            // the pads go back zeroed, as the hash library's key cache does
            (void)hipMemset(dmem, 0, (kInitWords + kOpadWords) * 4);
            (void)hipFree(dmem);
        }
        st = nullptr; ev = nullptr; bad_host = nullptr; dmem = nullptr;
    }
};

namespace {

typedef lcb_hash_stream_set_s Set;

// A call's epoch for the stamp words; they and the flag start over when the
// 32-bit counter wraps.
int next_epoch(Set* set, hipStream_t s, uint32_t* out) {
    if (++set->epoch == 0) {
        LCB_HOST_TRY(hipMemsetAsync(set->bad, 0, (kBadWords + set->nstreams) * 4, s));
        set->epoch = 1;
    }
    *out = set->epoch;
    return 0;
}

// One device-mode call: (check,) `launch`, then the wait for the check alone.
template <class F>
int run_device(Set* set, StreamArgs a, hipStream_t s, F launch) {
    const bool check = a.index != nullptr;
    if (check) {
        if (int rc = next_epoch(set, s, &a.epoch)) return rc;
        a.bad = set->bad;
        launch_stream_check(a, s);
        LCB_HOST_TRY(hipGetLastError());
        LCB_HOST_TRY(hipMemcpyAsync(set->bad_host, set->bad, 4, hipMemcpyDeviceToHost, s));
        LCB_HOST_TRY(hipEventRecord(set->ev, s));
    }
    launch(a, s);
    const hipError_t e = hipGetLastError();
    if (check) {
        LCB_HOST_TRY(hipEventSynchronize(set->ev));
        if (*set->bad_host == a.epoch) return EINVAL;
    }
    return map_err(e);
}

int common_check(Set* set, size_t count, uint32_t flags, uint32_t allowed) {
    if (!set) return EINVAL;
    if (flags & ~allowed) return EINVAL;
    if (count > set->nstreams) return EINVAL;   // without a list: past the set; with one: an index twice
    return 0;
}

int host_index_check(Set* set, const uint32_t* index, size_t count) {
    if (index && set->seen.size() != set->nstreams) set->seen.assign(set->nstreams, 0);
    return index_check(index, count, set->nstreams, set->seen.data());
}

// Host mode of reset / final: the index list (and the digests) through the
// staging buffers.
int host_simple(Set* set, const uint32_t* index, size_t count, uint8_t* digests, bool keep) {
    if (int rc = host_index_check(set, index, count)) return rc;
    LCB_HOST_TRY(hipDeviceSynchronize());   // behind whatever the caller's streams still hold for this set
    if (int rc = set->stage_ensure(0, count)) return rc;
    const size_t D = dsize(set->alg);
    StreamArgs a = set->args();
    a.count = count;
    uint8_t* d_dig = set->d_meta + up16(count * 4);
    if (index) {
        memcpy(set->h_meta, index, count * 4);
        LCB_HOST_TRY(hipMemcpyAsync(set->d_meta, set->h_meta, count * 4, hipMemcpyHostToDevice, set->st));
        a.index = reinterpret_cast<const uint32_t*>(set->d_meta);
    }
    if (digests) {
        a.digests = d_dig;
        a.keep = keep ? 1u : 0u;
        launch_stream_final(set->alg, a, set->st);
    } else {
        launch_stream_fill(a, set->st);
    }
    LCB_HOST_TRY(hipGetLastError());
    uint8_t* h_dig = set->h_meta + up16(count * 4);
    if (digests) LCB_HOST_TRY(hipMemcpyAsync(h_dig, d_dig, count * D, hipMemcpyDeviceToHost, set->st));
    LCB_HOST_TRY(hipStreamSynchronize(set->st));
    if (digests) memcpy(digests, h_dig, count * D);
    return 0;
}

int host_update(Set* set, const uint32_t* index, const uint8_t* data, const uint64_t* offsets,
                const uint32_t* lengths, size_t count, uint64_t stride, uint32_t fixed_len) {
    if (int rc = host_index_check(set, index, count)) return rc;
    LCB_HOST_TRY(hipDeviceSynchronize());   // behind whatever the caller's streams still hold for this set
    auto off_of = [&](size_t i) -> uint64_t { return offsets ? offsets[i] : (uint64_t)i * stride; };
    auto len_of = [&](size_t i) -> size_t { return lengths ? lengths[i] : fixed_len; };
    size_t maxlen = 0, sum = 0;
    const size_t limit0 = chunk_bytes(kChunkEnv, 64);
    for (size_t i = 0; i < count; ++i) {
        maxlen = std::max(maxlen, len_of(i));
        sum += up16(len_of(i));
    }
    // The chunk limit of THIS call (the staging buffers only ever grow).
    const size_t limit = std::max(limit0, up16(maxlen));
    if (int rc = set->stage_ensure(std::min(limit, sum), std::min(count, kChunkMsgs))) return rc;
    std::vector<Piece> pieces;
    size_t i = 0;
    while (i < count) {
        // Chunks [i, j), each packed at a 16-byte boundary, that fit the staging buffer.
        size_t j = i, total = 0;
        while (j < count && j - i < set->mcap) {
            const size_t n = up16(len_of(j));
            if (j > i && total + n > set->cap) break;
            total += n;
            ++j;
        }
        const size_t n = j - i;
        uint64_t* h_off = reinterpret_cast<uint64_t*>(set->h_meta);
        uint32_t* h_len = reinterpret_cast<uint32_t*>(set->h_meta + n * 8);
        uint32_t* h_idx = h_len + n;
        pieces.clear();
        size_t pos = 0, bytes = 0;
        for (size_t k = 0; k < n; ++k) {
            const size_t u = len_of(i + k);
            if (u) pieces.push_back(Piece{set->h_data + pos, data + off_of(i + k), u});
            h_off[k] = pos;
            h_len[k] = (uint32_t)u;
            h_idx[k] = index ? index[i + k] : (uint32_t)(i + k);
            pos += up16(u);
            bytes += u;
        }
        parallel_copy(pieces, bytes);
        StreamArgs a = set->args();
        a.count = n;
        a.data = set->d_data;
        a.offsets = reinterpret_cast<const uint64_t*>(set->d_meta);
        a.lengths = reinterpret_cast<const uint32_t*>(set->d_meta + n * 8);
        a.index = reinterpret_cast<const uint32_t*>(set->d_meta + n * 12);
        LCB_HOST_TRY(hipMemcpyAsync(set->d_meta, set->h_meta, n * 16, hipMemcpyHostToDevice, set->st));
        if (pos) LCB_HOST_TRY(hipMemcpyAsync(set->d_data, set->h_data, pos, hipMemcpyHostToDevice, set->st));
        launch_stream_update(set->alg, a, set->st);
        LCB_HOST_TRY(hipGetLastError());
        LCB_HOST_TRY(hipStreamSynchronize(set->st));
        i = j;
    }
    return 0;
}

}  // namespace

extern "C" {

int lcb_hash_stream_abi_version(void) { return LCB_HASH_STREAM_ABI_VERSION; }

int lcb_hash_stream_create(int alg, const uint8_t* key, size_t key_len, size_t nstreams, void* stream,
                           lcb_hash_stream_set_p* out) {
    if (!out) return EINVAL;
    *out = nullptr;
    if (!alg_valid(alg) || nstreams == 0 || nstreams > 0xffffffffull) return EINVAL;
    if (!key && key_len) return EINVAL;
    if (int rc = ensure_init()) return rc;
    Set* set = new (std::nothrow) Set;
    if (!set) return ENOMEM;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    auto fail = [&](int rc) {
        set->release();
        delete set;
        return rc;
    };
    auto build = [&]() -> int {
        LCB_HOST_TRY(hipGetDevice(&set->device));
        set->alg = alg;
        set->nstreams = nstreams;
        set->keyed = key != nullptr;
        set->words = alg_words(alg);
        set->pitch = (nstreams + 63) & ~(uint64_t)63;
        const size_t head = kInitWords + kOpadWords + kBadWords;
        const size_t total = head + set->pitch + (size_t)set->words * set->pitch;
        LCB_HOST_TRY(hipMalloc(reinterpret_cast<void**>(&set->dmem), total * 4));
        set->init = set->dmem;
        set->opad = set->init + kInitWords;
        set->bad = set->opad + kOpadWords;
        set->stamp = set->bad + kBadWords;
        set->ctx = set->stamp + set->pitch;
        LCB_HOST_TRY(hipHostMalloc(reinterpret_cast<void**>(&set->bad_host), 64, hipHostMallocDefault));
        *set->bad_host = 0;
        LCB_HOST_TRY(hipEventCreateWithFlags(&set->ev, hipEventDisableTiming));
        LCB_HOST_TRY(hipMemsetAsync(set->dmem, 0, (head + set->pitch) * 4, s));
        // The key travels through stream-ordered scratch, zeroed before it goes back.
        uint8_t* dkey = nullptr;
        const size_t kb = up16(key_len) + 16;
        if (set->keyed) {
            LCB_HOST_TRY(scratch_alloc(reinterpret_cast<void**>(&dkey), kb, s));
            hipError_t e = hipMemsetAsync(dkey, 0, kb, s);
            if (e == hipSuccess && key_len) {
                std::vector<uint8_t> img(key, key + key_len);   // pageable: the copy returns once the bytes are staged
                e = hipMemcpyAsync(dkey, img.data(), key_len, hipMemcpyHostToDevice, s);
                volatile uint8_t* p = img.data();
                for (size_t i = 0; i < img.size(); ++i) p[i] = 0;
            }
            if (e != hipSuccess) {
                (void)scratch_free(dkey, s);
                return map_err(e);
            }
        }
        launch_stream_prep(alg, dkey, key_len, set->keyed, set->init, set->opad, s);
        hipError_t e = hipGetLastError();
        if (dkey) {
            (void)hipMemsetAsync(dkey, 0, kb, s);
            (void)scratch_free(dkey, s);
        }
        if (e != hipSuccess) return map_err(e);
        StreamArgs a = set->args();
        a.count = nstreams;
        launch_stream_fill(a, s);
        LCB_HOST_TRY(hipGetLastError());
        return 0;
    };
    if (int rc = build()) return fail(rc);
    *out = set;
    return 0;
}

int lcb_hash_stream_destroy(lcb_hash_stream_set_p set) {
    if (!set) return EINVAL;
    {
        DevGuard g(set->device);
        (void)hipDeviceSynchronize();
        set->release();
    }
    delete set;
    return 0;
}

size_t lcb_hash_stream_count(lcb_hash_stream_set_p set) { return set ? set->nstreams : 0; }

int lcb_hash_stream_alg(lcb_hash_stream_set_p set) { return set ? set->alg : 0; }

int lcb_hash_stream_reset(lcb_hash_stream_set_p set, const uint32_t* stream_index, size_t count, uint32_t flags,
                          void* stream) {
    if (int rc = common_check(set, count, flags, LCB_HASH_F_DEVICE)) return rc;
    if (count == 0) return 0;
    DevGuard g(set->device);
    if (!(flags & LCB_HASH_F_DEVICE)) return host_simple(set, stream_index, count, nullptr, false);
    StreamArgs a = set->args();
    a.index = stream_index;
    a.count = count;
    return run_device(set, a, reinterpret_cast<hipStream_t>(stream),
                      [](const StreamArgs& x, hipStream_t s) { launch_stream_fill(x, s); });
}

int lcb_hash_stream_update(lcb_hash_stream_set_p set, const uint32_t* stream_index, const uint8_t* data,
                           const uint64_t* offsets, const uint32_t* lengths, size_t count, uint64_t stride,
                           uint32_t fixed_len, uint32_t flags, void* stream) {
    if (int rc = common_check(set, count, flags, LCB_HASH_F_DEVICE)) return rc;
    if (count == 0) return 0;
    if (!data) return EINVAL;
    DevGuard g(set->device);
    if (!(flags & LCB_HASH_F_DEVICE))
        return host_update(set, stream_index, data, offsets, lengths, count, stride, fixed_len);
    StreamArgs a = set->args();
    a.index = stream_index;
    a.count = count;
    a.data = data; a.offsets = offsets; a.lengths = lengths; a.stride = stride; a.fixed_len = fixed_len;
    const int alg = set->alg;
    return run_device(set, a, reinterpret_cast<hipStream_t>(stream),
                      [alg](const StreamArgs& x, hipStream_t s) { launch_stream_update(alg, x, s); });
}

int lcb_hash_stream_final(lcb_hash_stream_set_p set, const uint32_t* stream_index, size_t count, uint8_t* digests,
                          uint32_t flags, void* stream) {
    if (int rc = common_check(set, count, flags, LCB_HASH_F_DEVICE | LCB_HASH_STREAM_F_KEEP)) return rc;
    if (count == 0) return 0;
    if (!digests) return EINVAL;
    const bool keep = (flags & LCB_HASH_STREAM_F_KEEP) != 0;
    DevGuard g(set->device);
    if (!(flags & LCB_HASH_F_DEVICE)) return host_simple(set, stream_index, count, digests, keep);
    StreamArgs a = set->args();
    a.index = stream_index;
    a.count = count;
    a.digests = digests;
    a.keep = keep ? 1u : 0u;
    const int alg = set->alg;
    return run_device(set, a, reinterpret_cast<hipStream_t>(stream),
                      [alg](const StreamArgs& x, hipStream_t s) { launch_stream_final(alg, x, s); });
}

int lcb_hash_stream_export(lcb_hash_stream_set_p set, const uint32_t* stream_index, size_t count,
                           lcb_hash_stream_state_t* states) {
    if (!set || count > set->nstreams) return EINVAL;
    if (count == 0) return 0;
    if (!states) return EINVAL;
    if (int rc = host_index_check(set, stream_index, count)) return rc;
    DevGuard g(set->device);
    LCB_HOST_TRY(hipDeviceSynchronize());
    const size_t W = set->words;
    for (size_t i = 0; i < count;) {
        const size_t n = std::min(count - i, kChunkMsgs);
        if (int rc = set->stage_ensure(0, n)) return rc;
        StreamArgs a = set->args();
        a.count = n;
        uint32_t* d_img = reinterpret_cast<uint32_t*>(set->d_meta + up16(n * 4));
        const uint32_t* h_img = reinterpret_cast<const uint32_t*>(set->h_meta + up16(n * 4));
        uint32_t* h_idx = reinterpret_cast<uint32_t*>(set->h_meta);
        for (size_t k = 0; k < n; ++k) h_idx[k] = stream_index ? stream_index[i + k] : (uint32_t)(i + k);
        LCB_HOST_TRY(hipMemcpyAsync(set->d_meta, set->h_meta, n * 4, hipMemcpyHostToDevice, set->st));
        a.index = reinterpret_cast<const uint32_t*>(set->d_meta);
        launch_stream_gather(a, d_img, set->st);
        LCB_HOST_TRY(hipGetLastError());
        LCB_HOST_TRY(hipMemcpyAsync(set->h_meta + up16(n * 4), d_img, n * W * 4, hipMemcpyDeviceToHost, set->st));
        LCB_HOST_TRY(hipStreamSynchronize(set->st));
        for (size_t k = 0; k < n; ++k) words_to_state(set->alg, h_img + k * W, states[i + k]);
        i += n;
    }
    return 0;
}

int lcb_hash_stream_import(lcb_hash_stream_set_p set, const uint32_t* stream_index, size_t count,
                           const lcb_hash_stream_state_t* states) {
    if (!set || count > set->nstreams) return EINVAL;
    if (count == 0) return 0;
    if (!states) return EINVAL;
    for (size_t i = 0; i < count; ++i)
        if (int rc = state_check(set->alg, states[i])) return rc;
    if (int rc = host_index_check(set, stream_index, count)) return rc;
    DevGuard g(set->device);
    LCB_HOST_TRY(hipDeviceSynchronize());
    const size_t W = set->words;
    for (size_t i = 0; i < count;) {
        const size_t n = std::min(count - i, kChunkMsgs);
        if (int rc = set->stage_ensure(0, n)) return rc;
        StreamArgs a = set->args();
        a.count = n;
        uint32_t* h_idx = reinterpret_cast<uint32_t*>(set->h_meta);
        uint32_t* h_img = reinterpret_cast<uint32_t*>(set->h_meta + up16(n * 4));
        for (size_t k = 0; k < n; ++k) {
            h_idx[k] = stream_index ? stream_index[i + k] : (uint32_t)(i + k);
            state_to_words(set->alg, states[i + k], h_img + k * W);
        }
        const size_t bytes = up16(n * 4) + n * W * 4;
        LCB_HOST_TRY(hipMemcpyAsync(set->d_meta, set->h_meta, bytes, hipMemcpyHostToDevice, set->st));
        a.index = reinterpret_cast<const uint32_t*>(set->d_meta);
        launch_stream_scatter(a, reinterpret_cast<const uint32_t*>(set->d_meta + up16(n * 4)), set->st);
        LCB_HOST_TRY(hipGetLastError());
        LCB_HOST_TRY(hipStreamSynchronize(set->st));
        i += n;
    }
    return 0;
}

}  // extern "C"
