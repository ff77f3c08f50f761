// ecdsa_sign_host.hpp — what the C-ABI units of liblcb_ecdsa_sign_gpu.so and
// liblcb_ecdsa_wide_sign_gpu.so share on the host, at every limb count L: the
// cache of window tables, the host-mode staging of a signing and of a key
// batch, and the launch of either mode (sign_run, keys_run).  Host only;
// internal linkage, so every library has its own tables, lock and staging
// context.
//
// What differs per library comes in as a type `Lib`:
//
//   Lib::kChunkItems           items per host-mode chunk
//   Lib::sign(a, c, t, stream) the library's kernel launch for SignArgs
//   Lib::keys(a, c, t, stream) the library's kernel launch for KeyArgs
//
// and the caller passes the curve's constant block, which it looks up in its
// own curve table.  The argument checks, with the library's hash_size ceiling,
// and ensure_init() come before sign_run / keys_run, in the caller.
//
// The window table of a curve's base point (60 KiB at 8 limbs, 135 KiB at 12,
// 240 KiB at 16) is derived on the host once per process and uploaded once per
// device, under a lock, with a blocking copy; it stays for the life of the
// process.
//
// Device mode enqueues one kernel on the caller's stream and never
// synchronises (after that first upload).  Host mode stages chunk by chunk
// through page-locked memory on a private stream: copy -> H2D -> kernel ->
// D2H -> copy, one chunk in flight.  After the last chunk every staging
// buffer, page-locked and on the device, is overwritten with zeros: they held
// private keys and nonces (the staging context and its wipe() are
// host_stage.hpp's).  Nothing falls back to the CPU.
#pragma once
#include <errno.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/lcb_hash_gpu.h"
#include "ecdsa_sign_args.hpp"
#include "ecdsa_sign_math.hpp"
#include "host_stage.hpp"
#include "lcb_internal.hpp"

namespace lcbec {
namespace {

using lcbgpu::HostStage;
using lcbgpu::map_err;
using lcbgpu::up16;

static_assert(sizeof(BaseTable<8>) == 61440 && sizeof(BaseTable<12>) == 138240 && sizeof(BaseTable<16>) == 245760,
              "the tables are packed");

// ------------------------------------------------------- the window tables
// Host and device copies are kept as bytes: a curve has one limb count.
std::mutex g_tables_mu;
std::map<int, std::unique_ptr<uint8_t[]>> g_host_table;  // curve -> the derived table
std::map<std::pair<int, int>, void*> g_dev_table;        // (device, curve) -> device memory, never freed

// The window table of `curve` (constant block c) on the current device;
// uploads it on first use.
template <int L>
int base_table(int curve, const Curve<L>& c, const BaseTable<L>** out) {
    int dev = 0;
    LCB_HOST_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_tables_mu);
    auto it = g_dev_table.find({dev, curve});
    if (it == g_dev_table.end()) {
        if (!g_host_table[curve]) {
            std::unique_ptr<uint8_t[]> t(new uint8_t[sizeof(BaseTable<L>)]);
            const size_t n = 8 * L * kWinEntries;
            std::vector<Jac<L>> pts(n);
            std::vector<Num<L>> pre(n);
            if (!base_table_setup(*reinterpret_cast<BaseTable<L>*>(t.get()), c, pts.data(), pre.data())) return EINVAL;
            g_host_table[curve] = std::move(t);
        }
        void* d = nullptr;
        LCB_HOST_TRY(hipMalloc(&d, sizeof(BaseTable<L>)));
        const hipError_t e = hipMemcpy(d, g_host_table[curve].get(), sizeof(BaseTable<L>), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            return map_err(e);
        }
        it = g_dev_table.emplace(std::make_pair(dev, curve), d).first;
    }
    *out = static_cast<const BaseTable<L>*>(it->second);
    return 0;
}

// ------------------------------------------------------------ host mode
// h / d: one chunk, inputs | outputs | status.  h2 / d2: the whole key table of a
// key_idx batch.
thread_local HostStage g_stage;

struct SignLayout {
    size_t chunk, o_rnd, o_priv, o_idx, o_sig, o_st, bytes, key_bytes;
};

template <class Lib, int L>
int sign_chunks(HostStage& S, const SignLayout& y, const Curve<L>& c, const BaseTable<L>* t, int le,
                const uint8_t* hashes, size_t hash_size, const uint8_t* priv, size_t nkeys, const uint32_t* key_idx,
                const uint8_t* rnd, size_t count, uint8_t* sigs, int32_t* status) {
    constexpr size_t B = 4 * L;
    if (y.key_bytes) {
        memcpy(S.h2, priv, y.key_bytes);
        LCB_HOST_TRY(hipMemcpyAsync(S.d2, S.h2, y.key_bytes, hipMemcpyHostToDevice, S.st));
    }
    for (size_t i = 0; i < count; i += y.chunk) {
        const size_t n = std::min(y.chunk, count - i);
        memcpy(S.h, hashes + i * hash_size, n * hash_size);
        memcpy(S.h + y.o_rnd, rnd + i * B, n * B);
        if (key_idx)
            memcpy(S.h + y.o_idx, key_idx + i, n * 4);
        else
            memcpy(S.h + y.o_priv, priv + i * B, n * B);
        LCB_HOST_TRY(hipMemcpyAsync(S.d, S.h, y.o_sig, hipMemcpyHostToDevice, S.st));
        SignArgs a;
        a.hashes = S.d;
        a.rnd = S.d + y.o_rnd;
        a.priv = key_idx ? S.d2 : S.d + y.o_priv;
        a.key_idx = key_idx ? reinterpret_cast<const uint32_t*>(S.d + y.o_idx) : nullptr;
        a.sigs = S.d + y.o_sig;
        a.status = reinterpret_cast<int32_t*>(S.d + y.o_st);
        a.count = n;
        a.nkeys = key_idx ? nkeys : n;
        a.hash_size = (uint32_t)hash_size;
        a.le = le ? 1u : 0u;
        Lib::sign(a, c, t, S.st);
        LCB_HOST_TRY(hipGetLastError());
        LCB_HOST_TRY(
            hipMemcpyAsync(S.h + y.o_sig, S.d + y.o_sig, y.o_st - y.o_sig + n * 4, hipMemcpyDeviceToHost, S.st));
        LCB_HOST_TRY(hipStreamSynchronize(S.st));
        memcpy(sigs + i * 2 * B, S.h + y.o_sig, n * 2 * B);
        memcpy(status + i, S.h + y.o_st, n * 4);
    }
    return 0;
}

template <class Lib, int L>
int sign_host(const Curve<L>& c, const BaseTable<L>* t, int le, const uint8_t* hashes, size_t hash_size,
              const uint8_t* priv, size_t nkeys, const uint32_t* key_idx, const uint8_t* rnd, size_t count,
              uint8_t* sigs, int32_t* status) {
    constexpr size_t B = 4 * L;
    int dev = 0;
    LCB_HOST_TRY(hipGetDevice(&dev));
    SignLayout y;
    y.chunk = std::min(count, (size_t)Lib::kChunkItems);
    y.o_rnd = up16(y.chunk * hash_size);
    y.o_priv = y.o_rnd + y.chunk * B;
    y.o_idx = y.o_priv + (key_idx ? 0 : y.chunk * B);
    y.o_sig = y.o_idx + up16(y.chunk * 4);
    y.o_st = y.o_sig + y.chunk * 2 * B;
    y.bytes = y.o_st + y.chunk * 4;
    y.key_bytes = key_idx ? nkeys * B : 0;
    if (int rc = g_stage.ensure(dev, y.bytes, y.key_bytes)) return rc;
    const int rc =
        sign_chunks<Lib>(g_stage, y, c, t, le, hashes, hash_size, priv, nkeys, key_idx, rnd, count, sigs, status);
    const int wrc = g_stage.wipe(y.bytes, y.key_bytes);  // also after an error
    return rc ? rc : wrc;
}

struct KeyLayout {
    size_t chunk, o_priv, o_pub, o_st, bytes;
};

template <class Lib, int L>
int keys_chunks(HostStage& S, const KeyLayout& y, const Curve<L>& c, const BaseTable<L>* t, int le, bool from_rnd,
                const uint8_t* in, size_t count, uint8_t* priv, uint8_t* pub, int32_t* status) {
    constexpr size_t B = 4 * L;
    for (size_t i = 0; i < count; i += y.chunk) {
        const size_t n = std::min(y.chunk, count - i);
        memcpy(S.h, in + i * B, n * B);
        LCB_HOST_TRY(hipMemcpyAsync(S.d, S.h, n * B, hipMemcpyHostToDevice, S.st));
        KeyArgs a;
        a.in = S.d;
        a.priv = from_rnd ? S.d + y.o_priv : nullptr;
        a.pub = S.d + y.o_pub;
        a.status = reinterpret_cast<int32_t*>(S.d + y.o_st);
        a.count = n;
        a.from_rnd = from_rnd ? 1u : 0u;
        a.le = le ? 1u : 0u;
        Lib::keys(a, c, t, S.st);
        LCB_HOST_TRY(hipGetLastError());
        LCB_HOST_TRY(
            hipMemcpyAsync(S.h + y.o_priv, S.d + y.o_priv, y.o_st - y.o_priv + n * 4, hipMemcpyDeviceToHost, S.st));
        LCB_HOST_TRY(hipStreamSynchronize(S.st));
        if (from_rnd) memcpy(priv + i * B, S.h + y.o_priv, n * B);
        memcpy(pub + i * 2 * B, S.h + y.o_pub, n * 2 * B);
        memcpy(status + i, S.h + y.o_st, n * 4);
    }
    return 0;
}

template <class Lib, int L>
int keys_host(const Curve<L>& c, const BaseTable<L>* t, int le, bool from_rnd, const uint8_t* in, size_t count,
              uint8_t* priv, uint8_t* pub, int32_t* status) {
    constexpr size_t B = 4 * L;
    int dev = 0;
    LCB_HOST_TRY(hipGetDevice(&dev));
    KeyLayout y;
    y.chunk = std::min(count, (size_t)Lib::kChunkItems);
    y.o_priv = y.chunk * B;
    y.o_pub = y.o_priv + (from_rnd ? y.chunk * B : 0);
    y.o_st = y.o_pub + y.chunk * 2 * B;
    y.bytes = y.o_st + y.chunk * 4;
    if (int rc = g_stage.ensure(dev, y.bytes, 0)) return rc;
    const int rc = keys_chunks<Lib>(g_stage, y, c, t, le, from_rnd, in, count, priv, pub, status);
    const int wrc = g_stage.wipe(y.bytes, 0);  // also after an error
    return rc ? rc : wrc;
}

// ------------------------------------------------------- either memory mode
// After the argument checks and ensure_init, at the curve's limb count.
template <class Lib, int L>
int sign_run(int curve, const Curve<L>& c, int le, const uint8_t* hashes, size_t hash_size, const uint8_t* priv_keys,
             size_t nkeys, const uint32_t* key_idx, const uint8_t* rnd, size_t count, uint8_t* sigs, int32_t* status,
             uint32_t flags, void* stream) {
    const BaseTable<L>* t = nullptr;
    if (int rc = base_table<L>(curve, c, &t)) return rc;
    if (flags & LCB_HASH_F_DEVICE) {
        SignArgs a;
        a.hashes = hashes;
        a.priv = priv_keys;
        a.key_idx = key_idx;
        a.rnd = rnd;
        a.sigs = sigs;
        a.status = status;
        a.count = count;
        a.nkeys = nkeys;
        a.hash_size = (uint32_t)hash_size;
        a.le = le ? 1u : 0u;
        Lib::sign(a, c, t, reinterpret_cast<hipStream_t>(stream));
        return map_err(hipGetLastError());
    }
    return sign_host<Lib>(c, t, le, hashes, hash_size, priv_keys, nkeys, key_idx, rnd, count, sigs, status);
}

template <class Lib, int L>
int keys_run(int curve, const Curve<L>& c, int le, bool from_rnd, const uint8_t* in, size_t count, uint8_t* priv,
             uint8_t* pub, int32_t* status, uint32_t flags, void* stream) {
    const BaseTable<L>* t = nullptr;
    if (int rc = base_table<L>(curve, c, &t)) return rc;
    if (flags & LCB_HASH_F_DEVICE) {
        KeyArgs a;
        a.in = in;
        a.priv = from_rnd ? priv : nullptr;
        a.pub = pub;
        a.status = status;
        a.count = count;
        a.from_rnd = from_rnd ? 1u : 0u;
        a.le = le ? 1u : 0u;
        Lib::keys(a, c, t, reinterpret_cast<hipStream_t>(stream));
        return map_err(hipGetLastError());
    }
    return keys_host<Lib>(c, t, le, from_rnd, in, count, priv, pub, status);
}

}  // namespace
}  // namespace lcbec
