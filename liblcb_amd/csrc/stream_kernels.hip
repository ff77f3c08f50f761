// stream_kernels.hip — kernels of the batched streaming digests
// (include/lcb_hash_stream_gpu.h, liblcb_hash_stream_gpu.so): one lane per
// stream, contexts word-major in device memory (stream_state.hpp), so a
// wave's context loads and stores are coalesced when streams are addressed in
// order.  The compression functions, block loaders and the GOST LPS tables are
// the hash library's device headers; the kernels themselves live in this
// library's code object only.
#include <hip/hip_runtime.h>

#include "gost_device.hpp"
#include "hash_device.hpp"
#include "stream_internal.hpp"
#include "stream_state.hpp"

namespace lcbstream {

using namespace lcbgpu;

constexpr int kThreads = 256;

// True when the index check of this call (stream_check_kernel, earlier on
// the same stream) refused the list: the call then loads and stores nothing.
__device__ __forceinline__ bool aborted(const StreamArgs& a) {
    if (!a.bad) return false;
    return *(const __attribute__((address_space(1))) uint32_t*)(uintptr_t)a.bad == a.epoch;
}

// Entry i of the call and its stream; false for a lane without one.
__device__ __forceinline__ bool entry_of(const StreamArgs& a, uint64_t& i, uint32_t& sx) {
    i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return false;
    sx = a.index ? gptr(a.index)[i] : (uint32_t)i;
    return sx < a.nstreams;   // always true after the check; keeps every access inside ctx regardless
}

__device__ __forceinline__ void chunk_of(const StreamArgs& a, uint64_t i, const uint8_t*& p, uint64_t& len) {
    p = gptr(a.data) + (a.offsets ? gptr(a.offsets)[i] : i * a.stride);
    len = a.lengths ? (uint64_t)gptr(a.lengths)[i] : (uint64_t)a.fixed_len;
}

// OR bytes [lo, hi) of the block whose byte 0 is at p into w (raw LE words):
// the seam assembly of load_vblock64.  Only dwords holding a byte of
// [p + lo, p + hi) are read, so p itself may lie ahead of the chunk.
template <int kBlock>
__device__ __forceinline__ void or_block(const uint8_t* p, uint32_t lo, uint32_t hi, uint32_t* w) {
#pragma unroll
    for (int h = 0; h < kBlock / 64; ++h) {
        const uint32_t b = 64u * h;
        const uint32_t l = lo > b ? lo - b : 0u;
        const uint32_t e = hi > b ? (hi - b < 64u ? hi - b : 64u) : 0u;
        if (l < e) or_window64(p + b, l, e, w + 16 * h);
    }
}

template <int N>
__device__ __forceinline__ void ctx_load(uint32_t (&w)[N], const uint32_t* c, uint64_t P) {
#pragma unroll
    for (int k = 0; k < N; ++k) w[k] = c[k * P];
}
template <int N>
__device__ __forceinline__ void ctx_store(const uint32_t (&w)[N], uint32_t* c, uint64_t P) {
#pragma unroll
    for (int k = 0; k < N; ++k) c[k * P] = w[k];
}

// ------------------------------------------------------------ index check
// One stamp word per stream holds the epoch of the last call that listed it:
// meeting this call's epoch there means the index occurs twice.
__global__ __launch_bounds__(kThreads) void stream_check_kernel(StreamArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    const uint32_t sx = gptr(a.index)[i];
    bool bad = sx >= a.nstreams;
    if (!bad) bad = atomicExch(gptr(a.stamp) + sx, a.epoch) == a.epoch;
    if (bad) *gptr(a.bad) = a.epoch;
}

// ------------------------------------------------------------ reset, export, import
__global__ __launch_bounds__(kThreads) void stream_fill_kernel(StreamArgs a) {
    if (aborted(a)) return;
    uint64_t i;
    uint32_t sx;
    if (!entry_of(a, i, sx)) return;
    uint32_t* c = gptr(a.ctx) + sx;
    for (uint32_t k = 0; k < a.words; ++k) c[k * a.pitch] = gptr(a.init)[k];
}

__global__ __launch_bounds__(kThreads) void stream_gather_kernel(StreamArgs a, uint32_t* image) {
    uint64_t i;
    uint32_t sx;
    if (!entry_of(a, i, sx)) return;
    const uint32_t* c = gptr(a.ctx) + sx;
    for (uint32_t k = 0; k < a.words; ++k) gptr(image)[i * a.words + k] = c[k * a.pitch];
}

__global__ __launch_bounds__(kThreads) void stream_scatter_kernel(StreamArgs a, const uint32_t* image) {
    uint64_t i;
    uint32_t sx;
    if (!entry_of(a, i, sx)) return;
    uint32_t* c = gptr(a.ctx) + sx;
    for (uint32_t k = 0; k < a.words; ++k) c[k * a.pitch] = gptr(image)[i * a.words + k];
}

// ------------------------------------------------------------ MD5 / SHA
// *_update (md5.h:233-262, sha1.h:761-800, sha2.h:647-681): the whole blocks
// of the virtual message buf[0, used) || chunk go through H::compress, the
// rest becomes the new leftover.  No padding.  SHA-224 / SHA-384 run the
// SHA-256 / SHA-512 instance: the state comes from the context.
template <class H>
__global__ __launch_bounds__(kThreads) void stream_update_kernel(StreamArgs a) {
    if (aborted(a)) return;
    uint64_t i;
    uint32_t sx;
    if (!entry_of(a, i, sx)) return;
    const uint8_t* chunk;
    uint64_t len;
    chunk_of(a, i, chunk, len);
    if (len == 0) return;
    constexpr uint32_t B = H::kBlock;
    constexpr int S = sizeof(H::s) / 4;
    uint32_t* c = gptr(a.ctx) + sx;
    const uint64_t P = a.pitch;
    const uint64_t count = (uint64_t)c[kMdCount * P] | ((uint64_t)c[(kMdCount + 1) * P] << 32);
    const uint64_t ncount = count + len;
    c[kMdCount * P] = (uint32_t)ncount;
    c[(kMdCount + 1) * P] = (uint32_t)(ncount >> 32);
    if (B == 128 && ncount < count) {   // sha2.h:658-661
        const uint64_t hi = ((uint64_t)c[kMdCountHi * P] | ((uint64_t)c[(kMdCountHi + 1) * P] << 32)) + 1;
        c[kMdCountHi * P] = (uint32_t)hi;
        c[(kMdCountHi + 1) * P] = (uint32_t)(hi >> 32);
    }
    const uint32_t used = (uint32_t)(count & (B - 1));
    const uint64_t total = used + len;
    const uint64_t nblk = total / B;
    const uint32_t rem = (uint32_t)(total % B);
    const uint8_t* v0 = chunk - used;   // where byte 0 of the virtual message would lie
    uint32_t w[H::kWords];
    if (nblk == 0) {                    // the leftover grows
        ctx_load(w, c + kMdBuf * P, P);
        or_block<B>(v0, used, rem, w);
        ctx_store(w, c + kMdBuf * P, P);
        return;
    }
    H st;
    uint32_t sw[S];
    ctx_load(sw, c + kMdH * P, P);
    load_words(st.s, sw);
    for (uint64_t j = 0; j < nblk; ++j) {
        if (j == 0 && used) {           // the block across the seam
            ctx_load(w, c + kMdBuf * P, P);
            or_block<B>(v0, used, B, w);
        } else {
            load_block_full<H>(v0 + j * B, w);
        }
        st.compress(w);
    }
    save_words(st.s, sw);
    ctx_store(sw, c + kMdH * P, P);
    load_block_tail<H>(v0 + nblk * B, rem, w);
    ctx_store(w, c + kMdBuf * P, P);
}

// *_final (md5.h:266-288, sha1.h:816-840, sha2.h:706-742) from the leftover,
// the outer pass of a keyed set (md5.h:346-359), then the stream re-initialised
// unless the call keeps it.
template <class H>
__global__ __launch_bounds__(kThreads) void stream_final_kernel(StreamArgs a) {
    if (aborted(a)) return;
    uint64_t i;
    uint32_t sx;
    if (!entry_of(a, i, sx)) return;
    constexpr uint32_t B = H::kBlock;
    constexpr int S = sizeof(H::s) / 4;
    uint32_t* c = gptr(a.ctx) + sx;
    const uint64_t P = a.pitch;
    const uint64_t count = (uint64_t)c[kMdCount * P] | ((uint64_t)c[(kMdCount + 1) * P] << 32);
    const uint32_t rem = (uint32_t)(count & (B - 1));
    H st;
    uint32_t sw[S], w[H::kWords];
    ctx_load(sw, c + kMdH * P, P);
    load_words(st.s, sw);
    ctx_load(w, c + kMdBuf * P, P);
#pragma unroll
    for (int h = 0; h < (int)B / 64; ++h)
        if ((rem >> 6) == (uint32_t)h) put_byte(w + 16 * h, rem & 63u, 0x80u);
    if (rem + 1 + H::kLenBytes > B) {   // no room for the length
        st.compress(w);
#pragma unroll
        for (int k = 0; k < H::kWords; ++k) w[k] = 0u;
    }
    if constexpr (B == 64) {
        H::put_length(w, count);        // count << 3, modulo 2^64 as the reference
    } else {                            // sha2.h:727-730
        const uint64_t chi = (uint64_t)c[kMdCountHi * P] | ((uint64_t)c[(kMdCountHi + 1) * P] << 32);
        const uint64_t hi = (chi << 3) | (count >> 61), lo = count << 3;
        w[28] = bswap32((uint32_t)(hi >> 32)); w[29] = bswap32((uint32_t)hi);
        w[30] = bswap32((uint32_t)(lo >> 32)); w[31] = bswap32((uint32_t)lo);
    }
    st.compress(w);
    uint32_t dw[H::kDigest / 4];
    st.digest_words(dw);
    if (a.opad) {
        H o;
        load_words(o.s, gptr(a.opad) + kMdH);
        md_outer(o, dw);
        o.digest_words(dw);
    }
    store_digest<H::kDigest>(gptr(a.digests) + i * H::kDigest, dw);
    if (!a.keep)
        for (uint32_t k = 0; k < kMdWords; ++k) c[k * P] = gptr(a.init)[k];
}

// The initial context of a set and, for a keyed one, the K ^ ipad / K ^ opad
// mid-states (md5.h:309-338): one lane, once per set.
template <class H>
__global__ __launch_bounds__(64) void stream_prep_kernel(const uint8_t* key, uint64_t klen, uint32_t keyed,
                                                         uint32_t* init, uint32_t* opad) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    constexpr uint32_t B = H::kBlock;
    constexpr int S = sizeof(H::s) / 4;
    for (uint32_t k = 0; k < kMdWords; ++k) init[k] = 0u;
    H st;
    st.init();
    uint32_t sw[S];
    if (keyed) {
        uint32_t kb[H::kWords], w[H::kWords];
        if (klen > B) {                 // a long key is replaced by its digest
            H t;
            t.init();
            md_message(t, gptr(key), klen, 0);
            uint32_t dw[H::kDigest / 4];
            t.digest_words(dw);
#pragma unroll
            for (int k = 0; k < H::kWords; ++k) kb[k] = k < H::kDigest / 4 ? dw[k] : 0u;
        } else {
            load_block_tail<H>(gptr(key), (uint32_t)klen, kb);
        }
#pragma unroll
        for (int k = 0; k < H::kWords; ++k) w[k] = kb[k] ^ 0x36363636u;
        st.compress(w);
        H o;
        o.init();
#pragma unroll
        for (int k = 0; k < H::kWords; ++k) w[k] = kb[k] ^ 0x5c5c5c5cu;
        o.compress(w);
        save_words(o.s, sw);
        for (int k = 0; k < S; ++k) opad[kMdH + k] = sw[k];
        init[kMdCount] = B;             // the ipad block counts (md5.h:335)
    }
    save_words(st.s, sw);
    for (int k = 0; k < S; ++k) init[kMdH + k] = sw[k];
}

// ------------------------------------------------------------ GOST R 34.11-2012
// g_N(h, m) with the whole 512-bit counter (gost3411-2012.h:1129-1142; the
// batch kernels' gost_g carries only N's low word, enough for one message
// below 2^61 bytes, not for a resumed context).
template <class Tab>
__device__ __forceinline__ void gost_g_n(uint64_t h[8], const uint64_t n[8], const uint64_t m[8], const Tab& T) {
    uint64_t k[8], t[8], x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        k[i] = h[i];
        t[i] = m[i];
        h[i] ^= m[i];
    }
#pragma unroll 1
    for (int r = 0; r < 13; ++r) {
        if (r == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = k[i] ^ n[i];
        } else {
            T.xor_c(x, k, r - 1);
        }
        T.lps(k, x);
        if (r == 12) break;
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = t[i] ^ k[i];
        T.lps(t, x);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] ^= t[i] ^ k[i];
}

// The reference context's h, counter and sigma, carried from call to call
// (never recomputed from the message).
struct GostStream {
    uint64_t h[8], n[8], sg[8];
    __device__ __forceinline__ void init(bool k256) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            h[i] = k256 ? 0x0101010101010101ull : 0ull;
            n[i] = 0;
            sg[i] = 0;
        }
    }
    __device__ __forceinline__ void load(const uint32_t* c, uint64_t P) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            h[i] = (uint64_t)c[(kGoH + 2 * i) * P] | ((uint64_t)c[(kGoH + 2 * i + 1) * P] << 32);
            n[i] = (uint64_t)c[(kGoN + 2 * i) * P] | ((uint64_t)c[(kGoN + 2 * i + 1) * P] << 32);
            sg[i] = (uint64_t)c[(kGoSigma + 2 * i) * P] | ((uint64_t)c[(kGoSigma + 2 * i + 1) * P] << 32);
        }
    }
    __device__ __forceinline__ void save(uint32_t* c, uint64_t P) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            c[(kGoH + 2 * i) * P] = (uint32_t)h[i]; c[(kGoH + 2 * i + 1) * P] = (uint32_t)(h[i] >> 32);
            c[(kGoN + 2 * i) * P] = (uint32_t)n[i]; c[(kGoN + 2 * i + 1) * P] = (uint32_t)(n[i] >> 32);
            c[(kGoSigma + 2 * i) * P] = (uint32_t)sg[i]; c[(kGoSigma + 2 * i + 1) * P] = (uint32_t)(sg[i] >> 32);
        }
    }
    // One block of `bits` message bits (gost3411-2012.h:1129-1142).
    template <class Tab>
    __device__ __forceinline__ void block(const uint32_t* w, uint32_t bits, const Tab& T) {
        uint64_t m[8];
        uint32_t carry = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {   // Sigma += m mod 2^512 (:996-1013)
            m[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
            const uint64_t s1 = sg[i] + m[i];
            const uint32_t c1 = s1 < m[i];
            const uint64_t s2 = s1 + carry;
            carry = c1 | (s2 < s1);
            sg[i] = s2;
        }
        gost_g_n(h, n, m, T);
        uint64_t cr = bits;             // N += bits mod 2^512 (:1015-1024)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint64_t s = n[i] + cr;
            cr = s < cr ? 1u : 0u;
            n[i] = s;
        }
    }
    // gost3411_2012_final (:1820-1837): w holds the `rem` leftover bytes, zero filled.
    template <class Tab>
    __device__ __forceinline__ void finish(uint32_t* w, uint32_t rem, const Tab& T) {
        put_byte(w, rem, 0x01u);
        block(w, rem * 8u, T);
        uint64_t z[8], m[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { z[i] = 0; m[i] = n[i]; }
        gost_g_n(h, z, m, T);           // g_0(h, N)
#pragma unroll
        for (int i = 0; i < 8; ++i) m[i] = sg[i];
        gost_g_n(h, z, m, T);           // g_0(h, Sigma)
    }
};

// gost3411_2012_update (gost3411-2012.h:1767-1799); one kernel for both
// digest sizes (the chaining value comes from the context).
__global__ __launch_bounds__(kThreads) void gost_stream_update_kernel(StreamArgs a) {
    __shared__ __attribute__((aligned(256))) uint64_t Timg[256 * 32];   // 64 KiB rotated image
    if (aborted(a)) return;             // the same for every lane of the grid
    gost_stage_rot(Timg);
    GostRot T;
    T.init((lds_u8*)Timg);
    uint64_t i;
    uint32_t sx;
    if (!entry_of(a, i, sx)) return;
    const uint8_t* chunk;
    uint64_t len;
    chunk_of(a, i, chunk, len);
    if (len == 0) return;
    uint32_t* c = gptr(a.ctx) + sx;
    const uint64_t P = a.pitch;
    const uint32_t used = c[kGoUsed * P] & 63u;
    const uint64_t total = used + len;
    const uint64_t nblk = total >> 6;
    const uint32_t rem = (uint32_t)(total & 63u);
    const uint8_t* v0 = chunk - used;
    uint32_t w[16];
    c[kGoUsed * P] = rem;
    if (nblk == 0) {
        ctx_load(w, c + kGoBuf * P, P);
        or_block<64>(v0, used, rem, w);
        ctx_store(w, c + kGoBuf * P, P);
        return;
    }
    GostStream st;
    st.load(c, P);
    for (uint64_t j = 0; j < nblk; ++j) {
        if (j == 0 && used) {
            ctx_load(w, c + kGoBuf * P, P);
            or_block<64>(v0, used, 64, w);
        } else {
            load_full64(v0 + 64 * j, w);
        }
        st.block(w, 512, T);
    }
    st.save(c, P);
    load_tail64(v0 + 64 * nblk, rem, w);
    ctx_store(w, c + kGoBuf * P, P);
}

// gost3411_2012_final, and hmac_gost3411_2012_final's outer pass for a keyed
// set (gost3411-2012.h:1905-1922).
template <bool k256>
__global__ __launch_bounds__(kThreads) void gost_stream_final_kernel(StreamArgs a) {
    __shared__ __attribute__((aligned(256))) uint64_t Timg[256 * 32];
    if (aborted(a)) return;
    gost_stage_rot(Timg);
    GostRot T;
    T.init((lds_u8*)Timg);
    uint64_t i;
    uint32_t sx;
    if (!entry_of(a, i, sx)) return;
    constexpr int D = k256 ? 32 : 64;
    uint32_t* c = gptr(a.ctx) + sx;
    const uint64_t P = a.pitch;
    GostStream st;
    st.load(c, P);
    uint32_t rem = c[kGoUsed * P] & 63u;
    uint32_t w[16], dw[D / 4];
    ctx_load(w, c + kGoBuf * P, P);
    const int passes = a.opad ? 2 : 1;
#pragma unroll 1
    for (int pass = 0; pass < passes; ++pass) {
        if (pass == 1) {                // the inner digest from the state after K ^ opad
            st.load(gptr(a.opad), 1);
#pragma unroll
            for (int k = 0; k < 16; ++k) w[k] = k < D / 4 ? dw[k] : 0u;
            rem = D & 63;
            if (D == 64) {              // a whole block, then an empty tail
                st.block(w, 512, T);
#pragma unroll
                for (int k = 0; k < 16; ++k) w[k] = 0u;
            }
        }
        st.finish(w, rem, T);
#pragma unroll
        for (int k = 0; k < D / 8; ++k) {   // the last D bytes of h (:1839)
            dw[2 * k] = (uint32_t)st.h[8 - D / 8 + k];
            dw[2 * k + 1] = (uint32_t)(st.h[8 - D / 8 + k] >> 32);
        }
    }
    store_digest<D>(gptr(a.digests) + i * D, dw);
    if (!a.keep)
        for (uint32_t k = 0; k < kGoWords; ++k) c[k * P] = gptr(a.init)[k];
}

template <bool k256>
__global__ __launch_bounds__(256) void gost_stream_prep_kernel(const uint8_t* key, uint64_t klen, uint32_t keyed,
                                                               uint32_t* init, uint32_t* opad) {
    __shared__ __attribute__((aligned(16))) uint64_t Timg[8 * 256];
    gost_stage_table(Timg);
    const GostFlat T{{}, Timg};
    if (threadIdx.x != 0) return;
    for (uint32_t k = 0; k < kGoWords; ++k) init[k] = 0u;
    GostStream st;
    st.init(k256);
    if (keyed) {
        using G = Gost<k256>;
        uint32_t kb[16], w[16];
        if (klen > 64) {                // gost3411-2012.h:1874-1878
            G t;
            t.init();
            gost_message(t, gptr(key), klen, T);
            uint32_t dw[G::kDigest / 4];
            t.digest_words(dw, T);
#pragma unroll
            for (int k = 0; k < 16; ++k) kb[k] = k < G::kDigest / 4 ? dw[k] : 0u;
        } else if (klen == 64) {
            load_full64(gptr(key), kb);
        } else {
            load_tail64(gptr(key), (uint32_t)klen, kb);
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] = kb[k] ^ 0x36363636u;
        st.block(w, 512, T);
        GostStream o;
        o.init(k256);
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] = kb[k] ^ 0x5c5c5c5cu;
        o.block(w, 512, T);
        o.save(opad, 1);
    }
    st.save(init, 1);
}

// ------------------------------------------------------------ launchers
static dim3 grid_of(uint64_t count) { return dim3((unsigned)((count + kThreads - 1) / kThreads)); }

void launch_stream_prep(int alg, const uint8_t* key, uint64_t key_len, bool keyed, uint32_t* init, uint32_t* opad,
                        hipStream_t s) {
    const uint32_t kd = keyed ? 1u : 0u;
#define LCB_PREP(K, T) hipLaunchKernelGGL(K, dim3(1), dim3(T), 0, s, key, key_len, kd, init, opad)
    switch (alg) {
    case LCB_HASH_MD5: LCB_PREP(stream_prep_kernel<Md5>, 64); break;
    case LCB_HASH_SHA1: LCB_PREP(stream_prep_kernel<Sha1>, 64); break;
    case LCB_HASH_SHA224: LCB_PREP(stream_prep_kernel<Sha256<true>>, 64); break;
    case LCB_HASH_SHA256: LCB_PREP(stream_prep_kernel<Sha256<false>>, 64); break;
    case LCB_HASH_SHA384: LCB_PREP(stream_prep_kernel<Sha512<true>>, 64); break;
    case LCB_HASH_SHA512: LCB_PREP(stream_prep_kernel<Sha512<false>>, 64); break;
    case LCB_HASH_GOST256: LCB_PREP(gost_stream_prep_kernel<true>, 256); break;
    case LCB_HASH_GOST512: LCB_PREP(gost_stream_prep_kernel<false>, 256); break;
    }
#undef LCB_PREP
}

void launch_stream_check(const StreamArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(stream_check_kernel, grid_of(a.count), dim3(kThreads), 0, s, a);
}

void launch_stream_fill(const StreamArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(stream_fill_kernel, grid_of(a.count), dim3(kThreads), 0, s, a);
}

void launch_stream_gather(const StreamArgs& a, uint32_t* image, hipStream_t s) {
    hipLaunchKernelGGL(stream_gather_kernel, grid_of(a.count), dim3(kThreads), 0, s, a, image);
}

void launch_stream_scatter(const StreamArgs& a, const uint32_t* image, hipStream_t s) {
    hipLaunchKernelGGL(stream_scatter_kernel, grid_of(a.count), dim3(kThreads), 0, s, a, image);
}

void launch_stream_update(int alg, const StreamArgs& a, hipStream_t s) {
    const dim3 g = grid_of(a.count), b(kThreads);
    switch (alg) {
    case LCB_HASH_MD5: hipLaunchKernelGGL(stream_update_kernel<Md5>, g, b, 0, s, a); break;
    case LCB_HASH_SHA1: hipLaunchKernelGGL(stream_update_kernel<Sha1>, g, b, 0, s, a); break;
    case LCB_HASH_SHA224:
    case LCB_HASH_SHA256: hipLaunchKernelGGL(stream_update_kernel<Sha256<false>>, g, b, 0, s, a); break;
    case LCB_HASH_SHA384:
    case LCB_HASH_SHA512: hipLaunchKernelGGL(stream_update_kernel<Sha512<false>>, g, b, 0, s, a); break;
    case LCB_HASH_GOST256:
    case LCB_HASH_GOST512: hipLaunchKernelGGL(gost_stream_update_kernel, g, b, 0, s, a); break;
    }
}

void launch_stream_final(int alg, const StreamArgs& a, hipStream_t s) {
    const dim3 g = grid_of(a.count), b(kThreads);
    switch (alg) {
    case LCB_HASH_MD5: hipLaunchKernelGGL(stream_final_kernel<Md5>, g, b, 0, s, a); break;
    case LCB_HASH_SHA1: hipLaunchKernelGGL(stream_final_kernel<Sha1>, g, b, 0, s, a); break;
    case LCB_HASH_SHA224: hipLaunchKernelGGL(stream_final_kernel<Sha256<true>>, g, b, 0, s, a); break;
    case LCB_HASH_SHA256: hipLaunchKernelGGL(stream_final_kernel<Sha256<false>>, g, b, 0, s, a); break;
    case LCB_HASH_SHA384: hipLaunchKernelGGL(stream_final_kernel<Sha512<true>>, g, b, 0, s, a); break;
    case LCB_HASH_SHA512: hipLaunchKernelGGL(stream_final_kernel<Sha512<false>>, g, b, 0, s, a); break;
    case LCB_HASH_GOST256: hipLaunchKernelGGL(gost_stream_final_kernel<true>, g, b, 0, s, a); break;
    case LCB_HASH_GOST512: hipLaunchKernelGGL(gost_stream_final_kernel<false>, g, b, 0, s, a); break;
    }
}

}  // namespace lcbstream
