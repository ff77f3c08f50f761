// radius_kernels.hip — the device side of the batched RADIUS sign/verify
// (include/lcb_radius_gpu.h) around the keyed MD5 batches of
// liblcb_hash_gpu.so.  One lane per packet in every kernel:
//
//   radius_parse_kernel     the walk of radius_parse.hpp, the step plan, the
//                           lengths of the two keyed passes (0 = not in that
//                           pass) and, for verify, the field substitution of
//                           the HMAC pass with the originals parked aside
//   radius_password_kernel  User-Password hiding (radius.h:774-789, 821-836):
//                           MD5(secret || c_{j-1}) chained per packet
//   radius_mid_kernel       between the HMAC and the suffix pass: store or
//                           compare the Message-Authenticator, substitute the
//                           authenticator of the suffix pass
//   radius_fin_kernel       store or compare the authenticator, put parked
//                           bytes back, merge the error of every step
//
// Substitution is in place: no packet byte moves, 32 bytes per packet are
// parked.  The parse walk is a serial chain of dependent byte loads per lane
// (an attribute's length byte gives the next attribute's address), so these
// kernels are latency-bound: small registers, 256-lane blocks, as many waves
// in flight as the packets give.  None of them uses LDS or scratch.
#include <hip/hip_runtime.h>

#include "hash_device.hpp"
#include "radius_internal.hpp"

namespace lcbrad {

using lcbgpu::gptr;
using lcbgpu::Md5;

namespace {

// 16 bytes at any alignment as 4 raw LE words.
__device__ __forceinline__ uint4 ld16(const uint8_t* p) {
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        w[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) |
               ((uint32_t)p[4 * k + 3] << 24);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ void st16(uint8_t* p, uint4 v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) p[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
}

// Nonzero iff the 16 bytes differ; every word takes part whatever the first
// difference is (the reference compares with timingsafe_bcmp).
__device__ __forceinline__ uint32_t diff16(uint4 a, uint4 b) {
    return (a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w);
}

__device__ __forceinline__ uint8_t* pkt_at(const RadArgs& a, uint64_t i) {
    return gptr(a.pkts) + (a.offsets ? gptr(a.offsets)[i] : i * a.stride);
}

__device__ __forceinline__ void store_auth(uint8_t* p, uint32_t mode, const uint8_t* req) {
    if (mode == kAuthZero) st16(p + 4, make_uint4(0u, 0u, 0u, 0u));
    if (mode == kAuthReq) st16(p + 4, ld16(req + 4));
}

}  // namespace

template <bool kSign>
__global__ __launch_bounds__(256) void radius_parse_kernel(RadArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.count) return;
    uint8_t* p = pkt_at(a, i);
    const uint32_t bs = a.buf_sizes ? gptr(a.buf_sizes)[i] : a.fixed_size;
    const uint32_t ki = a.key_index ? gptr(a.key_index)[i] : 0u;
    RadRec r;
    rad_parse(p, bs, ki, a.nkeys, &r);
    uint32_t lm = 0, la = 0;
    if (kSign) {
        if (!r.err) r.err = rad_sign_static(r);
        if (!r.err) {
            lm = r.ma_off ? r.len : 0u;
            la = rad_random_auth(p[0]) ? 0u : r.len;
        }
    } else if (!r.err) {
        const uint8_t* req = a.req_hdrs ? gptr(a.req_hdrs) + 20 * i : nullptr;
        r.aux = rad_verify_plan(r, p[0], req ? (uint32_t)req[0] : 0u);
        if (r.aux & (kPlanMa | kPlanAu)) gptr(a.park)[2 * i] = ld16(p + 4);
        if (r.aux & kPlanMa) {
            // The HMAC pass reads the packet with the Message-Authenticator
            // zeroed and the authenticator of radius.h:870-905.
            gptr(a.park)[2 * i + 1] = ld16(p + r.ma_off + 2);
            st16(p + r.ma_off + 2, make_uint4(0u, 0u, 0u, 0u));
            store_auth(p, plan_ma_auth(r.aux), req);
            lm = r.len;
        }
        if (r.aux & kPlanAu) la = r.len;
    }
    gptr(a.rec)[i] = r;
    gptr(a.len_ma)[i] = lm;
    gptr(a.len_au)[i] = la;
    gptr(a.kidx)[i] = r.kidx;
}

template <bool kSign>
__global__ __launch_bounds__(256) void radius_password_kernel(RadArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.count) return;
    const RadRec r = gptr(a.rec)[i];
    if (r.err) return;
    uint8_t* p = pkt_at(a, i);
    if (kSign) {
        if (r.ma_off) st16(p + r.ma_off + 2, make_uint4(0u, 0u, 0u, 0u));
    } else if (gptr(a.errors)[i] != 0) {
        return;
    }
    if (!r.pw_off) return;
    const uint8_t* K = gptr(a.keys) + gptr(a.key_off)[r.kidx];
    const uint64_t kl = gptr(a.key_len)[r.kidx];
    uint8_t* pw = p + r.pw_off + 2;
    const uint32_t nb = r.pw_len >> 4;
    // Block j is XORed with MD5(secret || c_{j-1}), c_{-1} = the packet's own
    // authenticator.  Encoding writes c_j before link j + 1 reads it; decoding
    // runs from the last block down, so c_{j-1} is still in place when link j
    // reads it.
    for (uint32_t n = 0; n < nb; ++n) {
        const uint32_t j = kSign ? n : nb - 1 - n;
        const uint8_t* prev = j ? pw + 16 * (j - 1) : p + 4;
        Md5 st;
        st.init();
        lcbgpu::md_message2(st, K, kl, prev, 16, 0);
        uint32_t dw[4];
        st.digest_words(dw);
        const uint4 c = ld16(pw + 16 * j);
        st16(pw + 16 * j, make_uint4(c.x ^ dw[0], c.y ^ dw[1], c.z ^ dw[2], c.w ^ dw[3]));
    }
}

template <bool kSign>
__global__ __launch_bounds__(256) void radius_mid_kernel(RadArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.count) return;
    const RadRec r = gptr(a.rec)[i];
    if (r.err) return;
    uint8_t* p = pkt_at(a, i);
    if (kSign) {
        if (r.ma_off) st16(p + r.ma_off + 2, gptr(a.dig)[i]);
        return;
    }
    if (r.aux & kPlanMa) {
        const uint4 have = gptr(a.park)[2 * i + 1];
        if (diff16(have, gptr(a.dig)[i])) gptr(a.rec)[i].aux = r.aux | kPlanMaBad;
        st16(p + r.ma_off + 2, have);
    }
    if (r.aux & kPlanAu) store_auth(p, plan_au_auth(r.aux), a.req_hdrs ? gptr(a.req_hdrs) + 20 * i : nullptr);
}

template <bool kSign>
__global__ __launch_bounds__(256) void radius_fin_kernel(RadArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.count) return;
    const RadRec r = gptr(a.rec)[i];
    int32_t e = r.err;
    if (kSign) {
        if (!e && gptr(a.len_au)[i]) st16(pkt_at(a, i) + 4, gptr(a.dig)[i]);
    } else if (!e) {
        uint4 own = make_uint4(0u, 0u, 0u, 0u);
        if (r.aux & (kPlanMa | kPlanAu)) {
            own = gptr(a.park)[2 * i];
            st16(pkt_at(a, i) + 4, own);
        }
        // The first failing step decides (radius.h:1545-1565).
        e = (int32_t)plan_e1(r.aux);
        if (!e && (r.aux & kPlanMaBad)) e = EBADMSG;
        if (!e) e = (int32_t)plan_e2(r.aux);
        if (!e && (r.aux & kPlanAu) && diff16(own, gptr(a.dig)[i])) e = EBADMSG;
        if (!e) e = (int32_t)plan_e3(r.aux);
    }
    gptr(a.errors)[i] = e;
}

namespace {
dim3 grid_of(uint64_t count) { return dim3((unsigned)((count + 255) / 256)); }
}  // namespace

#define LCB_RAD_LAUNCH(fn, kernel)                                                        \
    void fn(const RadArgs& a, bool sign, hipStream_t s) {                                 \
        if (sign)                                                                         \
            hipLaunchKernelGGL((kernel<true>), grid_of(a.count), dim3(256), 0, s, a);     \
        else                                                                              \
            hipLaunchKernelGGL((kernel<false>), grid_of(a.count), dim3(256), 0, s, a);    \
    }
LCB_RAD_LAUNCH(launch_radius_parse, radius_parse_kernel)
LCB_RAD_LAUNCH(launch_radius_password, radius_password_kernel)
LCB_RAD_LAUNCH(launch_radius_mid, radius_mid_kernel)
LCB_RAD_LAUNCH(launch_radius_fin, radius_fin_kernel)
#undef LCB_RAD_LAUNCH

}  // namespace lcbrad
