// radius_parse.hpp — the per-packet walk of the batched RADIUS sign/verify
// (include/lcb_radius_gpu.h): the structural guard, the first
// Message-Authenticator and User-Password, and the code tables that pick the
// authenticator each hash covers.  Plain C++ with no dependency but <errno.h>:
// the parse kernel (radius_kernels.hip) and a host program
// (tests/c/radius_parse_host.cpp, built with the host compiler's sanitizers)
// compile the same text.
//
// Line numbers are those of the reference's include/proto/radius.h.
#pragma once
#include <errno.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LCB_RAD_HD __host__ __device__ inline
#else
#define LCB_RAD_HD inline
#endif

namespace lcbrad {

constexpr uint32_t kHdrSize = 20;          // RADIUS_PKT_HDR_SIZE
constexpr uint32_t kPktMax = 4096;         // RADIUS_PKT_MAX_SIZE
constexpr uint32_t kAttrUserPassword = 2;  // radius.h:70
constexpr uint32_t kAttrMsgAuthentic = 80; // radius.h:232
constexpr uint32_t kPwMax = 128;           // RADIUS_A_T_USER_PASSWORD_MAX_LEN

// What the walk leaves per packet.  A nonzero err zeroes every other field:
// such a packet takes part in no later step.
struct RadRec {
    int32_t err;      // 0, EBADMSG (structure) or EINVAL (key index)
    uint32_t len;     // the packet's Length field
    uint32_t ma_off;  // first Message-Authenticator attribute (0: none)
    uint32_t ma_len;  // its len byte
    uint32_t pw_off;  // first User-Password attribute (0: none)
    uint32_t pw_len;  // its data bytes (len byte - 2)
    uint32_t kidx;    // the key index used (0 where the caller's was refused)
    uint32_t aux;     // verify: the plan (rad_verify_plan)
};

// The structural part of radius_pkt_chk (radius.h:1253-1256, 1280-1284), the
// find walk's checks (:715-720) over the WHOLE attribute list, and both
// attribute lookups in the same pass.  Reads p[2..3] only when buf_size >= 20
// and nothing at or past min(Length, buf_size).
LCB_RAD_HD void rad_parse(const uint8_t* p, uint32_t buf_size, uint32_t key_index, uint32_t nkeys, RadRec* r) {
    r->err = EBADMSG;
    r->len = r->ma_off = r->ma_len = r->pw_off = r->pw_len = r->kidx = r->aux = 0;
    if (buf_size < kHdrSize) return;
    const uint32_t len = ((uint32_t)p[2] << 8) | p[3];
    if (len < kHdrSize || len > buf_size || len > kPktMax) return;
    uint32_t ma_off = 0, ma_len = 0, pw_off = 0, pw_len = 0;
    uint32_t i = kHdrSize;
    while (i < len) {
        if (len - i < 2) return;               // no attribute header
        const uint32_t t = p[i], n = p[i + 1];
        if (n > len - i) return;               // runs past Length
        if (t == 0 || n < 2) return;           // bad attribute
        if (t == kAttrMsgAuthentic && ma_off == 0) {
            ma_off = i;
            ma_len = n;
        }
        if (t == kAttrUserPassword && pw_off == 0) {
            pw_off = i;
            pw_len = n - 2;
        }
        i += n;
    }
    if (key_index >= nkeys) {
        r->err = EINVAL;
        return;
    }
    r->err = 0;
    r->len = len;
    r->ma_off = ma_off;
    r->ma_len = ma_len;
    r->pw_off = pw_off;
    r->pw_len = pw_len;
    r->kidx = key_index;
}

// Codes whose authenticator is random data (radius.h:871-873, 1323-1325).
LCB_RAD_HD bool rad_random_auth(uint32_t code) { return code == 1 || code == 12 || code == 13; }
// Accounting-Request, Disconnect-Request, CoA-Request (radius.h:883-885, 1339-1341).
LCB_RAD_HD bool rad_zero_auth(uint32_t code) { return code == 4 || code == 40 || code == 43; }
// Access-Accept/-Reject/-Challenge, Disconnect-ACK/-NAK, CoA-ACK/-NAK (radius.h:889-895).
LCB_RAD_HD bool rad_reply_auth(uint32_t code) {
    return code == 2 || code == 3 || code == 11 || code == 41 || code == 42 || code == 44 || code == 45;
}

// radius_pkt_sign's checks that need no hash (add_msg_authr = 0): the
// User-Password as radius_pkt_attr_password_encode sees it with buf_size =
// password_len (radius.h:752-765), then the Message-Authenticator's length
// (:858).  0 or the error radius_pkt_sign returns.
LCB_RAD_HD int32_t rad_sign_static(const RadRec& r) {
    if (r.pw_off) {
        if (r.pw_len > kPwMax) return EINVAL;
        if (r.pw_len == 0 || (r.pw_len & 15u)) return EOVERFLOW;
    }
    if (r.ma_off && r.ma_len != 18) return EBADMSG;
    return 0;
}

// The plan of radius_pkt_verify for one packet: per step the error known
// without a hash and the authenticator the hash covers.
enum : uint32_t { kAuthOwn = 0, kAuthZero = 1, kAuthReq = 2 };
constexpr uint32_t kPlanMa = 1u << 24;    // step 1 hashes (HMAC pass)
constexpr uint32_t kPlanAu = 1u << 25;    // step 2 hashes (suffix pass)
constexpr uint32_t kPlanPw = 1u << 26;    // step 3 decodes
constexpr uint32_t kPlanMaBad = 1u << 27; // set later: the HMAC differed
LCB_RAD_HD uint32_t plan_e1(uint32_t aux) { return aux & 0xffu; }
LCB_RAD_HD uint32_t plan_e2(uint32_t aux) { return (aux >> 8) & 0xffu; }
LCB_RAD_HD uint32_t plan_e3(uint32_t aux) { return (aux >> 16) & 0xffu; }
LCB_RAD_HD uint32_t plan_ma_auth(uint32_t aux) { return (aux >> 28) & 3u; }
LCB_RAD_HD uint32_t plan_au_auth(uint32_t aux) { return (aux >> 30) & 3u; }

// code: the packet's; req_code: the request's code byte, 0 = pkt_req NULL.
LCB_RAD_HD uint32_t rad_verify_plan(const RadRec& r, uint32_t code, uint32_t req_code) {
    uint32_t e1 = 0, e2 = 0, e3 = 0, ma_auth = kAuthOwn, au_auth = kAuthOwn, flags = 0;
    // 1. Message-Authenticator, authenticator outside (radius.h:858, 870-905).
    if (r.ma_off) {
        if (r.ma_len != 18) {
            e1 = EBADMSG;
        } else if (rad_random_auth(code)) {
            ma_auth = kAuthOwn;
        } else if (code == 5 && req_code == 12) {
            ma_auth = kAuthReq;
        } else if (code == 5 || rad_zero_auth(code)) {
            ma_auth = kAuthZero;
        } else if (rad_reply_auth(code)) {
            if (req_code == 0) e1 = EINVAL;
            ma_auth = kAuthReq;
        } else {
            e1 = EBADMSG;
        }
        if (!e1) flags |= kPlanMa;
    }
    // 2. Authenticator (radius.h:1388-1398 over 1338-1374).
    if (!rad_random_auth(code)) {
        if (rad_zero_auth(code)) {
            au_auth = kAuthZero;
        } else if (rad_reply_auth(code) || code == 5) {
            if (req_code == 0) e2 = EINVAL;
            au_auth = kAuthReq;
        } else {
            e2 = EINVAL;
        }
        if (!e1 && !e2) flags |= kPlanAu;
    }
    // 3. User-Password decode (radius.h:802-808).
    if (r.pw_off) {
        if (r.pw_len == 0 || r.pw_len > kPwMax || (r.pw_len & 15u)) e3 = EINVAL;
        if (!e1 && !e2 && !e3) flags |= kPlanPw;
    }
    return e1 | (e2 << 8) | (e3 << 16) | flags | (ma_auth << 28) | (au_auth << 30);
}

}  // namespace lcbrad
