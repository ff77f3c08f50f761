/*
 * lcb_ecdsa_wide_gpu.h — batched ECDSA / GOST R 34.10-2012 signature
 * verification on the 384- and 512-bit curves, on the MI355X
 * (liblcb_ecdsa_wide_gpu.so).  The 256-bit curves are lcb_ecdsa_gpu.h's.
 *
 * The reference's verification (include/crypto/dsa/ecdsa.h) is header-only
 * and one signature per call:
 *
 *   ecdsa_verify_be(curve, hash, hash_size, sign_r, sign_s, sign_size,
 *                   pub_key_x, pub_key_y, pub_key_size)        ecdsa.h:1450-1486
 *   ecdsa_verify_le(...)                                       ecdsa.h:1487-1523
 *
 * Let B = (m + 7) / 8 be the curve's number size, 48 or 64 bytes
 * (lcb_ecdsa_wide_curve_bytes).  lcb_ecdsa_wide_verify_batch writes, for
 * every item i, exactly the value the reference returns for
 *
 *   ecdsa_verify_{be,le}(curve, hash_i, hash_size, r_i, s_i, B, Qx, Qy, B)
 *
 * with hash_i = hashes + i * hash_size, r_i = sigs + 2 B i, s_i = r_i + B and
 * (Qx, Qy) = pub_keys + 2 B k, k = key_idx ? key_idx[i] : i.  In the le form
 * every number (hash, r, s, Qx, Qy) is little-endian, as the reference
 * imports it.  status[i] is
 *
 *    0       the signature verifies
 *   -2       it does not (R.x mod n != r)
 *   -1       the public key is refused: x >= p, y >= p or y^2 != x^3 + a x + b;
 *            or u1 G + u2 Q is the point at infinity (on a GOST curve
 *            r = s = 0 ends here).  The key is checked first, so an off-curve
 *            key with r >= n is -1.
 *   EINVAL   r >= n or s >= n; s = 0 on an ECDSA curve (no inverse);
 *            key_idx[i] >= nkeys (no key is read)
 *
 * The hash number is the first min(hash_size, B) bytes of hash_i.  A number
 * e >= n is replaced, as the reference's bn_mod_reduce does it, by
 * (e mod (n - 1)) + 1 — not by e mod n.  On the GOST curves e = 0 becomes 1.
 *
 * The reference also computes n Q for the public key.  Every curve here has
 * cofactor 1, where the on-curve check implies n Q = O, so the result is the
 * same without it.
 *
 * Curves, addressed by id or by the reference's name (ecdsa.h:96-739):
 *   0 secp384r1, 1 brainpoolP384r1                     (ECDSA, B = 48)
 *   2 brainpoolP512r1                                  (ECDSA, B = 64)
 *   3 id-tc26-gost-3410-12-512-paramSetA,
 *   4 id-tc26-gost-3410-12-512-paramSetB,
 *   5 id-tc26-gost-3410-2012-512-paramSetTest          (GOST,  B = 64)
 * The digests they pair with are SHA-384 (secp384r1, be), SHA-512
 * (brainpoolP512r1, be) and GOST R 34.11-2012 512 (the tc26 sets, le).
 *
 * Signing, key generation and public keys from private keys on these curves
 * are lcb_ecdsa_wide_sign_gpu.h's (liblcb_ecdsa_wide_sign_gpu.so).  Not
 * offered: ECDH, key import and export (the compressed and packed key forms)
 * on these curves; the reference's 320- and 521-bit curves and its curves
 * below 256 bits.
 *
 * Memory modes (flags): LCB_HASH_F_DEVICE (include/lcb_hash_gpu.h) — hashes,
 * sigs, pub_keys, key_idx and status are device pointers and the work is
 * enqueued on `stream` without waiting; 0 — host pointers, staged chunk by
 * chunk through page-locked memory, returns when status is written.
 * An unknown curve, hash_size outside 1..128, a NULL pointer with count > 0,
 * key_idx == NULL with nkeys != count, or count or nkeys above 2^32 - 1 are
 * EINVAL before the device is touched; count == 0 returns 0.  Errors: 0,
 * EINVAL, ENOMEM, ENODEV, EIO (no CPU fallback).
 */
#ifndef LCB_ECDSA_WIDE_GPU_H
#define LCB_ECDSA_WIDE_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LCB_ECDSA_WIDE_ALGO_ECDSA	0	/* EC_CURVE_ALGO_ECDSA */
#define LCB_ECDSA_WIDE_ALGO_GOST	1	/* EC_CURVE_ALGO_GOST20XX */

int		lcb_ecdsa_wide_curve_count(void);
const char	*lcb_ecdsa_wide_curve_name(int id);	/* NULL if unknown */
int		lcb_ecdsa_wide_curve_id(const char *name);	/* -1 if unknown */
int		lcb_ecdsa_wide_curve_bytes(int id);	/* B: 48 or 64; -1 if unknown */
/* Test aid: p, a, b, Gx, Gy, n as 6 x B big-endian bytes, the algo
 * (LCB_ECDSA_WIDE_ALGO_*) and the cofactor. */
int		lcb_ecdsa_wide_curve_params(int id, uint8_t *out, uint32_t *algo,
		    uint32_t *h);

/* le: 0 = ecdsa_verify_be, != 0 = ecdsa_verify_le. */
int	lcb_ecdsa_wide_verify_batch(int curve, int le, const uint8_t *hashes,
	    size_t hash_size, const uint8_t *sigs, const uint8_t *pub_keys,
	    size_t nkeys, const uint32_t *key_idx, size_t count,
	    int32_t *status, uint32_t flags, void *stream);

/* Reference-named entry points, batched. */
int	ecdsa_verify_be_wide_batch(int curve, const uint8_t *hashes,
	    size_t hash_size, const uint8_t *sigs, const uint8_t *pub_keys,
	    size_t nkeys, const uint32_t *key_idx, size_t count,
	    int32_t *status, uint32_t flags, void *stream);
int	ecdsa_verify_le_wide_batch(int curve, const uint8_t *hashes,
	    size_t hash_size, const uint8_t *sigs, const uint8_t *pub_keys,
	    size_t nkeys, const uint32_t *key_idx, size_t count,
	    int32_t *status, uint32_t flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LCB_ECDSA_WIDE_GPU_H */
