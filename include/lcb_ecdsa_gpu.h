/*
 * lcb_ecdsa_gpu.h — batched ECDSA / GOST R 34.10 signature verification on
 * the MI355X (liblcb_ecdsa_gpu.so).
 *
 * The reference's verification (include/crypto/dsa/ecdsa.h) is header-only
 * and one signature per call:
 *
 *   ecdsa_verify_be(curve, hash, hash_size, sign_r, sign_s, sign_size,
 *                   pub_key_x, pub_key_y, pub_key_size)        ecdsa.h:1450-1486
 *   ecdsa_verify_le(...)                                       ecdsa.h:1487-1523
 *
 * lcb_ecdsa_verify_batch writes, for every item i, exactly the value the
 * reference returns for
 *
 *   ecdsa_verify_{be,le}(curve, hash_i, hash_size, r_i, s_i, 32, Qx, Qy, 32)
 *
 * with hash_i = hashes + i * hash_size, r_i = sigs + 64 i, s_i = r_i + 32 and
 * (Qx, Qy) = pub_keys + 64 k, k = key_idx ? key_idx[i] : i.  In the le form
 * every number (hash, r, s, Qx, Qy) is little-endian, as the reference
 * imports it.  status[i] is
 *
 *    0       the signature verifies
 *   -2       it does not (R.x mod n != r)
 *   -1       the public key is refused: x >= p, y >= p or y^2 != x^3 + a x + b;
 *            or u1 G + u2 Q is the point at infinity.  The key is checked
 *            first, so an off-curve key with r >= n is -1.
 *   EINVAL   r >= n or s >= n; s = 0 on an ECDSA curve (no inverse);
 *            key_idx[i] >= nkeys (no key is read)
 *
 * The hash number is the first min(hash_size, 32) bytes of hash_i.  A number
 * e >= n is replaced, as the reference's bn_mod_reduce does it, by
 * (e mod (n - 1)) + 1 — not by e mod n.  On the GOST curves e = 0 becomes 1.
 *
 * The reference also computes n Q for the public key (ecdsa.h:966,
 * elliptic_curve.h:2497-2510).  Every curve here has cofactor 1, where the
 * on-curve check implies n Q = O, so the result is the same without it.
 * Only the (x, y) key form is offered: the reference's compressed and packed
 * forms (a leading 02/03/04/06/07 byte) need a modular square root or are a
 * re-framing of (x, y) and are left to the caller.
 *
 * Curves: the ten 256-bit prime-field curves of the reference's table
 * (ecdsa.h:96-739), addressed by id or by the reference's name:
 *   0 secp256k1, 1 secp256r1, 2 brainpoolP256r1                     (ECDSA)
 *   3 id-GostR3410-2001-ParamSet-cc, 4 id-gostR3410-2001-Test_ParamSet,
 *   5..9 id-gostR3410-2001-CryptoPro-{A,B,C,XchA,XchB}-ParamSet     (GOST)
 *
 * Memory modes (flags): LCB_HASH_F_DEVICE (include/lcb_hash_gpu.h) — hashes,
 * sigs, pub_keys, key_idx and status are device pointers and the work is
 * enqueued on `stream` without waiting; 0 — host pointers, staged chunk by
 * chunk through page-locked memory, returns when status is written.
 * An unknown curve, hash_size outside 1..64, a NULL pointer with count > 0,
 * key_idx == NULL with nkeys != count, or count or nkeys above 2^32 - 1 are
 * EINVAL before the device is touched; count == 0 returns 0.  Errors: 0,
 * EINVAL, ENOMEM, ENODEV, EIO (no CPU fallback).
 */
#ifndef LCB_ECDSA_GPU_H
#define LCB_ECDSA_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LCB_ECDSA_ALGO_ECDSA	0	/* EC_CURVE_ALGO_ECDSA */
#define LCB_ECDSA_ALGO_GOST	1	/* EC_CURVE_ALGO_GOST20XX */

int		lcb_ecdsa_curve_count(void);
const char	*lcb_ecdsa_curve_name(int id);		/* NULL if unknown */
int		lcb_ecdsa_curve_id(const char *name);	/* -1 if unknown */
/* Test aid: p, a, b, Gx, Gy, n as 6 x 32 big-endian bytes, the algo
 * (LCB_ECDSA_ALGO_*) and the cofactor. */
int		lcb_ecdsa_curve_params(int id, uint8_t *out, uint32_t *algo,
		    uint32_t *h);

/* le: 0 = ecdsa_verify_be, != 0 = ecdsa_verify_le. */
int	lcb_ecdsa_verify_batch(int curve, int le, const uint8_t *hashes,
	    size_t hash_size, const uint8_t *sigs, const uint8_t *pub_keys,
	    size_t nkeys, const uint32_t *key_idx, size_t count,
	    int32_t *status, uint32_t flags, void *stream);

/* Reference-named entry points, batched. */
int	ecdsa_verify_be_batch(int curve, const uint8_t *hashes,
	    size_t hash_size, const uint8_t *sigs, const uint8_t *pub_keys,
	    size_t nkeys, const uint32_t *key_idx, size_t count,
	    int32_t *status, uint32_t flags, void *stream);
int	ecdsa_verify_le_batch(int curve, const uint8_t *hashes,
	    size_t hash_size, const uint8_t *sigs, const uint8_t *pub_keys,
	    size_t nkeys, const uint32_t *key_idx, size_t count,
	    int32_t *status, uint32_t flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LCB_ECDSA_GPU_H */
