/*
 * lcb_ecdsa_wide_sign_gpu.h — batched ECDSA / GOST R 34.10-2012 signing, key
 * generation and public keys from private keys on the 384- and 512-bit
 * curves, on the MI355X (liblcb_ecdsa_wide_sign_gpu.so).  The other half of
 * lcb_ecdsa_wide_gpu.h, which verifies; curve ids and names are the same
 * (0 secp384r1, 1 brainpoolP384r1, 2 brainpoolP512r1, 3..5 the
 * id-tc26-gost-3410-12-512 sets), and B = lcb_ecdsa_wide_curve_bytes(id) is 48
 * for ids 0 and 1 and 64 for ids 2..5.  The 256-bit curves are
 * lcb_ecdsa_sign_gpu.h's.
 *
 * The reference (include/crypto/dsa/ecdsa.h) is header-only and one item per
 * call.  For every item i the batch calls write exactly the value the
 * reference returns, and on 0 exactly the bytes it writes, for
 *
 *   ecdsa_sign_{be,le}(curve, hash_i, hash_size, d, B, rnd_i, B, r, s, NULL)
 *   ecdsa_key_gen_{be,le}(curve, rnd_i, B, 0, d, NULL, x, y, &size)
 *   ecdsa_recover_pub_key_from_priv_key_{be,le}(curve, d, B, 0, x, y, &size)
 *
 * Every number is B bytes; le != 0 makes every number little-endian, as the
 * reference's _le forms import and export them.  hash_i = hashes +
 * i * hash_size, rnd_i = rnd + B i, d = priv_keys + B k with
 * k = key_idx ? key_idx[i] : i; sigs holds r || s (2 B bytes per item),
 * pub_keys holds x || y (2 B bytes per item), which is what
 * lcb_ecdsa_wide_verify_batch takes.  Buffers must not overlap.
 * On any status but 0 the item's outputs (r || s; d, x || y) are written as
 * zeros: the reference writes nothing there, zeros leave no stale secret.
 *
 * Signing, status[i] (the 256-bit contract; the reference says nothing else
 * at these widths, tests/golden/ecdsa_wide_sign.json records it):
 *    0       r || s written
 *   EINVAL   d >= n (checked before anything else: d = n with rnd = 0 is
 *            EINVAL); key_idx[i] >= nkeys (no key is read).  d = 0 is accepted.
 *   -1       k = 0; r = (k G).x mod n = 0 (no curve here has Gx = 0, so no
 *            input that can be exhibited ends there); s = 0
 *   The nonce is k = bn_mod_reduce(rnd): rnd itself below n, else
 *   (rnd mod (n - 1)) + 1, so rnd = n signs with k = 2.  The hash number e is
 *   the first min(hash_size, B) bytes of hash_i, reduced the same way;
 *   hash_size is 1..128 as in the wide verification.
 *   ECDSA: s = k^-1 (e + r d).  GOST: s = k e + r d with e = 0 taken as 1.
 *   As in the reference the caller supplies rnd.  It MUST come from a
 *   cryptographic random generator and MUST never repeat for a key: two
 *   signatures of one key with one nonce give the key away.
 *
 * Key generation: d = bn_mod_reduce(rnd_i), Q = d G; priv_keys receives the
 * reduced d.  rnd = 0 is -1; rnd = n gives d = 2.
 * Public key from private key: Q = d G; d >= n is EINVAL, d = 0 is -1.
 *
 * The fixed-base multiple runs over a 4-bit window table of G (8 L x 15
 * affine points for L = B / 4 limbs: 138,240 bytes at B = 48 and 245,760
 * bytes at B = 64, per curve), derived on the host once per process and curve
 * and uploaded once per device and curve.  That first use of a curve on a
 * device is a one-time BLOCKING copy, in device mode too (do it outside a
 * stream capture); the table stays for the life of the process.
 *
 * Secrets.  Guaranteed: no load address depends on a secret (every window
 * reads all 15 entries through lane-uniform addresses and picks one with
 * selects; digit 0 adds an entry and drops the sum with a select), and every
 * loop has a fixed trip count.  NOT guaranteed: rejected items return early,
 * and the point addition branches on its exceptional cases (P = O, P = T,
 * P = -T).  The library is not hardened beyond that.  Host mode overwrites
 * its staging buffers, page-locked and on the device, with zeros after the
 * last chunk, also after an error.
 *
 * Not offered on these curves: ECDH, key import and export (the compressed
 * and packed key forms).
 *
 * Memory modes (flags): LCB_HASH_F_DEVICE (include/lcb_hash_gpu.h) — every
 * pointer is a device pointer and the work is enqueued on `stream` without
 * waiting; 0 — host pointers, staged chunk by chunk through page-locked
 * memory, returns when the outputs are written.  An unknown curve, hash_size
 * outside 1..128, unknown flag bits, a NULL pointer with count > 0,
 * key_idx == NULL with nkeys != count, or count or nkeys above 2^32 - 1 are
 * EINVAL before the device is touched; count == 0 returns 0.  Errors: 0,
 * EINVAL, ENOMEM, ENODEV, EIO (no CPU fallback).
 */
#ifndef LCB_ECDSA_WIDE_SIGN_GPU_H
#define LCB_ECDSA_WIDE_SIGN_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* le: 0 = the reference's _be form, != 0 = its _le form. */
int	lcb_ecdsa_wide_sign_batch(int curve, int le, const uint8_t *hashes,
	    size_t hash_size, const uint8_t *priv_keys, size_t nkeys,
	    const uint32_t *key_idx, const uint8_t *rnd, size_t count,
	    uint8_t *sigs, int32_t *status, uint32_t flags, void *stream);
int	lcb_ecdsa_wide_key_gen_batch(int curve, int le, const uint8_t *rnd,
	    size_t count, uint8_t *priv_keys, uint8_t *pub_keys,
	    int32_t *status, uint32_t flags, void *stream);
int	lcb_ecdsa_wide_pub_key_batch(int curve, int le,
	    const uint8_t *priv_keys, size_t count, uint8_t *pub_keys,
	    int32_t *status, uint32_t flags, void *stream);

/* Reference-named entry points, batched. */
int	ecdsa_sign_be_wide_batch(int curve, const uint8_t *hashes,
	    size_t hash_size, const uint8_t *priv_keys, size_t nkeys,
	    const uint32_t *key_idx, const uint8_t *rnd, size_t count,
	    uint8_t *sigs, int32_t *status, uint32_t flags, void *stream);
int	ecdsa_sign_le_wide_batch(int curve, const uint8_t *hashes,
	    size_t hash_size, const uint8_t *priv_keys, size_t nkeys,
	    const uint32_t *key_idx, const uint8_t *rnd, size_t count,
	    uint8_t *sigs, int32_t *status, uint32_t flags, void *stream);
int	ecdsa_key_gen_be_wide_batch(int curve, const uint8_t *rnd, size_t count,
	    uint8_t *priv_keys, uint8_t *pub_keys, int32_t *status,
	    uint32_t flags, void *stream);
int	ecdsa_key_gen_le_wide_batch(int curve, const uint8_t *rnd, size_t count,
	    uint8_t *priv_keys, uint8_t *pub_keys, int32_t *status,
	    uint32_t flags, void *stream);
int	ecdsa_recover_pub_key_from_priv_key_be_wide_batch(int curve,
	    const uint8_t *priv_keys, size_t count, uint8_t *pub_keys,
	    int32_t *status, uint32_t flags, void *stream);
int	ecdsa_recover_pub_key_from_priv_key_le_wide_batch(int curve,
	    const uint8_t *priv_keys, size_t count, uint8_t *pub_keys,
	    int32_t *status, uint32_t flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LCB_ECDSA_WIDE_SIGN_GPU_H */
