/*
 * lcb_ecdsa_dh_gpu.h — batched ECDH key agreement on the MI355X
 * (liblcb_ecdsa_dh_gpu.so).  The third piece of the ECDSA / GOST R 34.10
 * family beside lcb_ecdsa_gpu.h (verification) and lcb_ecdsa_sign_gpu.h
 * (signing, key generation); the curve ids and names are the same
 * (0 secp256k1, 1 secp256r1, 2 brainpoolP256r1, 3..9 the GOST R 34.10-2001
 * sets; lcb_ecdsa_curve_id() of lcb_ecdsa_gpu.h maps the names).
 *
 * The reference (include/crypto/dsa/ecdsa.h) is header-only and one item per
 * call.  For every item i the batch call writes exactly the value the
 * reference returns, and on 0 exactly the 32 bytes it writes, for
 *
 *   ecdsa_dh_{be,le}(curve, use_cofactor, Qx, Qy, 32, d, 32, shared, &size)
 *                                                          ecdsa.h:1712-1824
 *
 * the x coordinate of d Q.  Every number is 32 bytes; le != 0 makes every
 * number little-endian, as the reference's _le form imports and exports them.
 * (Qx || Qy) = pub_keys + 64 k with k = pub_idx ? pub_idx[i] : i,
 * d = priv_keys + 32 j with j = priv_idx ? priv_idx[i] : i, the secret goes to
 * shared + 32 i.  A NULL index array means "item i uses entry i", and then
 * the table size must equal count.  A server that holds one private key and
 * sees many peers passes npriv = 1 and a priv_idx of zeros.  Buffers must not
 * overlap.  On any status but 0 the item's 32 output bytes are written as
 * zeros: the reference writes nothing there, zeros leave no stale secret.
 *
 * status[i], in the order of the checks:
 *   EINVAL   pub_idx[i] >= npub or priv_idx[i] >= npriv (checked before
 *            anything else; no key is read)
 *   -1       the public key is refused: x >= p, y >= p, or (x, y) not on the
 *            curve; (0, 0) is refused on every curve.  A refused key together
 *            with d >= n is -1, not EINVAL.
 *   EINVAL   d >= n
 *   -1       d = 0 (d Q is the point at infinity)
 *    0       the x coordinate of d Q written
 *   Every curve of the table has cofactor 1: use_cofactor multiplies d by
 *   h = 1, so the flag is accepted and both values give the same bytes.
 *
 * Secrets.  d Q is a binary double-and-add-always over all 256 bits of d.
 * Guaranteed: every loop has a fixed trip count, and no load address and no
 * branch of the multiplication is taken on a bit of d (the sum is kept or
 * dropped with a select).  NOT guaranteed: rejected items return early, and
 * the point addition branches on its exceptional cases, which are reached
 * only while the leading bits of d are zero (the sum so far is the point at
 * infinity) and in the last step of d = n - 1.  The library is not hardened
 * beyond that.  Host mode overwrites its staging buffers, page-locked and on
 * the device, with zeros after the last chunk, also after an error.
 *
 * Not offered: the compressed, packed and one-byte-infinity key forms and
 * ecdsa_pub_key_import / export_*, key recovery from a signature,
 * ecdsa_verify_priv_key_*, curves of other sizes (the 384- and 512-bit curves
 * have verification only: lcb_ecdsa_wide_gpu.h), a windowed variable-base
 * multiplication, and any key derivation beyond one digest of the secret
 * (liblcb_amd.ecdsa_dh.dh_digest).
 *
 * Memory modes (flags): LCB_HASH_F_DEVICE (include/lcb_hash_gpu.h) — every
 * pointer is a device pointer and the work is enqueued on `stream` without
 * waiting; 0 — host pointers, staged chunk by chunk through page-locked
 * memory, returns when the outputs are written.  An unknown curve, unknown
 * flag bits, a NULL pointer with count > 0, a NULL index with its table size
 * != count, or count, npub or npriv above 2^32 - 1 are EINVAL before the
 * device is touched; count == 0 returns 0.  Errors: 0, EINVAL, ENOMEM,
 * ENODEV, EIO (no CPU fallback).
 */
#ifndef LCB_ECDSA_DH_GPU_H
#define LCB_ECDSA_DH_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* le: 0 = the reference's _be form, != 0 = its _le form. */
int	lcb_ecdsa_dh_batch(int curve, int le, int use_cofactor,
	    const uint8_t *pub_keys, size_t npub, const uint32_t *pub_idx,
	    const uint8_t *priv_keys, size_t npriv, const uint32_t *priv_idx,
	    size_t count, uint8_t *shared, int32_t *status,
	    uint32_t flags, void *stream);

/* Reference-named entry points, batched. */
int	ecdsa_dh_be_batch(int curve, int use_cofactor,
	    const uint8_t *pub_keys, size_t npub, const uint32_t *pub_idx,
	    const uint8_t *priv_keys, size_t npriv, const uint32_t *priv_idx,
	    size_t count, uint8_t *shared, int32_t *status,
	    uint32_t flags, void *stream);
int	ecdsa_dh_le_batch(int curve, int use_cofactor,
	    const uint8_t *pub_keys, size_t npub, const uint32_t *pub_idx,
	    const uint8_t *priv_keys, size_t npriv, const uint32_t *priv_idx,
	    size_t count, uint8_t *shared, int32_t *status,
	    uint32_t flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LCB_ECDSA_DH_GPU_H */
