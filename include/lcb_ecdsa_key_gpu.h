/*
 * lcb_ecdsa_key_gpu.h — batched public-key import and export on the MI355X
 * (liblcb_ecdsa_key_gpu.so).  The fourth piece of the ECDSA / GOST R 34.10
 * family beside lcb_ecdsa_gpu.h (verification), lcb_ecdsa_sign_gpu.h
 * (signing, key generation) and lcb_ecdsa_dh_gpu.h (key agreement); the curve
 * ids and names are the same (0 secp256k1, 1 secp256r1, 2 brainpoolP256r1,
 * 3..9 the GOST R 34.10-2001 sets; lcb_ecdsa_curve_id() of lcb_ecdsa_gpu.h
 * maps the names).  Those three take and give public keys only as x || y,
 * 32 bytes each: this library turns the wire forms into that and back.
 *
 * The reference (include/crypto/dsa/ecdsa.h) is header-only and one key per
 * call.  Every number is 32 bytes; le != 0 makes every number little-endian,
 * as the reference's _le forms import and export them.  The prefix byte of a
 * form is its first byte in both byte orders.  Buffers must not overlap.
 *
 * Import.  For every item i the call writes exactly the value the reference
 * returns for
 *
 *   ecdsa_pub_key_import_{be,le}(curve, key, key_y, size, &point)
 *                                                          ecdsa.h:939-1071
 *
 * with key = keys + i key_stride, size = sizes ? sizes[i] : key_size and
 * key_y = keys_y ? keys_y + 32 i : NULL, and on 0 at pub_keys + 64 i the x || y
 * that the reference's export of the imported point writes, in the byte order
 * of the form.  For the point at infinity (status 0) the 64 bytes are zeros
 * and infinity[i] = 1; on every other status the 64 bytes are zeros and
 * infinity[i] = 0.  infinity may be NULL.  (0, 0) is refused by all three
 * sibling libraries, so a table of imported keys can go to them unfiltered,
 * the statuses beside it.
 *
 * status[i], in the order of the checks:
 *   EINVAL   size > key_stride (no key byte is read), or size = 0
 *   size 1   key[0] = 0: the point at infinity, 0; else EINVAL
 *   size 32  x = key, y = key_y: EINVAL where keys_y is NULL; -1 where the key
 *            is refused; else 0
 *   size 33  compressed, prefix 2 or 3, then x: -1 for any other prefix, for
 *            x >= p, and where x^3 + a x + b has no square root; else 0 with
 *            the root y whose lowest bit is prefix & 1
 *   size 65  packed, prefix 4, 6 or 7, then x, then y: -1 for any other
 *            prefix and where the key is refused; else 0.  The prefixes 6 and
 *            7 are NOT compared with the parity of y, as in the reference
 *   size 64  x, then y, no prefix: -1 where the key is refused; else 0
 *   -1       every other size
 *   "Refused": x >= p, y >= p, or (x, y) not on the curve.  Every curve of
 *   the table has cofactor 1, so the reference's n Q = O follows.
 *
 * Export.  For every item i what
 *
 *   ecdsa_pub_key_export_{be,le}(curve, compress, &point, out, NULL, &size)
 *                                                          ecdsa.h:837-924
 *
 * writes for the point (x, y) = pub_keys + 64 i, or for the point at infinity
 * where infinity && infinity[i]: at out + i out_stride one zero byte for the
 * point at infinity, (2 | y & 1) || x compressed, 4 || x || y packed, and its
 * size (1, 33, 65) in out_sizes[i].  Nothing is validated, as in the
 * reference; status[i] is 0.  No byte past an item's size is written.
 *
 * Not offered: the export into separate x and y buffers (a copy), key
 * recovery from a signature, curves of other sizes, and a check of the hybrid
 * prefixes against y.
 *
 * Memory modes (flags): LCB_HASH_F_DEVICE (include/lcb_hash_gpu.h) — every
 * pointer is a device pointer and the work is enqueued on `stream` without
 * waiting; 0 — host pointers, staged through page-locked memory in chunks of
 * at most 2^18 items, returns when the outputs are written.  An unknown
 * curve, unknown flag bits, an unknown form, a NULL keys, pub_keys, out,
 * out_sizes or status with count > 0, out_stride below the size of the form,
 * or count, key_stride or out_stride above 2^32 - 1 are EINVAL before the
 * device is touched; count == 0 returns 0.  Errors: 0, EINVAL, ENOMEM,
 * ENODEV, EIO (no CPU fallback).  Public keys are no secrets: the staging
 * buffers are not wiped.
 */
#ifndef LCB_ECDSA_KEY_GPU_H
#define LCB_ECDSA_KEY_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* form of lcb_ecdsa_key_export_batch */
#define LCB_ECDSA_KEY_PACKED		0	/* 04 || x || y, 65 bytes */
#define LCB_ECDSA_KEY_COMPRESSED	1	/* 02 / 03 || x, 33 bytes */

/* le: 0 = the reference's _be form, != 0 = its _le form. */
int	lcb_ecdsa_key_import_batch(int curve, int le,
	    const uint8_t *keys, size_t key_stride, const uint32_t *sizes,
	    size_t key_size, const uint8_t *keys_y, size_t count,
	    uint8_t *pub_keys, uint8_t *infinity, int32_t *status,
	    uint32_t flags, void *stream);
int	lcb_ecdsa_key_export_batch(int curve, int le, int form,
	    const uint8_t *pub_keys, const uint8_t *infinity, size_t count,
	    uint8_t *out, size_t out_stride, uint32_t *out_sizes,
	    int32_t *status, uint32_t flags, void *stream);

/* Reference-named entry points, batched. */
int	ecdsa_pub_key_import_be_batch(int curve,
	    const uint8_t *keys, size_t key_stride, const uint32_t *sizes,
	    size_t key_size, const uint8_t *keys_y, size_t count,
	    uint8_t *pub_keys, uint8_t *infinity, int32_t *status,
	    uint32_t flags, void *stream);
int	ecdsa_pub_key_import_le_batch(int curve,
	    const uint8_t *keys, size_t key_stride, const uint32_t *sizes,
	    size_t key_size, const uint8_t *keys_y, size_t count,
	    uint8_t *pub_keys, uint8_t *infinity, int32_t *status,
	    uint32_t flags, void *stream);
int	ecdsa_pub_key_export_be_batch(int curve, int compress,
	    const uint8_t *pub_keys, const uint8_t *infinity, size_t count,
	    uint8_t *out, size_t out_stride, uint32_t *out_sizes,
	    int32_t *status, uint32_t flags, void *stream);
int	ecdsa_pub_key_export_le_batch(int curve, int compress,
	    const uint8_t *pub_keys, const uint8_t *infinity, size_t count,
	    uint8_t *out, size_t out_stride, uint32_t *out_sizes,
	    int32_t *status, uint32_t flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LCB_ECDSA_KEY_GPU_H */
