/*
 * lcb_gost28147_gpu.h — batched GOST 28147-89 on the MI355X
 * (liblcb_gost28147_gpu.so): ECB encrypt / decrypt and the MAC
 * (imitovstavka).
 *
 * The reference's cipher (include/crypto/cipher/gost28147.h) is header-only
 * and one buffer per call:
 *
 *   gost28147_init[_be](key, key_size, sbox, &ctx)               gost28147.h:486-532
 *   gost28147_blocks_encrypt[_be](&ctx, src, blocks_count, dst)  gost28147.h:336-407
 *   gost28147_blocks_decrypt[_be](&ctx, src, blocks_count, dst)  gost28147.h:410-481
 *   gost28147_blocks_mac[_be](&ctx, src, blocks_count)           gost28147.h:288-333
 *   gost28147_final[_be](&ctx, mac, mac_size)                    gost28147.h:534-566
 *
 * Each entry point here computes, for every buffer i, exactly the bytes the
 * reference writes for one call on 4-byte aligned memory with
 *
 *   src = src + off_i, dst = dst + off_i, blocks_count = len_i / 8
 *
 * (integer division, as the reference's own self test calls it), with
 * off_i = offsets ? offsets[i] : i * stride and
 * len_i = lengths ? lengths[i] : fixed_len.  The trailing len_i % 8 bytes of
 * a buffer are not read for the MAC and never written in dst; no byte of dst
 * outside a described buffer is written.  src may equal dst (in place);
 * buffers must not overlap.
 *
 * Alignment.  The reference's encrypt and MAC functions give the same bytes
 * through their 4-byte aligned and their byte-wise code paths.  Its two
 * decrypt functions do not: the unaligned branches (gost28147.h:432-434,
 * 469-476) load and store with the other form's byte order.  The aligned
 * path is the one the reference's self test pins and the one that inverts
 * encrypt, and this API reproduces the ALIGNED path at every byte offset.
 *
 * One key and one sbox per batch, both in host memory in either memory mode;
 * the caller may reuse them as soon as the call returns.  key_size must be
 * 32 or 256 (gost28147.h:490-492; 32 bytes are read either way), else
 * EINVAL.  sbox: 128 bytes, 8 rows of 16 nibbles (gost28147.h:74-139); NULL
 * or an entry above 15 is EINVAL (the reference would OR such an entry into
 * the neighbouring nibble).  A fixed_len that is no multiple of 8 is EINVAL.
 * mac_size must be 1..8, else EINVAL: the reference zero-fills a longer
 * `mac`, which is no MAC, so that is refused here.  A buffer without a whole
 * block has the MAC 00...00, the reference's initial state.  Per-buffer keys
 * and stream modes (CFB/CNT) do not exist in the reference header and not
 * here.
 *
 * Memory modes (flags): LCB_HASH_F_DEVICE (include/lcb_hash_gpu.h) — src,
 * dst, data, macs, offsets and lengths are device pointers and the work is
 * enqueued on `stream` without waiting; 0 — host pointers, staged chunk by
 * chunk through page-locked memory (not pipelined), returns when the output
 * is written.  Errors: 0, EINVAL, ENOMEM, ENODEV, EIO (no CPU fallback).
 */
#ifndef LCB_GOST28147_GPU_H
#define LCB_GOST28147_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* op: 0 encrypt, 1 decrypt.  be: 0 = gost28147_init + gost28147_blocks_*,
 *                                 != 0 = gost28147_init_be + gost28147_blocks_*_be */
int	lcb_gost28147_crypt_batch(int op, int be, const uint8_t *key,
	    size_t key_size, const uint8_t *sbox, const uint8_t *src,
	    uint8_t *dst, const uint64_t *offsets, const uint32_t *lengths,
	    size_t count, uint64_t stride, uint32_t fixed_len, uint32_t flags,
	    void *stream);

/* macs: count x mac_size bytes, packed: what gost28147_final[_be] copies out
 * after gost28147_blocks_mac[_be] over the buffer's whole blocks. */
int	lcb_gost28147_mac_batch(int be, const uint8_t *key, size_t key_size,
	    const uint8_t *sbox, const uint8_t *data, const uint64_t *offsets,
	    const uint32_t *lengths, size_t count, uint64_t stride,
	    uint32_t fixed_len, uint8_t *macs, size_t mac_size, uint32_t flags,
	    void *stream);

/* Reference-named entry points, batched. */
int	gost28147_blocks_encrypt_batch(const uint8_t *key, size_t key_size,
	    const uint8_t *sbox, const uint8_t *src, uint8_t *dst,
	    const uint64_t *offsets, const uint32_t *lengths, size_t count,
	    uint64_t stride, uint32_t fixed_len, uint32_t flags, void *stream);
int	gost28147_blocks_encrypt_be_batch(const uint8_t *key, size_t key_size,
	    const uint8_t *sbox, const uint8_t *src, uint8_t *dst,
	    const uint64_t *offsets, const uint32_t *lengths, size_t count,
	    uint64_t stride, uint32_t fixed_len, uint32_t flags, void *stream);
int	gost28147_blocks_decrypt_batch(const uint8_t *key, size_t key_size,
	    const uint8_t *sbox, const uint8_t *src, uint8_t *dst,
	    const uint64_t *offsets, const uint32_t *lengths, size_t count,
	    uint64_t stride, uint32_t fixed_len, uint32_t flags, void *stream);
int	gost28147_blocks_decrypt_be_batch(const uint8_t *key, size_t key_size,
	    const uint8_t *sbox, const uint8_t *src, uint8_t *dst,
	    const uint64_t *offsets, const uint32_t *lengths, size_t count,
	    uint64_t stride, uint32_t fixed_len, uint32_t flags, void *stream);
int	gost28147_blocks_mac_batch(const uint8_t *key, size_t key_size,
	    const uint8_t *sbox, const uint8_t *data, const uint64_t *offsets,
	    const uint32_t *lengths, size_t count, uint64_t stride,
	    uint32_t fixed_len, uint8_t *macs, size_t mac_size, uint32_t flags,
	    void *stream);
int	gost28147_blocks_mac_be_batch(const uint8_t *key, size_t key_size,
	    const uint8_t *sbox, const uint8_t *data, const uint64_t *offsets,
	    const uint32_t *lengths, size_t count, uint64_t stride,
	    uint32_t fixed_len, uint8_t *macs, size_t mac_size, uint32_t flags,
	    void *stream);

/* The six parameter sets of gost28147.h:74-139 as data (128 bytes each):
 * 0 id-GostR3411-94-TestParamSet, 1..4 id-Gost28147-89-CryptoPro-A..D,
 * 5 id-tc26-gost-28147-param-Z.  NULL for an unknown id. */
const uint8_t	*lcb_gost28147_sbox(int id);

/* Test and measurement aids.  _gpu_table: the 256-word packed table the
 * kernels use for `sbox`, P[i] = rotl32(t0[i] | t1[i] << 8 | t2[i] << 16 |
 * t3[i] << 24, 11) with tk the significant byte of the reference's
 * sboxx[k] (gost28147.h:494-507).  _gpu_copy_probe: the ECB kernel with
 * its rounds skipped (dst = src over every whole block): its memory ceiling. */
int	lcb_gost28147_gpu_table(const uint8_t *sbox, uint32_t *out);
int	lcb_gost28147_gpu_copy_probe(const uint8_t *src, uint8_t *dst,
	    const uint64_t *offsets, const uint32_t *lengths, size_t count,
	    uint64_t stride, uint32_t fixed_len, uint32_t flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LCB_GOST28147_GPU_H */
