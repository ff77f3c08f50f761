/*
 * lcb_hash_stream_gpu.h — batched streaming digests on the MI355X
 * (liblcb_hash_stream_gpu.so): device-resident init / update / final
 * contexts.
 *
 * The reference's main interface is the streaming one:
 *
 *   md5_init / md5_update / md5_final                    md5.h:233-288
 *   sha1_init / sha1_update / sha1_final                 sha1.h:761-840
 *   sha2_init / sha2_update / sha2_final                 sha2.h:647-742
 *   gost3411_2012_init / _update / _final                gost3411-2012.h:1767-1843
 *   hmac_*_init / hmac_*_update / hmac_*_final           md5.h:309-359 (and the same in each header)
 *
 * A STREAM SET is `nstreams` contexts of one algorithm, resident on the HIP
 * device that was current when it was created, optionally keyed (one HMAC key
 * per set; key == NULL: plain digests).  One call updates, finalises or resets
 * many streams at once, one GPU lane per stream.
 *
 * update   Chunk i is data + (offsets ? offsets[i] : i * stride),
 *          (lengths ? lengths[i] : fixed_len) bytes at any byte alignment (the
 *          buffer description of lcb_hash_batch), absorbed into stream
 *          (stream_index ? stream_index[i] : i).  Afterwards the stream holds
 *          exactly what the reference context holds after *_update(ctx, chunk,
 *          len): chaining value, byte count and count % block leftover bytes
 *          (a full block is never kept: gost3411-2012.h:1777-1798).  A
 *          zero-length chunk changes nothing.
 * final    Digest i, packed at digests + i * D, equals *_final (hmac_*_final
 *          for a keyed set) of the listed stream.  The stream is then freshly
 *          initialised (the reference zeroises the context and wants a new
 *          init; here the slot is reusable at once).  With
 *          LCB_HASH_STREAM_F_KEEP the stream is left as it was: "copy the
 *          context, finalise the copy" (proto/radius.h:776-789).
 * reset    The listed streams (stream_index == NULL: the first `count`) as
 *          after *_init / hmac_*_init(key).
 *
 * Index lists.  stream_index lives where the batch lives.  Without it the
 * streams are 0 .. count-1 and count > nstreams is EINVAL.  An index >=
 * nstreams, or one that occurs twice in one call, is EINVAL and no stream is
 * changed.  In device mode the indices are checked on the device ahead of the
 * work and every store is gated on the result; the call waits for that check
 * only (4 bytes back), so for the work already on `stream`, not for its own
 * kernels.  With stream_index == NULL a device-mode call waits for nothing.
 *
 * Memory modes (flags): LCB_HASH_F_DEVICE (include/lcb_hash_gpu.h) —
 * data/offsets/lengths/stream_index/digests are device pointers and the work
 * is enqueued on `stream` (a hipStream_t, NULL = the default stream); 0 —
 * host pointers: the call waits for the device's earlier work, stages through
 * page-locked memory (not pipelined) and returns when it is done.  The key of lcb_hash_stream_create and the records
 * of export / import (with their stream_index) are host memory in every mode.
 *
 * Ordering and threads: calls on one set are ordered by the caller (one HIP
 * stream, or events); a set is not used from two threads at once; different
 * sets are independent.
 *
 * Errors: 0, EINVAL, ENOMEM, ENODEV, EIO.  Argument errors are decided before
 * HIP is touched.  There is no CPU fallback.
 */
#ifndef LCB_HASH_STREAM_GPU_H
#define LCB_HASH_STREAM_GPU_H

#include <stddef.h>
#include <stdint.h>

#include "lcb_hash_gpu.h"	/* LCB_HASH_* algorithm ids, LCB_HASH_F_DEVICE */

#ifdef __cplusplus
extern "C" {
#endif

#define LCB_HASH_STREAM_ABI_VERSION	1

/* lcb_hash_stream_final: do not consume the streams. */
#define LCB_HASH_STREAM_F_KEEP		0x0002u

typedef struct lcb_hash_stream_set_s *lcb_hash_stream_set_p;

/*
 * One stream's state for export / import (checkpoint, migration): the
 * little-endian memory image of the reference context's fields, 344 bytes.
 * For a keyed set the record is the inner context; the opad state belongs
 * to the set.
 */
typedef struct lcb_hash_stream_state_s {
	uint32_t alg;		/* LCB_HASH_* */
	uint32_t used;		/* bytes in buf, < block size */
	uint64_t count;		/* bytes absorbed so far, low 64 bits (HMAC: includes the ipad block) */
	uint64_t count_hi;	/* SHA-384/512 only, else 0 */
	uint8_t  h[64];		/* chaining value as the reference ctx holds it (SHA-224/256: 8 u32; unused tail 0) */
	uint8_t  n[64];		/* GOST counter N, else 0 */
	uint8_t  sigma[64];	/* GOST Sigma, else 0 */
	uint8_t  buf[128];	/* partial block; bytes >= used are 0 */
} lcb_hash_stream_state_t;

int	lcb_hash_stream_abi_version(void);

/* Every stream starts as after *_init, or hmac_*_init(key) for key != NULL
 * (a key longer than the block is replaced by its digest, as in the
 * reference; the ipad and opad mid-states are computed once per set on the
 * device).  The creation work is enqueued on `stream`. */
int	lcb_hash_stream_create(int alg, const uint8_t *key, size_t key_len,
	    size_t nstreams, void *stream, lcb_hash_stream_set_p *out);
/* Waits for the device, zeroes a keyed set's pads, frees everything. */
int	lcb_hash_stream_destroy(lcb_hash_stream_set_p set);
size_t	lcb_hash_stream_count(lcb_hash_stream_set_p set);	/* 0 for NULL */
int	lcb_hash_stream_alg(lcb_hash_stream_set_p set);		/* 0 for NULL */

int	lcb_hash_stream_reset(lcb_hash_stream_set_p set,
	    const uint32_t *stream_index, size_t count, uint32_t flags,
	    void *stream);
int	lcb_hash_stream_update(lcb_hash_stream_set_p set,
	    const uint32_t *stream_index, const uint8_t *data,
	    const uint64_t *offsets, const uint32_t *lengths, size_t count,
	    uint64_t stride, uint32_t fixed_len, uint32_t flags, void *stream);
int	lcb_hash_stream_final(lcb_hash_stream_set_p set,
	    const uint32_t *stream_index, size_t count, uint8_t *digests,
	    uint32_t flags, void *stream);

/*
 * Synchronous; `states` and `stream_index` are host memory.  Export waits for
 * the device's work first.  Import validates every record on the host before
 * anything changes: EINVAL for a wrong alg, used >= block, or (MD5 / SHA)
 * used != count % block.  GOST: `count` is written on export (N / 8 + used)
 * and ignored on import.
 */
int	lcb_hash_stream_export(lcb_hash_stream_set_p set,
	    const uint32_t *stream_index, size_t count,
	    lcb_hash_stream_state_t *states);
int	lcb_hash_stream_import(lcb_hash_stream_set_p set,
	    const uint32_t *stream_index, size_t count,
	    const lcb_hash_stream_state_t *states);

#ifdef __cplusplus
}
#endif
#endif
