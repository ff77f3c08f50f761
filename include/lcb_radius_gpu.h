/*
 * lcb_radius_gpu.h — batched RADIUS packet signing and verification on the
 * MI355X (liblcb_radius_gpu.so, linked against liblcb_hash_gpu.so).
 *
 * The reference (include/proto/radius.h) signs and verifies one packet per
 * call on the CPU:
 *
 *   radius_pkt_sign(pkt, buf_size, NULL, key, key_len, 0)   radius.h:1487-1532
 *   radius_pkt_verify(pkt, key, key_len, pkt_req)           radius.h:1535-1568
 *
 * The two entry points here do the same for `count` packed packets, each with
 * its own shared secret, and leave one error code per packet.  Every MD5 and
 * HMAC-MD5 runs on the GPU; nothing is computed per packet on the host and no
 * result travels back to the host between the steps of a call.
 *
 * Buffer description.  Packet i lives in the buffer at
 *   pkts + (offsets ? offsets[i] : i * stride),
 * (buf_sizes ? buf_sizes[i] : fixed_size) bytes long, at any byte alignment;
 * buffers must not overlap.  Only [0, Length) is hashed, Length being the
 * packet's own big-endian Length field; bytes from Length to the end of the
 * buffer are never written (the reference does the same with a receive buffer
 * longer than the packet) and, in host mode, not even read.
 *
 * Keys.  The key table follows lcb_hash_batch_keyed: key k is
 * keys + (key_offsets ? key_offsets[k] : 0), key_lengths[k] bytes; keys,
 * key_offsets and key_lengths are HOST memory in both memory modes and may be
 * released on return.  key_index[i] (NULL: key 0) lives where the batch lives.
 *
 * Requests (verify).  req_hdrs[20 i .. 20 i + 19] holds the first 20 bytes of
 * the request that reply i answers (code, id, length, authenticator); the
 * reference reads only pkt_req->code and pkt_req->authenticator
 * (radius.h:879-901, 1361-1366).  A record whose code byte is 0 (not a RADIUS
 * code) stands for pkt_req == NULL; req_hdrs == NULL for no request at all.
 * req_hdrs lives where the batch lives.
 *
 * errors[i] (where the batch lives) is 0 or the code the reference function
 * returns for packet i:
 *   sign    EINVAL / EOVERFLOW   a User-Password radius_pkt_attr_password_
 *                                encode refuses (radius.h:752-765, buf_size =
 *                                password_len): longer than 128; empty or not
 *                                a multiple of 16
 *           EBADMSG              a Message-Authenticator whose length is not 18
 *   verify  EBADMSG / EINVAL     the first failing step of Message-
 *                                Authenticator check (inside = 0, radius.h:
 *                                858-905, 948), authenticator check (:1388-1398)
 *                                and User-Password decode (:802-808)
 * Sign writes the encoded User-Password, the first Message-Authenticator's
 * 16 data bytes and the authenticator (except for Access-Request, Status-
 * Server and Status-Client).  The only bytes verify ever changes are the
 * User-Password data of a packet with errors[i] == 0 (decoded in place).
 * While a verify call is in flight the authenticator and Message-Authenticator
 * fields of its packets hold substituted values; they are put back before the
 * call's work on the stream ends.
 *
 * Structural guard.  The reference asks for radius_pkt_chk before either
 * function; a batch cannot trust that, so every packet first gets the
 * structural part of radius_pkt_chk and the find walk's checks:
 *   buf_size < 20, Length < 20, Length > buf_size, Length > 4096   EBADMSG
 *   an attribute with fewer than 2 bytes left, len < 2, type 0,
 *   or running past Length (anywhere in the list)                  EBADMSG
 *   key_index[i] >= nkeys                                          EINVAL
 * Such a packet is untouched and no byte of it outside [0, Length) is read.
 * radius_pkt_chk's semantic rules (per-type attribute lengths, attribute
 * counts, the code whitelist) are not applied: for an unknown code verify
 * returns what radius_pkt_verify returns.
 *
 * Two deliberate differences from the reference:
 *   1. A packet with a nonzero error is left byte-for-byte unchanged.  The
 *      reference's sign has already encoded the User-Password in its buffer
 *      when it meets a Message-Authenticator of length != 18 or a malformed
 *      attribute behind the password.
 *   2. The structural guard returns EBADMSG where the reference's verify,
 *      called without radius_pkt_chk, would read out of bounds.
 *
 * Call-level errors, decided before HIP is touched: EINVAL for NULL pkts,
 * errors or keys, nkeys == 0, NULL key_lengths, unknown flags, buf_sizes ==
 * NULL with fixed_size < 20, offsets == NULL with stride < fixed_size while
 * count > 1.  count == 0 returns 0.  Then ENODEV without a usable device
 * (there is no CPU fallback), ENOMEM, EIO.
 *
 * Memory modes (flags):
 *   LCB_HASH_F_DEVICE  pkts, offsets, buf_sizes, key_index, req_hdrs and
 *                      errors are device pointers; the work is enqueued on
 *                      `stream` (a hipStream_t, NULL = default stream).  With
 *                      nkeys == 1 the call waits for nothing.  With more keys
 *                      the two keyed passes go through lcb_hash_batch_keyed,
 *                      whose key-index check the host waits for (4 bytes from
 *                      the device per pass, see include/lcb_hash_gpu.h): the
 *                      call has then waited for its parse, password and HMAC
 *                      steps, not for the suffix pass and what follows it.
 *                      No other device-to-host copy is made and no per-packet
 *                      value reaches the host.
 *   0                  host pointers; packets, key_index, req_hdrs are staged
 *                      chunk by chunk through page-locked memory (only
 *                      [0, Length) of each packet), the device path runs, and
 *                      errors plus [0, Length) of the packets with errors[i]
 *                      == 0 are copied back.  Not pipelined.  `stream` ignored.
 * Secrets the call uploads to device buffers of its own are zeroed before the
 * buffers are released.
 *
 * Out of scope: add_msg_authr != 0 (it grows the packet), Tunnel-Password and
 * other salted attributes, multi-device batches.
 */
#ifndef LCB_RADIUS_GPU_H
#define LCB_RADIUS_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int	radius_pkt_sign_batch(uint8_t *pkts, const uint64_t *offsets,
	    const uint32_t *buf_sizes, size_t count, uint64_t stride, uint32_t fixed_size,
	    const uint8_t *keys, const uint64_t *key_offsets, const uint32_t *key_lengths,
	    size_t nkeys, const uint32_t *key_index,
	    int32_t *errors, uint32_t flags, void *stream);

int	radius_pkt_verify_batch(uint8_t *pkts, const uint64_t *offsets,
	    const uint32_t *buf_sizes, size_t count, uint64_t stride, uint32_t fixed_size,
	    const uint8_t *keys, const uint64_t *key_offsets, const uint32_t *key_lengths,
	    size_t nkeys, const uint32_t *key_index,
	    const uint8_t *req_hdrs,      /* count x 20 bytes, or NULL */
	    int32_t *errors, uint32_t flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LCB_RADIUS_GPU_H */
