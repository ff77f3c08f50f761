/*
 * ref_stream_shim.c — C entry points around the reference's header-only
 * streaming digests (include/crypto/hash/{md5,sha1,sha2,gost3411-2012}.h),
 * for tests/golden/make_golden_stream.py (compiled into oracle/_ref/, only
 * where the reference sources exist).
 *
 * ref_stream_record: the reference context's fields after *_init (or
 * hmac_*_init(key)) and ONE *_update of n bytes, as the 344-byte record of
 * include/lcb_hash_stream_gpu.h (restated here, so that only the
 * reference's include directory is on the include path).
 * ref_stream_digest: *_final after the same.
 */
#include <sys/param.h>
#include <sys/types.h>
#include <stdint.h>
#include <string.h>

#undef __SSE2__		/* the generic code paths, as the reference's tests/hash/main.c builds them */

#include "crypto/hash/md5.h"
#include "crypto/hash/sha1.h"
#include "crypto/hash/sha2.h"
#include "crypto/hash/gost3411-2012.h"

typedef struct rec_s {
	uint32_t alg, used;
	uint64_t count, count_hi;
	uint8_t h[64], n[64], sigma[64], buf[128];
} rec_t;

typedef char rec_size_is_344[(sizeof(rec_t) == 344) ? 1 : -1];

static const size_t sha2_bits[] = {0, 0, 0, 224, 256, 384, 512};

typedef union any_ctx_u {
	md5_ctx_t md5; hmac_md5_ctx_t hmd5;
	sha1_ctx_t sha1; hmac_sha1_ctx_t hsha1;
	sha2_ctx_t sha2; hmac_sha2_ctx_t hsha2;
	gost3411_2012_ctx_t gost; hmac_gost3411_2012_ctx_t hgost;
} any_ctx_t;

/* init (+ key) and one update; 0 or -1 for an unknown alg. */
static int
absorb(any_ctx_t *c, int alg, int keyed, const uint8_t *key, size_t key_len, const uint8_t *msg, size_t n)
{
	switch (alg) {
	case 1:
		if (keyed) { hmac_md5_init(key, key_len, &c->hmd5); hmac_md5_update(&c->hmd5, msg, n); }
		else { md5_init(&c->md5); md5_update(&c->md5, msg, n); }
		return 0;
	case 2:
		if (keyed) { hmac_sha1_init(key, key_len, &c->hsha1); hmac_sha1_update(&c->hsha1, msg, n); }
		else { sha1_init(&c->sha1); sha1_update(&c->sha1, msg, n); }
		return 0;
	case 3: case 4: case 5: case 6:
		if (keyed) { hmac_sha2_init(sha2_bits[alg], key, key_len, &c->hsha2); hmac_sha2_update(&c->hsha2, msg, n); }
		else { sha2_init(sha2_bits[alg], &c->sha2); sha2_update(&c->sha2, msg, n); }
		return 0;
	case 7: case 8:
		if (keyed) {
			hmac_gost3411_2012_init(alg == 7 ? 256 : 512, key, key_len, &c->hgost);
			hmac_gost3411_2012_update(&c->hgost, msg, n);
		} else {
			gost3411_2012_init(alg == 7 ? 256 : 512, &c->gost);
			gost3411_2012_update(&c->gost, msg, n);
		}
		return 0;
	}
	return -1;
}

int
ref_stream_record(int alg, int keyed, const uint8_t *key, size_t key_len, const uint8_t *msg, size_t n, uint8_t *out)
{
	static any_ctx_t c;	/* the contexts ask for 32-byte alignment */
	rec_t r;

	if (absorb(&c, alg, keyed, key, key_len, msg, n))
		return -1;
	memset(&r, 0, sizeof(r));
	r.alg = (uint32_t)alg;
	switch (alg) {
	case 1: {
		const md5_ctx_t *x = keyed ? &c.hmd5.ctx : &c.md5;
		r.count = x->count; r.used = (uint32_t)(x->count & 63);
		memcpy(r.h, x->hash, 16); memcpy(r.buf, x->buffer, r.used);
		break;
	}
	case 2: {
		const sha1_ctx_t *x = keyed ? &c.hsha1.ctx : &c.sha1;
		r.count = x->count; r.used = (uint32_t)(x->count & 63);
		memcpy(r.h, x->hash, 20); memcpy(r.buf, x->buffer, r.used);
		break;
	}
	case 3: case 4: case 5: case 6: {
		const sha2_ctx_t *x = keyed ? &c.hsha2.ctx : &c.sha2;
		r.count = x->count; r.count_hi = x->count_hi;
		r.used = (uint32_t)(x->count & (x->block_size - 1));
		memcpy(r.h, x->hash, x->block_size == 64 ? 32 : 64); memcpy(r.buf, x->buffer, r.used);
		break;
	}
	default: {
		const gost3411_2012_ctx_t *x = keyed ? &c.hgost.ctx : &c.gost;
		r.used = (uint32_t)x->buffer_usage;
		r.count = (x->counter[0] >> 3 | x->counter[1] << 61) + r.used;
		memcpy(r.h, x->hash, 64); memcpy(r.n, x->counter, 64); memcpy(r.sigma, x->sigma, 64);
		memcpy(r.buf, x->buffer, r.used);
		break;
	}
	}
	memcpy(out, &r, sizeof(r));
	return 0;
}

int
ref_stream_digest(int alg, int keyed, const uint8_t *key, size_t key_len, const uint8_t *msg, size_t n, uint8_t *digest)
{
	static any_ctx_t c;
	size_t ds = 0;

	if (absorb(&c, alg, keyed, key, key_len, msg, n))
		return -1;
	switch (alg) {
	case 1: if (keyed) hmac_md5_final(&c.hmd5, digest); else md5_final(&c.md5, digest); break;
	case 2: if (keyed) hmac_sha1_final(&c.hsha1, digest); else sha1_final(&c.sha1, digest); break;
	case 3: case 4: case 5: case 6:
		if (keyed) hmac_sha2_final(&c.hsha2, digest, &ds); else sha2_final(&c.sha2, digest);
		break;
	default:
		if (keyed) hmac_gost3411_2012_final(&c.hgost, digest, &ds); else gost3411_2012_final(&c.gost, digest);
		break;
	}
	return 0;
}
