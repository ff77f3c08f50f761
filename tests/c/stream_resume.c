/*
 * stream_resume.c — resumes a drop-in context (the headers of include/crypto/hash) from
 * a record of include/lcb_hash_stream_gpu.h: the mapping INTEGRATION.md
 * documents, checked without a GPU (tests/test_stream_state_host.py).
 *
 * stdin, per case: int32 alg, int32 key_len (-1: plain), key bytes, the
 * 344-byte record, int32 rest_len, rest bytes.  The context is initialised
 * (hmac_*_init(key) for a keyed case, which also makes k_opad), its fields
 * are filled from the record, the rest of the message goes through *_update
 * and *_final prints the digest as hex.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "crypto/hash/md5.h"
#include "crypto/hash/sha1.h"
#include "crypto/hash/sha2.h"
#include "crypto/hash/gost3411-2012.h"
#include "lcb_hash_stream_gpu.h"

static const size_t bits_of[] = {0, 0, 0, 224, 256, 384, 512, 256, 512};
static const size_t dsize_of[] = {0, 16, 20, 28, 32, 48, 64, 32, 64};

static void
fill_md5(md5_ctx_p c, const lcb_hash_stream_state_t *r)
{
	memcpy(c->hash, r->h, sizeof(c->hash));
	c->count = r->count;
	memcpy(c->buffer, r->buf, r->used);
}

static void
fill_sha1(sha1_ctx_p c, const lcb_hash_stream_state_t *r)
{
	memcpy(c->hash, r->h, sizeof(c->hash));
	c->count = r->count;
	memcpy(c->buffer, r->buf, r->used);
}

static void
fill_sha2(sha2_ctx_p c, const lcb_hash_stream_state_t *r)
{
	memcpy(c->hash, r->h, c->block_size == 64 ? 32 : 64);
	c->count = r->count;
	c->count_hi = r->count_hi;
	memcpy(c->buffer, r->buf, r->used);
}

static void
fill_gost(gost3411_2012_ctx_p c, const lcb_hash_stream_state_t *r)
{
	memcpy(c->hash, r->h, 64);
	memcpy(c->counter, r->n, 64);
	memcpy(c->sigma, r->sigma, 64);
	c->buffer_usage = r->used;
	memcpy(c->buffer, r->buf, r->used);
}

int
main(void)
{
	static union {
		hmac_md5_ctx_t md5; hmac_sha1_ctx_t sha1; hmac_sha2_ctx_t sha2; hmac_gost3411_2012_ctx_t gost;
	} u;
	int32_t alg, klen, rlen;
	lcb_hash_stream_state_t rec;
	uint8_t key[512], dig[64], *rest;
	size_t ds, hs, i;

	while (fread(&alg, 4, 1, stdin) == 1) {
		if (fread(&klen, 4, 1, stdin) != 1 || klen > (int32_t)sizeof(key))
			return 2;
		if (klen > 0 && fread(key, (size_t)klen, 1, stdin) != 1)
			return 2;
		if (fread(&rec, sizeof(rec), 1, stdin) != 1 || fread(&rlen, 4, 1, stdin) != 1)
			return 2;
		rest = malloc((size_t)rlen + 1);
		if (rlen > 0 && fread(rest, (size_t)rlen, 1, stdin) != 1)
			return 2;
		if ((int32_t)rec.alg != alg)
			return 3;
		if (alg < 1 || alg > 8)
			return 4;
		ds = dsize_of[alg];
		memset(&u, 0, sizeof(u));
		switch (alg) {
		case LCB_HASH_MD5:
			if (klen >= 0) hmac_md5_init(key, (size_t)klen, &u.md5); else md5_init(&u.md5.ctx);
			fill_md5(&u.md5.ctx, &rec);
			md5_update(&u.md5.ctx, rest, (size_t)rlen);
			if (klen >= 0) hmac_md5_final(&u.md5, dig); else md5_final(&u.md5.ctx, dig);
			break;
		case LCB_HASH_SHA1:
			if (klen >= 0) hmac_sha1_init(key, (size_t)klen, &u.sha1); else sha1_init(&u.sha1.ctx);
			fill_sha1(&u.sha1.ctx, &rec);
			sha1_update(&u.sha1.ctx, rest, (size_t)rlen);
			if (klen >= 0) hmac_sha1_final(&u.sha1, dig); else sha1_final(&u.sha1.ctx, dig);
			break;
		case LCB_HASH_SHA224: case LCB_HASH_SHA256: case LCB_HASH_SHA384: case LCB_HASH_SHA512:
			if (klen >= 0) hmac_sha2_init(bits_of[alg], key, (size_t)klen, &u.sha2);
			else sha2_init(bits_of[alg], &u.sha2.ctx);
			fill_sha2(&u.sha2.ctx, &rec);
			sha2_update(&u.sha2.ctx, rest, (size_t)rlen);
			if (klen >= 0) hmac_sha2_final(&u.sha2, dig, &hs); else sha2_final(&u.sha2.ctx, dig);
			break;
		case LCB_HASH_GOST256: case LCB_HASH_GOST512:
			if (klen >= 0) hmac_gost3411_2012_init(bits_of[alg], key, (size_t)klen, &u.gost);
			else gost3411_2012_init(bits_of[alg], &u.gost.ctx);
			fill_gost(&u.gost.ctx, &rec);
			gost3411_2012_update(&u.gost.ctx, rest, (size_t)rlen);
			if (klen >= 0) hmac_gost3411_2012_final(&u.gost, dig, &hs); else gost3411_2012_final(&u.gost.ctx, dig);
			break;
		default:
			return 4;
		}
		for (i = 0; i < ds; i++)
			printf("%02x", dig[i]);
		printf("\n");
		free(rest);
	}
	return 0;
}
