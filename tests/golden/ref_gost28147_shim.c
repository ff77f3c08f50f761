/*
 * ref_gost28147_shim.c — C entry points around the reference's header-only
 * include/crypto/cipher/gost28147.h, for tests/golden/make_golden_gost28147.py
 * (compiled into oracle/_ref/, only where the reference sources exist).
 * Every reference call here is made on 4-byte aligned copies: the aligned
 * path is the one lcb_gost28147_gpu.h reproduces.
 */
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#ifndef GOST28147_SELF_TEST
#define GOST28147_SELF_TEST 1
#endif
#include "crypto/cipher/gost28147.h"

static const uint8_t *
sbox_by_id(int id)
{
	switch (id) {
	case 0: return id_gostr3411_94_testparamset_sbox;
	case 1: return id_gost28147_89_cryptopro_a_paramset_sbox;
	case 2: return id_gost28147_89_cryptopro_b_paramset_sbox;
	case 3: return id_gost28147_89_cryptopro_c_paramset_sbox;
	case 4: return id_gost28147_89_cryptopro_d_paramset_sbox;
	case 5: return id_tc26_gost_28147_param_z_sbox;
	}
	return NULL;
}

static int
id_of_sbox(const uint8_t *p)
{
	int id;

	for (id = 0; id < 6; id++)
		if (sbox_by_id(id) == p)
			return id;
	return -1;
}

int
ref_gost28147_self_test(void)
{
	return gost28147_self_test();
}

/* out: 128 bytes, or returns -1. */
int
ref_gost28147_sbox(int id, uint8_t *out)
{
	const uint8_t *p = sbox_by_id(id);

	if (p == NULL)
		return -1;
	memcpy(out, p, 128);
	return 0;
}

/* out: the four expanded tables of gost28147_init, 4 x 256 words. */
int
ref_gost28147_tables(int id, uint32_t *out)
{
	static const uint8_t key[32];
	gost28147_context_t ctx;
	int error = gost28147_init(key, 32, sbox_by_id(id), &ctx);

	if (error == 0)
		memcpy(out, ctx.sboxx, sizeof(ctx.sboxx));
	return error;
}

/* op 0 encrypt / 1 decrypt over `blocks` blocks, aligned copies. */
int
ref_gost28147_crypt(int op, int be, const uint8_t *key, int sbox_id,
    const uint8_t *src, size_t blocks, uint8_t *dst)
{
	gost28147_context_t ctx;
	uint32_t *a, *b;
	int error;

	error = be ? gost28147_init_be(key, 32, sbox_by_id(sbox_id), &ctx)
		   : gost28147_init(key, 32, sbox_by_id(sbox_id), &ctx);
	if (error != 0)
		return error;
	a = malloc(blocks * 8 + 8);
	b = malloc(blocks * 8 + 8);
	if (a == NULL || b == NULL)
		return ENOMEM;
	memcpy(a, src, blocks * 8);
	if (op == 0) {
		if (be)
			gost28147_blocks_encrypt_be(&ctx, (uint8_t *)a, blocks, (uint8_t *)b);
		else
			gost28147_blocks_encrypt(&ctx, (uint8_t *)a, blocks, (uint8_t *)b);
	} else {
		if (be)
			gost28147_blocks_decrypt_be(&ctx, (uint8_t *)a, blocks, (uint8_t *)b);
		else
			gost28147_blocks_decrypt(&ctx, (uint8_t *)a, blocks, (uint8_t *)b);
	}
	memcpy(dst, b, blocks * 8);
	free(a);
	free(b);
	return 0;
}

int
ref_gost28147_mac(int be, const uint8_t *key, int sbox_id, const uint8_t *src,
    size_t blocks, uint8_t *mac, size_t mac_size)
{
	gost28147_context_t ctx;
	uint32_t *a;
	int error;

	error = be ? gost28147_init_be(key, 32, sbox_by_id(sbox_id), &ctx)
		   : gost28147_init(key, 32, sbox_by_id(sbox_id), &ctx);
	if (error != 0)
		return error;
	a = malloc(blocks * 8 + 8);
	if (a == NULL)
		return ENOMEM;
	memcpy(a, src, blocks * 8);
	if (be) {
		gost28147_blocks_mac_be(&ctx, (uint8_t *)a, blocks);
		gost28147_final_be(&ctx, mac, mac_size);
	} else {
		gost28147_blocks_mac(&ctx, (uint8_t *)a, blocks);
		gost28147_final(&ctx, mac, mac_size);
	}
	free(a);
	return 0;
}

/*
 * Self-test vector `idx` of table `tbl` (0 ECB LE, 1 ECB BE, 2 MAC LE,
 * 3 MAC BE), decoded by the reference's own hex import.  Returns the data
 * size in bytes, or -1 past the table's end.  key: 32 bytes; plain/out: up to
 * GOST28147_TEST_LEN bytes (out: the ciphertext, or the 8-byte MAC).
 */
long
ref_gost28147_kat(int tbl, size_t idx, uint8_t *key, int *sbox_id,
    uint8_t *plain, uint8_t *out)
{
	uint8_t k[GOST28147_KEY_SIZE + 1];
	size_t i, n;

	if (tbl == 0 || tbl == 1) {
		gost28147_tst1v_p v = tbl ? gost28147_tst1v_be : gost28147_tst1v;

		for (i = 0; i < idx; i++)
			if (v[i].key_size == 0)
				return -1;
		if (v[idx].key_size == 0)
			return -1;
		n = v[idx].data_size / 2;
		if (gost28147_import_le_hex(k, sizeof(k), v[idx].key, v[idx].key_size) != 0 ||
		    gost28147_import_le_hex(plain, GOST28147_TEST_LEN, v[idx].plain, v[idx].data_size) != 0 ||
		    gost28147_import_le_hex(out, GOST28147_TEST_LEN, v[idx].encrypted, v[idx].data_size) != 0)
			return -2;
		*sbox_id = id_of_sbox(v[idx].sbox);
	} else {
		gost28147_tst2v_p v = tbl == 3 ? gost28147_tst2v_be : gost28147_tst2v;

		for (i = 0; i < idx; i++)
			if (v[i].key_size == 0)
				return -1;
		if (v[idx].key_size == 0)
			return -1;
		n = v[idx].data_size / 2;
		if (gost28147_import_le_hex(k, sizeof(k), v[idx].key, v[idx].key_size) != 0 ||
		    gost28147_import_le_hex(plain, GOST28147_TEST_LEN, v[idx].plain, v[idx].data_size) != 0 ||
		    gost28147_import_le_hex(out, GOST28147_TEST_LEN, v[idx].mac, 16) != 0)
			return -2;
		*sbox_id = id_of_sbox(v[idx].sbox);
	}
	memcpy(key, k, 32);
	return (long)n;
}
