/*
 * ecdsa_wide_sign_caller.c — a plain C caller of
 * include/lcb_ecdsa_wide_sign_gpu.h.  Without arguments it checks what needs
 * no GPU (the argument errors), prints "ok" and exits 0.  With the argument
 * "sign" it reads records
 *   <curve id> <le> <hash_size> <hash> <d> <rnd>      (hex; d and rnd B bytes)
 * from stdin, signs each with one host-mode call of ecdsa_sign_be_wide_batch /
 * ecdsa_sign_le_wide_batch, recovers the public key with
 * ecdsa_recover_pub_key_from_priv_key_*_wide_batch and prints
 *   <status> <r || s> <key status> <x || y>
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lcb_ecdsa_wide_sign_gpu.h"

static size_t
unhex(const char *s, uint8_t *out, size_t cap)
{
	size_t n = strlen(s) / 2, i;
	unsigned v;

	if (n > cap)
		n = cap;
	for (i = 0; i < n; i++) {
		sscanf(s + 2 * i, "%2x", &v);
		out[i] = (uint8_t)v;
	}
	return n;
}

static void
puthex(const uint8_t *p, size_t n)
{
	size_t i;

	for (i = 0; i < n; i++)
		printf("%02x", p[i]);
}

static int
sign_stdin(void)
{
	char h[260], d[140], k[140];
	int id, le;
	unsigned hash_size;

	while (scanf("%d %d %u %259s %139s %139s", &id, &le, &hash_size, h, d, k) == 6) {
		uint8_t hash[128] = {0}, priv[64], rnd[64], sig[128 + 8], pub[128 + 8];
		int32_t status = 12345, kstatus = 12345;
		size_t B;
		int rc;

		unhex(h, hash, 128);
		B = unhex(d, priv, 64);
		if ((B != 48 && B != 64) || unhex(k, rnd, 64) != B)
			return 20;
		memset(sig, 0xa5, sizeof(sig));
		memset(pub, 0xa5, sizeof(pub));
		rc = le ? ecdsa_sign_le_wide_batch(id, hash, hash_size, priv, 1, NULL, rnd, 1, sig, &status, 0, NULL)
			: ecdsa_sign_be_wide_batch(id, hash, hash_size, priv, 1, NULL, rnd, 1, sig, &status, 0, NULL);
		if (rc == 0)
			rc = le ? ecdsa_recover_pub_key_from_priv_key_le_wide_batch(id, priv, 1, pub, &kstatus, 0, NULL)
				: ecdsa_recover_pub_key_from_priv_key_be_wide_batch(id, priv, 1, pub, &kstatus, 0, NULL);
		if (rc != 0) {
			printf("error %d\n", rc);
			return 21;
		}
		if (sig[2 * B] != 0xa5 || pub[2 * B] != 0xa5)	/* 2 B bytes and no more */
			return 22;
		printf("%d ", (int)status);
		puthex(sig, 2 * B);
		printf(" %d ", (int)kstatus);
		puthex(pub, 2 * B);
		printf("\n");
	}
	return 0;
}

int
main(int argc, char **argv)
{
	uint8_t buf[256] = {0}, out[256];
	uint32_t idx = 0;
	int32_t status = 777;

	if (argc > 1 && strcmp(argv[1], "sign") == 0)
		return sign_stdin();
	memset(out, 0x5a, sizeof(out));
	if (ecdsa_sign_be_wide_batch(6, buf, 48, buf, 1, NULL, buf, 1, out, &status, 0, NULL) != EINVAL)
		return 1;
	if (ecdsa_sign_le_wide_batch(3, buf, 129, buf, 1, NULL, buf, 1, out, &status, 0, NULL) != EINVAL)
		return 2;
	if (lcb_ecdsa_wide_sign_batch(0, 0, buf, 48, buf, 2, NULL, buf, 1, out, &status, 0, NULL) != EINVAL)
		return 3;
	if (lcb_ecdsa_wide_sign_batch(0, 0, buf, 48, buf, 2, &idx, buf, 0, out, &status, 0, NULL) != 0)
		return 4;
	if (lcb_ecdsa_wide_sign_batch(2, 0, buf, 64, buf, 1, NULL, NULL, 1, out, &status, 0, NULL) != EINVAL)
		return 5;
	if (ecdsa_key_gen_be_wide_batch(-1, buf, 1, out, out + 64, &status, 0, NULL) != EINVAL)
		return 6;
	if (ecdsa_key_gen_le_wide_batch(3, buf, 1, NULL, out + 64, &status, 0, NULL) != EINVAL)
		return 7;
	if (lcb_ecdsa_wide_key_gen_batch(0, 0, buf, 0, NULL, NULL, NULL, 0, NULL) != 0)
		return 8;
	if (ecdsa_recover_pub_key_from_priv_key_be_wide_batch(0, buf, 1, out, &status, 0x10, NULL) != EINVAL)
		return 9;
	if (ecdsa_recover_pub_key_from_priv_key_le_wide_batch(3, NULL, 1, out, &status, 0, NULL) != EINVAL)
		return 10;
	if (lcb_ecdsa_wide_pub_key_batch(6, 0, buf, 1, out, &status, 0, NULL) != EINVAL)
		return 11;
	if (status != 777 || out[0] != 0x5a || out[255] != 0x5a)	/* nothing was written */
		return 12;
	puts("ok");
	return 0;
}
