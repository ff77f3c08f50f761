/*
 * ecdsa_sign_caller.c — a plain C caller of include/lcb_ecdsa_sign_gpu.h.
 * Without arguments it checks what needs no GPU (the argument errors), prints
 * "ok" and exits 0.  With the argument "sign" it reads records
 *   <curve id> <le> <hash_size> <hash> <d> <rnd>      (hex)
 * from stdin, signs each with one host-mode call of ecdsa_sign_be_batch /
 * ecdsa_sign_le_batch, recovers the public key with
 * ecdsa_recover_pub_key_from_priv_key_*_batch and prints
 *   <status> <r || s> <key status> <x || y>
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lcb_ecdsa_sign_gpu.h"

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
	char h[140], d[80], k[80];
	int id, le;
	unsigned hash_size;

	while (scanf("%d %d %u %139s %79s %79s", &id, &le, &hash_size, h, d, k) == 6) {
		uint8_t hash[64] = {0}, priv[32], rnd[32], sig[64], pub[64];
		int32_t status = 12345, kstatus = 12345;
		int rc;

		unhex(h, hash, 64);
		if (unhex(d, priv, 32) != 32 || unhex(k, rnd, 32) != 32)
			return 20;
		memset(sig, 0xa5, sizeof(sig));
		memset(pub, 0xa5, sizeof(pub));
		rc = le ? ecdsa_sign_le_batch(id, hash, hash_size, priv, 1, NULL, rnd, 1, sig, &status, 0, NULL)
			: ecdsa_sign_be_batch(id, hash, hash_size, priv, 1, NULL, rnd, 1, sig, &status, 0, NULL);
		if (rc == 0)
			rc = le ? ecdsa_recover_pub_key_from_priv_key_le_batch(id, priv, 1, pub, &kstatus, 0, NULL)
				: ecdsa_recover_pub_key_from_priv_key_be_batch(id, priv, 1, pub, &kstatus, 0, NULL);
		if (rc != 0) {
			printf("error %d\n", rc);
			return 21;
		}
		printf("%d ", (int)status);
		puthex(sig, 64);
		printf(" %d ", (int)kstatus);
		puthex(pub, 64);
		printf("\n");
	}
	return 0;
}

int
main(int argc, char **argv)
{
	uint8_t buf[128] = {0}, out[128];
	uint32_t idx = 0;
	int32_t status = 777;

	if (argc > 1 && strcmp(argv[1], "sign") == 0)
		return sign_stdin();
	memset(out, 0x5a, sizeof(out));
	if (ecdsa_sign_be_batch(10, buf, 32, buf, 1, NULL, buf, 1, out, &status, 0, NULL) != EINVAL)
		return 1;
	if (ecdsa_sign_le_batch(1, buf, 65, buf, 1, NULL, buf, 1, out, &status, 0, NULL) != EINVAL)
		return 2;
	if (lcb_ecdsa_sign_batch(1, 0, buf, 32, buf, 2, NULL, buf, 1, out, &status, 0, NULL) != EINVAL)
		return 3;
	if (lcb_ecdsa_sign_batch(1, 0, buf, 32, buf, 2, &idx, buf, 0, out, &status, 0, NULL) != 0)
		return 4;
	if (lcb_ecdsa_sign_batch(1, 0, buf, 32, buf, 1, NULL, NULL, 1, out, &status, 0, NULL) != EINVAL)
		return 5;
	if (ecdsa_key_gen_be_batch(-1, buf, 1, out, out + 32, &status, 0, NULL) != EINVAL)
		return 6;
	if (ecdsa_key_gen_le_batch(1, buf, 1, NULL, out + 32, &status, 0, NULL) != EINVAL)
		return 7;
	if (lcb_ecdsa_key_gen_batch(1, 0, buf, 0, NULL, NULL, NULL, 0, NULL) != 0)
		return 8;
	if (ecdsa_recover_pub_key_from_priv_key_be_batch(1, buf, 1, out, &status, 0x10, NULL) != EINVAL)
		return 9;
	if (ecdsa_recover_pub_key_from_priv_key_le_batch(1, NULL, 1, out, &status, 0, NULL) != EINVAL)
		return 10;
	if (lcb_ecdsa_pub_key_batch(10, 0, buf, 1, out, &status, 0, NULL) != EINVAL)
		return 11;
	if (status != 777 || out[0] != 0x5a || out[127] != 0x5a)	/* nothing was written */
		return 12;
	puts("ok");
	return 0;
}
