/*
 * ecdsa_caller.c — a plain C caller of include/lcb_ecdsa_gpu.h.
 * Without arguments it checks what needs no GPU (the curve table, the
 * argument errors), prints "ok" and exits 0.  With the argument "verify" it
 * reads records
 *   <curve name> <le> <hash_size> <hash> <r> <s> <Qx> <Qy>      (hex)
 * from stdin, verifies each with one host-mode call of
 * ecdsa_verify_be_batch / ecdsa_verify_le_batch and prints its status.
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lcb_ecdsa_gpu.h"

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

static int
verify_stdin(void)
{
	char name[80], h[140], r[80], s[80], qx[80], qy[80];
	int le;
	unsigned hash_size;

	while (scanf("%79s %d %u %139s %79s %79s %79s %79s", name, &le, &hash_size, h, r, s, qx, qy) == 8) {
		uint8_t hash[64] = {0}, sig[64], key[64];
		int32_t status = 12345;
		int id = lcb_ecdsa_curve_id(name), rc;

		unhex(h, hash, 64);
		if (unhex(r, sig, 32) != 32 || unhex(s, sig + 32, 32) != 32 ||
		    unhex(qx, key, 32) != 32 || unhex(qy, key + 32, 32) != 32)
			return 20;
		rc = le ? ecdsa_verify_le_batch(id, hash, hash_size, sig, key, 1, NULL, 1, &status, 0, NULL)
			: ecdsa_verify_be_batch(id, hash, hash_size, sig, key, 1, NULL, 1, &status, 0, NULL);
		if (rc != 0) {
			printf("error %d\n", rc);
			return 21;
		}
		printf("%d\n", (int)status);
	}
	return 0;
}

int
main(int argc, char **argv)
{
	uint8_t buf[192] = {0}, params[192];
	uint32_t idx = 0, algo = 9, h = 9;
	int32_t status = 0;
	int id;

	if (argc > 1 && strcmp(argv[1], "verify") == 0)
		return verify_stdin();
	if (lcb_ecdsa_curve_count() != 10)
		return 1;
	for (id = 0; id < 10; id++)
		if (lcb_ecdsa_curve_name(id) == NULL || lcb_ecdsa_curve_id(lcb_ecdsa_curve_name(id)) != id)
			return 2;
	if (lcb_ecdsa_curve_name(10) != NULL || lcb_ecdsa_curve_id("secp521r1") != -1)
		return 3;
	if (lcb_ecdsa_curve_id("secp256r1") != 1 || lcb_ecdsa_curve_params(1, params, &algo, &h) != 0)
		return 4;
	/* secp256r1: p = ffffffff 00000001 ..., ECDSA, cofactor 1 */
	if (params[0] != 0xff || params[4] != 0 || params[7] != 1 || algo != LCB_ECDSA_ALGO_ECDSA || h != 1)
		return 5;
	if (lcb_ecdsa_curve_params(5, params, &algo, &h) != 0 || algo != LCB_ECDSA_ALGO_GOST)
		return 6;
	if (ecdsa_verify_be_batch(10, buf, 32, buf, buf, 1, NULL, 1, &status, 0, NULL) != EINVAL)
		return 7;
	if (ecdsa_verify_le_batch(1, buf, 65, buf, buf, 1, NULL, 1, &status, 0, NULL) != EINVAL)
		return 8;
	if (lcb_ecdsa_verify_batch(1, 0, buf, 32, buf, buf, 2, NULL, 1, &status, 0, NULL) != EINVAL)
		return 9;
	if (lcb_ecdsa_verify_batch(1, 0, buf, 32, buf, buf, 2, &idx, 0, &status, 0, NULL) != 0)
		return 10;
	puts("ok");
	return 0;
}
