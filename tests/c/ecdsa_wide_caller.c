/*
 * ecdsa_wide_caller.c — a plain C caller of include/lcb_ecdsa_wide_gpu.h.
 * Without arguments it checks what needs no GPU (the curve table, the
 * argument errors), prints "ok" and exits 0.  With the argument "verify" it
 * reads records
 *   <curve name> <le> <hash_size> <hash> <r> <s> <Qx> <Qy>      (hex)
 * from stdin, verifies each with one host-mode call of
 * ecdsa_verify_be_wide_batch / ecdsa_verify_le_wide_batch and prints its
 * status.
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lcb_ecdsa_wide_gpu.h"

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
	char name[80], h[264], r[136], s[136], qx[136], qy[136];
	int le;
	unsigned hash_size;

	while (scanf("%79s %d %u %263s %135s %135s %135s %135s", name, &le, &hash_size, h, r, s, qx, qy) == 8) {
		uint8_t hash[128] = {0}, sig[128], key[128];
		int32_t status = 12345;
		int id = lcb_ecdsa_wide_curve_id(name), rc;
		size_t B;

		if (lcb_ecdsa_wide_curve_bytes(id) < 0)
			return 19;
		B = (size_t)lcb_ecdsa_wide_curve_bytes(id);
		unhex(h, hash, 128);
		if (unhex(r, sig, 64) != B || unhex(s, sig + B, 64) != B ||
		    unhex(qx, key, 64) != B || unhex(qy, key + B, 64) != B)
			return 20;
		rc = le ? ecdsa_verify_le_wide_batch(id, hash, hash_size, sig, key, 1, NULL, 1, &status, 0, NULL)
			: ecdsa_verify_be_wide_batch(id, hash, hash_size, sig, key, 1, NULL, 1, &status, 0, NULL);
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
	uint8_t buf[256] = {0}, params[384];
	uint32_t idx = 0, algo = 9, h = 9;
	int32_t status = 0;
	int id;

	if (argc > 1 && strcmp(argv[1], "verify") == 0)
		return verify_stdin();
	if (lcb_ecdsa_wide_curve_count() != 6)
		return 1;
	for (id = 0; id < 6; id++)
		if (lcb_ecdsa_wide_curve_name(id) == NULL ||
		    lcb_ecdsa_wide_curve_id(lcb_ecdsa_wide_curve_name(id)) != id ||
		    lcb_ecdsa_wide_curve_bytes(id) != (id < 2 ? 48 : 64))
			return 2;
	if (lcb_ecdsa_wide_curve_name(6) != NULL || lcb_ecdsa_wide_curve_id("secp521r1") != -1 ||
	    lcb_ecdsa_wide_curve_id("secp256r1") != -1 || lcb_ecdsa_wide_curve_bytes(6) != -1)
		return 3;
	if (lcb_ecdsa_wide_curve_id("secp384r1") != 0 || lcb_ecdsa_wide_curve_params(0, params, &algo, &h) != 0)
		return 4;
	/* secp384r1: p = ff ... fe ffffffff 00000000 00000000 ffffffff, ECDSA, cofactor 1 */
	if (params[0] != 0xff || params[31] != 0xfe || params[36] != 0 || params[47] != 0xff ||
	    algo != LCB_ECDSA_WIDE_ALGO_ECDSA || h != 1)
		return 5;
	if (lcb_ecdsa_wide_curve_params(3, params, &algo, &h) != 0 || algo != LCB_ECDSA_WIDE_ALGO_GOST ||
	    params[63] != 0xc7)
		return 6;
	if (ecdsa_verify_be_wide_batch(6, buf, 48, buf, buf, 1, NULL, 1, &status, 0, NULL) != EINVAL)
		return 7;
	if (ecdsa_verify_le_wide_batch(3, buf, 129, buf, buf, 1, NULL, 1, &status, 0, NULL) != EINVAL)
		return 8;
	if (lcb_ecdsa_wide_verify_batch(0, 0, buf, 48, buf, buf, 2, NULL, 1, &status, 0, NULL) != EINVAL)
		return 9;
	if (lcb_ecdsa_wide_verify_batch(0, 0, buf, 48, buf, buf, 2, &idx, 0, &status, 0, NULL) != 0)
		return 10;
	puts("ok");
	return 0;
}
