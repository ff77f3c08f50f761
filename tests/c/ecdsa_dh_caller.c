/*
 * ecdsa_dh_caller.c — a plain C caller of include/lcb_ecdsa_dh_gpu.h.
 * Without arguments it checks what needs no GPU (the argument errors), prints
 * "ok" and exits 0.  With the argument "dh" it reads records
 *   <curve id> <le> <use_cofactor> <Qx> <Qy> <d>      (hex)
 * from stdin, runs each through one host-mode call of ecdsa_dh_be_batch /
 * ecdsa_dh_le_batch and prints
 *   <status> <shared>
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lcb_ecdsa_dh_gpu.h"

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
dh_stdin(void)
{
	char x[80], y[80], d[80];
	int id, le, cof;

	while (scanf("%d %d %d %79s %79s %79s", &id, &le, &cof, x, y, d) == 6) {
		uint8_t pub[64], priv[32], shared[32 + 8];
		int32_t status = 12345;
		size_t i;
		int rc;

		if (unhex(x, pub, 32) != 32 || unhex(y, pub + 32, 32) != 32 || unhex(d, priv, 32) != 32)
			return 20;
		memset(shared, 0xa5, sizeof(shared));
		rc = le ? ecdsa_dh_le_batch(id, cof, pub, 1, NULL, priv, 1, NULL, 1, shared, &status, 0, NULL)
			: ecdsa_dh_be_batch(id, cof, pub, 1, NULL, priv, 1, NULL, 1, shared, &status, 0, NULL);
		if (rc != 0) {
			printf("error %d\n", rc);
			return 21;
		}
		for (i = 32; i < sizeof(shared); i++)
			if (shared[i] != 0xa5)
				return 22;
		printf("%d ", (int)status);
		for (i = 0; i < 32; i++)
			printf("%02x", shared[i]);
		printf("\n");
	}
	return 0;
}

int
main(int argc, char **argv)
{
	uint8_t buf[128] = {0}, out[64];
	uint32_t idx[2] = {0, 0};
	int32_t status = 777;

	if (argc > 1 && strcmp(argv[1], "dh") == 0)
		return dh_stdin();
	memset(out, 0x5a, sizeof(out));
	if (ecdsa_dh_be_batch(10, 0, buf, 1, NULL, buf, 1, NULL, 1, out, &status, 0, NULL) != EINVAL)
		return 1;
	if (ecdsa_dh_le_batch(-1, 0, buf, 1, NULL, buf, 1, NULL, 1, out, &status, 0, NULL) != EINVAL)
		return 2;
	if (lcb_ecdsa_dh_batch(1, 0, 0, buf, 2, NULL, buf, 1, NULL, 1, out, &status, 0, NULL) != EINVAL)
		return 3;	/* pub_idx == NULL needs npub == count */
	if (lcb_ecdsa_dh_batch(1, 0, 0, buf, 1, NULL, buf, 2, NULL, 1, out, &status, 0, NULL) != EINVAL)
		return 4;	/* priv_idx == NULL needs npriv == count */
	if (lcb_ecdsa_dh_batch(1, 0, 1, buf, 2, idx, buf, 1, idx, 0, out, &status, 0, NULL) != 0)
		return 5;	/* an empty batch */
	if (lcb_ecdsa_dh_batch(1, 0, 0, NULL, 1, NULL, buf, 1, NULL, 1, out, &status, 0, NULL) != EINVAL)
		return 6;
	if (lcb_ecdsa_dh_batch(1, 0, 0, buf, 1, NULL, NULL, 1, idx, 1, out, &status, 0, NULL) != EINVAL)
		return 7;
	if (ecdsa_dh_be_batch(1, 0, buf, 1, NULL, buf, 1, NULL, 1, NULL, &status, 0, NULL) != EINVAL)
		return 8;
	if (ecdsa_dh_le_batch(1, 0, buf, 1, NULL, buf, 1, NULL, 1, out, NULL, 0, NULL) != EINVAL)
		return 9;
	if (ecdsa_dh_be_batch(1, 0, buf, 1, NULL, buf, 1, NULL, 1, out, &status, 0x10, NULL) != EINVAL)
		return 10;
	if (status != 777 || out[0] != 0x5a || out[63] != 0x5a)	/* nothing was written */
		return 11;
	puts("ok");
	return 0;
}
