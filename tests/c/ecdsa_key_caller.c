/*
 * ecdsa_key_caller.c — a plain C caller of include/lcb_ecdsa_key_gpu.h.
 * Without arguments it checks what needs no GPU (the argument errors), prints
 * "ok" and exits 0.  With the argument "import" it reads records
 *   <curve id> <le> <key>      (hex)
 * from stdin, runs each through one host-mode call of
 * ecdsa_pub_key_import_be_batch / _le_batch, the result through
 * ecdsa_pub_key_export_be_batch / _le_batch in the compressed form, and prints
 *   <status> <infinity> <x || y> <size> <compressed form>
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lcb_ecdsa_key_gpu.h"

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
import_stdin(void)
{
	char k[200];
	int id, le;

	while (scanf("%d %d %199s", &id, &le, k) == 3) {
		uint8_t key[80], pub[64 + 8], form[33 + 8], inf = 0x5a;
		uint32_t fsize = 0;
		int32_t status = 12345, est = 12345;
		size_t size = unhex(k, key, sizeof(key)), i;
		int rc;

		memset(pub, 0xa5, sizeof(pub));
		memset(form, 0xa5, sizeof(form));
		rc = le ? ecdsa_pub_key_import_le_batch(id, key, size, NULL, size, NULL, 1, pub, &inf, &status, 0, NULL)
			: ecdsa_pub_key_import_be_batch(id, key, size, NULL, size, NULL, 1, pub, &inf, &status, 0, NULL);
		if (rc != 0) {
			printf("error %d\n", rc);
			return 21;
		}
		rc = le ? ecdsa_pub_key_export_le_batch(id, 1, pub, &inf, 1, form, 33, &fsize, &est, 0, NULL)
			: ecdsa_pub_key_export_be_batch(id, 1, pub, &inf, 1, form, 33, &fsize, &est, 0, NULL);
		if (rc != 0 || est != 0 || fsize > 33) {
			printf("error %d\n", rc);
			return 23;
		}
		for (i = 64; i < sizeof(pub); i++)
			if (pub[i] != 0xa5)
				return 22;
		for (i = fsize; i < sizeof(form); i++)
			if (form[i] != 0xa5)
				return 24;
		printf("%d %d ", (int)status, (int)inf);
		for (i = 0; i < 64; i++)
			printf("%02x", pub[i]);
		printf(" %u ", (unsigned)fsize);
		for (i = 0; i < fsize; i++)
			printf("%02x", form[i]);
		printf("\n");
	}
	return 0;
}

int
main(int argc, char **argv)
{
	uint8_t buf[160] = {0}, out[160], inf = 0x5a;
	uint32_t sizes[2] = {33, 33};
	int32_t status = 777;

	if (argc > 1 && strcmp(argv[1], "import") == 0)
		return import_stdin();
	memset(out, 0x5a, sizeof(out));
	if (ecdsa_pub_key_import_be_batch(10, buf, 33, NULL, 33, NULL, 1, out, &inf, &status, 0, NULL) != EINVAL)
		return 1;
	if (ecdsa_pub_key_import_le_batch(-1, buf, 33, NULL, 33, NULL, 1, out, &inf, &status, 0, NULL) != EINVAL)
		return 2;
	if (lcb_ecdsa_key_import_batch(1, 0, NULL, 33, NULL, 33, NULL, 1, out, &inf, &status, 0, NULL) != EINVAL)
		return 3;
	if (lcb_ecdsa_key_import_batch(1, 0, buf, 33, sizes, 0, NULL, 1, NULL, &inf, &status, 0, NULL) != EINVAL)
		return 4;
	if (lcb_ecdsa_key_import_batch(1, 1, buf, 33, NULL, 33, NULL, 1, out, NULL, NULL, 0, NULL) != EINVAL)
		return 5;
	if (lcb_ecdsa_key_import_batch(1, 0, buf, 33, NULL, 33, NULL, 1, out, &inf, &status, 0x10, NULL) != EINVAL)
		return 6;
	if (lcb_ecdsa_key_import_batch(1, 0, NULL, 33, NULL, 33, NULL, 0, NULL, NULL, NULL, 0, NULL) != 0)
		return 7;	/* an empty batch */
	if (ecdsa_pub_key_export_be_batch(10, 1, buf, NULL, 1, out, 33, sizes, &status, 0, NULL) != EINVAL)
		return 8;
	if (ecdsa_pub_key_export_le_batch(1, 1, buf, NULL, 1, out, 32, sizes, &status, 0, NULL) != EINVAL)
		return 9;	/* out_stride below the compressed form */
	if (ecdsa_pub_key_export_be_batch(1, 0, buf, NULL, 1, out, 64, sizes, &status, 0, NULL) != EINVAL)
		return 10;	/* out_stride below the packed form */
	if (lcb_ecdsa_key_export_batch(1, 0, 2, buf, NULL, 1, out, 80, sizes, &status, 0, NULL) != EINVAL)
		return 11;	/* an unknown form */
	if (lcb_ecdsa_key_export_batch(1, 0, LCB_ECDSA_KEY_PACKED, buf, NULL, 1, out, 65, NULL, &status, 0, NULL) != EINVAL)
		return 12;
	if (lcb_ecdsa_key_export_batch(1, 0, LCB_ECDSA_KEY_COMPRESSED, buf, NULL, 0, NULL, 33, NULL, NULL, 0, NULL) != 0)
		return 13;	/* an empty batch */
	if (status != 777 || inf != 0x5a || out[0] != 0x5a || out[159] != 0x5a || sizes[0] != 33)
		return 14;	/* nothing was written */
	puts("ok");
	return 0;
}
