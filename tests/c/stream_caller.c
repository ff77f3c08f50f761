/*
 * stream_caller.c — a plain C99 caller of include/lcb_hash_stream_gpu.h.
 *
 *   stream_caller            the record's size and field offsets, then what
 *                            needs no GPU: every argument error is EINVAL
 *                            before HIP is touched; prints "ok".
 *   stream_caller ALG N KEY  (KEY: "-" for none) create, update x 2 and final
 *                            in host mode over N streams; stream s takes
 *                            pat[200 s, 200 s + 37 + s) and then the next
 *                            64 + 2 s bytes, pat[i] = (i * 131 + (i >> 8) * 7 + 5) & 255.
 *                            Prints one digest per line.
 */
#include <errno.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lcb_hash_stream_gpu.h"

static int
run(int alg, size_t n, const char *key)
{
	lcb_hash_stream_set_p set = NULL;
	const size_t D = lcb_hash_digest_size(alg);
	uint8_t *pat = malloc(200 * n + 512), *dig = malloc(n * 64);
	uint64_t *off = malloc(n * sizeof(uint64_t));
	uint32_t *len = malloc(n * sizeof(uint32_t));
	size_t i, s;
	int rc;

	for (i = 0; i < 200 * n + 512; i++)
		pat[i] = (uint8_t)(i * 131 + (i >> 8) * 7 + 5);
	rc = lcb_hash_stream_create(alg, strcmp(key, "-") ? (const uint8_t *)key : NULL,
	    strcmp(key, "-") ? strlen(key) : 0, n, NULL, &set);
	if (rc)
		return rc;
	if (lcb_hash_stream_count(set) != n || lcb_hash_stream_alg(set) != alg)
		return -1;
	for (s = 0; s < n; s++) { off[s] = 200 * s; len[s] = (uint32_t)(37 + s); }
	if ((rc = lcb_hash_stream_update(set, NULL, pat, off, len, n, 0, 0, 0, NULL)))
		return rc;
	for (s = 0; s < n; s++) { off[s] += len[s]; len[s] = (uint32_t)(64 + 2 * s); }
	if ((rc = lcb_hash_stream_update(set, NULL, pat, off, len, n, 0, 0, 0, NULL)))
		return rc;
	if ((rc = lcb_hash_stream_final(set, NULL, n, dig, 0, NULL)))
		return rc;
	for (s = 0; s < n; s++) {
		for (i = 0; i < D; i++)
			printf("%02x", dig[s * D + i]);
		printf("\n");
	}
	return lcb_hash_stream_destroy(set);
}

int
main(int argc, char **argv)
{
	lcb_hash_stream_set_p set = NULL;
	lcb_hash_stream_state_t st;
	uint8_t buf[64] = {0};

	if (argc == 4) {
		const int rc = run(atoi(argv[1]), (size_t)atol(argv[2]), argv[3]);

		if (rc)
			fprintf(stderr, "error %d\n", rc);
		return rc ? 1 : 0;
	}
	printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(st), offsetof(lcb_hash_stream_state_t, alg),
	    offsetof(lcb_hash_stream_state_t, used), offsetof(lcb_hash_stream_state_t, count),
	    offsetof(lcb_hash_stream_state_t, count_hi), offsetof(lcb_hash_stream_state_t, h),
	    offsetof(lcb_hash_stream_state_t, n), offsetof(lcb_hash_stream_state_t, sigma),
	    offsetof(lcb_hash_stream_state_t, buf));
	if (lcb_hash_stream_abi_version() != LCB_HASH_STREAM_ABI_VERSION)
		return 1;
	if (lcb_hash_stream_create(LCB_HASH_MD5, NULL, 0, 4, NULL, NULL) != EINVAL)
		return 2;
	if (lcb_hash_stream_create(0, NULL, 0, 4, NULL, &set) != EINVAL || set != NULL)
		return 3;
	if (lcb_hash_stream_create(9, NULL, 0, 4, NULL, &set) != EINVAL)
		return 4;
	if (lcb_hash_stream_create(LCB_HASH_MD5, NULL, 0, 0, NULL, &set) != EINVAL)
		return 5;
	if (lcb_hash_stream_create(LCB_HASH_MD5, NULL, 3, 4, NULL, &set) != EINVAL)
		return 6;
	if (lcb_hash_stream_update(NULL, NULL, buf, NULL, NULL, 1, 64, 64, 0, NULL) != EINVAL)
		return 7;
	if (lcb_hash_stream_final(NULL, NULL, 1, buf, 0, NULL) != EINVAL)
		return 8;
	if (lcb_hash_stream_reset(NULL, NULL, 1, 0, NULL) != EINVAL)
		return 9;
	if (lcb_hash_stream_export(NULL, NULL, 1, &st) != EINVAL || lcb_hash_stream_import(NULL, NULL, 1, &st) != EINVAL)
		return 10;
	if (lcb_hash_stream_destroy(NULL) != EINVAL || lcb_hash_stream_count(NULL) != 0 || lcb_hash_stream_alg(NULL) != 0)
		return 11;
	puts("ok");
	return 0;
}
