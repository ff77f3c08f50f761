/*
 * radius_caller.c — a plain C caller of include/lcb_radius_gpu.h.
 * Checks what needs no GPU: every call-level EINVAL is decided before HIP
 * is touched and an empty batch returns 0; prints "ok" and exits 0.
 */
#include <errno.h>
#include <stdio.h>
#include <string.h>

#include "lcb_hash_gpu.h"
#include "lcb_radius_gpu.h"

int
main(void)
{
	uint8_t pkts[128] = {0}, req[40] = {0};
	const uint8_t key[] = "testing123";
	const uint32_t klen[1] = {10};
	int32_t err[2] = {-1, -1};

	if (radius_pkt_sign_batch(NULL, NULL, NULL, 2, 64, 64, key, NULL, klen, 1, NULL, err, 0, NULL) != EINVAL)
		return 1;
	if (radius_pkt_sign_batch(pkts, NULL, NULL, 2, 64, 64, key, NULL, klen, 1, NULL, NULL, 0, NULL) != EINVAL)
		return 2;
	if (radius_pkt_sign_batch(pkts, NULL, NULL, 2, 64, 64, NULL, NULL, klen, 1, NULL, err, 0, NULL) != EINVAL)
		return 3;
	if (radius_pkt_sign_batch(pkts, NULL, NULL, 2, 64, 64, key, NULL, klen, 0, NULL, err, 0, NULL) != EINVAL)
		return 4;
	if (radius_pkt_sign_batch(pkts, NULL, NULL, 2, 64, 64, key, NULL, NULL, 1, NULL, err, 0, NULL) != EINVAL)
		return 5;
	if (radius_pkt_sign_batch(pkts, NULL, NULL, 2, 64, 64, key, NULL, klen, 1, NULL, err, 0x10, NULL) != EINVAL)
		return 6;
	if (radius_pkt_sign_batch(pkts, NULL, NULL, 2, 64, 19, key, NULL, klen, 1, NULL, err, 0, NULL) != EINVAL)
		return 7;
	if (radius_pkt_sign_batch(pkts, NULL, NULL, 2, 63, 64, key, NULL, klen, 1, NULL, err, 0, NULL) != EINVAL)
		return 8;
	if (radius_pkt_verify_batch(pkts, NULL, NULL, 2, 63, 64, key, NULL, klen, 1, NULL, req, err, 0, NULL) != EINVAL)
		return 9;
	if (radius_pkt_verify_batch(pkts, NULL, NULL, 2, 64, 64, key, NULL, klen, 1, NULL, req, err,
	    LCB_HASH_F_DEVICE | 2u, NULL) != EINVAL)
		return 10;
	if (radius_pkt_sign_batch(pkts, NULL, NULL, 0, 64, 64, key, NULL, klen, 1, NULL, err, 0, NULL) != 0)
		return 11;
	if (radius_pkt_verify_batch(pkts, NULL, NULL, 0, 64, 64, key, NULL, klen, 1, NULL, NULL, err, 0, NULL) != 0)
		return 12;
	if (err[0] != -1 || err[1] != -1)
		return 13;
	puts("ok");
	return 0;
}
