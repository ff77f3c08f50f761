/*
 * gost28147_caller.c — a plain C caller of include/lcb_gost28147_gpu.h.
 * Checks what needs no GPU: the parameter sets, the packed table and the
 * argument errors; prints "ok" and exits 0.
 */
#include <errno.h>
#include <stdio.h>
#include <string.h>

#include "lcb_gost28147_gpu.h"

int
main(void)
{
	uint8_t key[32] = {0}, buf[64] = {0}, macs[8];
	uint32_t table[256];
	const uint8_t *z = lcb_gost28147_sbox(5);
	int id;

	for (id = 0; id < 6; id++)
		if (lcb_gost28147_sbox(id) == NULL)
			return 1;
	if (lcb_gost28147_sbox(6) != NULL || lcb_gost28147_sbox(-1) != NULL)
		return 2;
	/* id-tc26-gost-28147-param-Z starts c 4 6 2 */
	if (z[0] != 0xc || z[1] != 4 || z[2] != 6 || z[3] != 2)
		return 3;
	if (lcb_gost28147_gpu_table(z, table) != 0 || lcb_gost28147_gpu_table(NULL, table) != EINVAL)
		return 4;
	if (gost28147_blocks_encrypt_batch(key, 16, z, buf, buf, NULL, NULL, 1, 0, 64, 0, NULL) != EINVAL)
		return 5;
	if (gost28147_blocks_decrypt_be_batch(key, 32, z, buf, buf, NULL, NULL, 1, 0, 60, 0, NULL) != EINVAL)
		return 6;
	if (gost28147_blocks_mac_batch(key, 32, z, buf, NULL, NULL, 1, 0, 64, macs, 9, 0, NULL) != EINVAL)
		return 7;
	if (gost28147_blocks_mac_be_batch(key, 32, z, buf, NULL, NULL, 0, 0, 64, macs, 8, 0, NULL) != 0)
		return 8;
	puts("ok");
	return 0;
}
