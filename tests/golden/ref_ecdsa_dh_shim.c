/*
 * ref_ecdsa_dh_shim.c — C entry points around the key agreement of the
 * reference's header-only include/crypto/dsa/ecdsa.h (ecdsa_dh_be / _le), for
 * tests/golden/make_golden_ecdsa_dh.py and tools/ecdsa_dh_bench.py (compiled
 * into oracle/_ref/, only where the reference sources exist).  The
 * configuration is the one of ref_ecdsa_sign_shim.c.
 */
#include <sys/param.h>
#include <sys/types.h>
#include <errno.h>
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#define BN_DIGIT_BIT_CNT		64
#define BN_BIT_LEN			1408
#define BN_CC_MULL_DIV			1
#define BN_NO_POINTERS_CHK		1
#define BN_MOD_REDUCE_ALGO		BN_MOD_REDUCE_ALGO_BASIC
#define EC_USE_PROJECTIVE		1
#define EC_PROJ_REPEAT_DOUBLE		1
#define EC_PROJ_ADD_MIX			1
#define EC_PF_FXP_MULT_ALGO		EC_PF_FXP_MULT_ALGO_COMB_2T
#define EC_PF_FXP_MULT_WIN_BITS		9
#define EC_PF_UNKPT_MULT_ALGO		EC_PF_UNKPT_MULT_ALGO_COMB_1T
#define EC_PF_UNKPT_MULT_WIN_BITS	2
#define EC_PF_TWIN_MULT_ALGO		EC_PF_TWIN_MULT_ALGO_INTER

#include "crypto/dsa/ecdsa.h"

#define SLOTS 16
static ec_curve_t *slots[SLOTS];
static char slot_name[SLOTS][64];

/* Slot of the loaded curve `name` (loaded on first use), or -1. */
int
ref_dh_load(const char *name)
{
	int i;
	ec_curve_str_p cs;

	for (i = 0; i < SLOTS && slots[i] != NULL; i++)
		if (strcmp(slot_name[i], name) == 0)
			return i;
	if (i == SLOTS || strlen(name) >= sizeof(slot_name[0]))
		return -1;
	/* By strcmp: the table's name_size of one GOST test set is one short. */
	cs = NULL;
	for (size_t k = 0; k < nitems(ec_curve_str); k++)
		if (strcmp(ec_curve_str[k].name, name) == 0)
			cs = &ec_curve_str[k];
	if (cs == NULL)
		return -1;
	slots[i] = malloc(sizeof(ec_curve_t));
	if (slots[i] == NULL)
		return -1;
	if (ecdsa_curve_from_str(cs, slots[i]) != 0) {
		free(slots[i]);
		slots[i] = NULL;
		return -1;
	}
	strcpy(slot_name[i], name);
	return i;
}

/* All numbers 32 bytes, in the byte order of the form (le != 0: little-endian).
 * *size: the size the reference reports for the shared secret. */
int
ref_dh(int slot, int le, int use_cofactor, uint8_t *qx, uint8_t *qy,
    uint8_t *priv, uint8_t *shared, size_t *size)
{
	ec_curve_p c = (slot >= 0 && slot < SLOTS) ? slots[slot] : NULL;

	if (c == NULL)
		return EINVAL;
	if (le)
		return ecdsa_dh_le(c, use_cofactor, qx, qy, 32, priv, 32, shared, size);
	return ecdsa_dh_be(c, use_cofactor, qx, qy, 32, priv, 32, shared, size);
}

/* `count` agreements (timing aid): records are qx[32] qy[32] priv[32];
 * returns the number of non-zero results. */
long
ref_dh_many(int slot, int le, uint8_t *recs, size_t count)
{
	uint8_t shared[32];
	size_t i, size;
	long bad = 0;

	for (i = 0; i < count; i++) {
		uint8_t *p = recs + 96 * i;

		if (ref_dh(slot, le, 0, p, p + 32, p + 64, shared, &size) != 0)
			bad++;
	}
	return bad;
}
