/*
 * ref_ecdsa_wide_sign_shim.c — C entry points around the signing half of the
 * reference's header-only include/crypto/dsa/ecdsa.h (ecdsa_sign_be / _le,
 * ecdsa_key_gen_be / _le, ecdsa_recover_pub_key_from_priv_key_be / _le) on its
 * 384- and 512-bit curves, for tests/golden/make_golden_ecdsa_wide_sign.py and
 * tools/ecdsa_wide_sign_bench.py (compiled into
 * oracle/_ref/libref_ecdsa_wide_sign.so, only where the reference sources
 * exist).  The configuration is the one of ref_ecdsa_wide_shim.c.  Every
 * number is B bytes, B = (m + 7) / 8 of the loaded curve.
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

#define SLOTS 8
static ec_curve_t *slots[SLOTS];
static char slot_name[SLOTS][64];

/* Slot of the loaded curve `name` (loaded on first use), or -1. */
int
ref_wide_sign_load(const char *name)
{
	int i;
	ec_curve_str_p cs;

	for (i = 0; i < SLOTS && slots[i] != NULL; i++)
		if (strcmp(slot_name[i], name) == 0)
			return i;
	if (i == SLOTS || strlen(name) >= sizeof(slot_name[0]))
		return -1;
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

static ec_curve_p
curve_of(int slot)
{
	return (slot >= 0 && slot < SLOTS) ? slots[slot] : NULL;
}

/* B of the loaded curve, 0 for no curve. */
size_t
ref_wide_sign_bytes(int slot)
{
	ec_curve_p c = curve_of(slot);

	return c != NULL ? (c->m + 7) / 8 : 0;
}

/* All numbers B bytes, in the byte order of the form (le != 0: little-endian). */
int
ref_wide_sign(int slot, int le, uint8_t *hash, size_t hash_size, uint8_t *priv,
    uint8_t *rnd, uint8_t *r, uint8_t *s)
{
	ec_curve_p c = curve_of(slot);
	size_t B = ref_wide_sign_bytes(slot);

	if (c == NULL)
		return EINVAL;
	if (le)
		return ecdsa_sign_le(c, hash, hash_size, priv, B, rnd, B, r, s, NULL);
	return ecdsa_sign_be(c, hash, hash_size, priv, B, rnd, B, r, s, NULL);
}

/* *size: the public key size the reference reports (B for an (x, y) pair). */
int
ref_wide_key_gen(int slot, int le, uint8_t *rnd, uint8_t *priv, uint8_t *qx,
    uint8_t *qy, size_t *size)
{
	ec_curve_p c = curve_of(slot);
	size_t B = ref_wide_sign_bytes(slot);

	if (c == NULL)
		return EINVAL;
	if (le)
		return ecdsa_key_gen_le(c, rnd, B, 0, priv, NULL, qx, qy, size);
	return ecdsa_key_gen_be(c, rnd, B, 0, priv, NULL, qx, qy, size);
}

int
ref_wide_pub_key(int slot, int le, uint8_t *priv, uint8_t *qx, uint8_t *qy,
    size_t *size)
{
	ec_curve_p c = curve_of(slot);
	size_t B = ref_wide_sign_bytes(slot);

	if (c == NULL)
		return EINVAL;
	if (le)
		return ecdsa_recover_pub_key_from_priv_key_le(c, priv, B, 0, qx, qy, size);
	return ecdsa_recover_pub_key_from_priv_key_be(c, priv, B, 0, qx, qy, size);
}

int
ref_wide_verify(int slot, int le, uint8_t *hash, size_t hash_size, uint8_t *r,
    uint8_t *s, uint8_t *qx, uint8_t *qy)
{
	ec_curve_p c = curve_of(slot);
	size_t B = ref_wide_sign_bytes(slot);

	if (c == NULL)
		return EINVAL;
	if (le)
		return ecdsa_verify_le(c, hash, hash_size, r, s, B, qx, qy, B);
	return ecdsa_verify_be(c, hash, hash_size, r, s, B, qx, qy, B);
}

/* `count` signatures (timing aid): records are hash[B] priv[B] rnd[B];
 * returns the number of non-zero results. */
long
ref_wide_sign_many(int slot, int le, uint8_t *recs, size_t count)
{
	uint8_t r[64], s[64];
	size_t i, B = ref_wide_sign_bytes(slot);
	long bad = 0;

	if (B == 0 || B > 64)
		return -1;
	for (i = 0; i < count; i++) {
		uint8_t *p = recs + 3 * B * i;

		if (ref_wide_sign(slot, le, p, B, p + B, p + 2 * B, r, s) != 0)
			bad++;
	}
	return bad;
}
