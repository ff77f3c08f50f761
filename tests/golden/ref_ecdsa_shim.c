/*
 * ref_ecdsa_shim.c — C entry points around the reference's header-only
 * include/crypto/dsa/ecdsa.h, for tests/golden/make_golden_ecdsa.py and
 * tools/ecdsa_bench.py (compiled into oracle/_ref/, only where the reference
 * sources exist).  The configuration is the one of the reference's
 * tests/ecdsa/main.c without EC_DISABLE_PUB_KEY_CHK (the public key check is
 * part of the contract), BN_SELF_TEST and EC_SELF_TEST.
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
ref_ecdsa_load(const char *name)
{
	int i;
	ec_curve_str_p cs;

	for (i = 0; i < SLOTS && slots[i] != NULL; i++)
		if (strcmp(slot_name[i], name) == 0)
			return i;
	if (i == SLOTS || strlen(name) >= sizeof(slot_name[0]))
		return -1;
	/* Not ecdsa_curve_str_get_by_name: it compares name_size first, and the
	 * table's name_size of id-gostR3410-2001-Test_ParamSet is one short. */
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

/* The loaded curve's numbers: p, a, b, Gx, Gy, n as 6 x 32 big-endian bytes. */
int
ref_ecdsa_params(int slot, uint8_t *out, uint32_t *algo, uint32_t *h, uint32_t *bits)
{
	ec_curve_p c = curve_of(slot);
	bn_p v[6];
	int i, error;

	if (c == NULL)
		return EINVAL;
	v[0] = &c->p; v[1] = &c->a; v[2] = &c->b;
	v[3] = &c->G.x; v[4] = &c->G.y; v[5] = &c->n;
	for (i = 0; i < 6; i++) {
		error = bn_export_be_bin(v[i], 0, out + 32 * i, 32, NULL);
		if (error != 0)
			return error;
	}
	*algo = c->algo;
	*h = c->h;
	*bits = (uint32_t)c->m;
	return 0;
}

/* rnd: 32 big-endian bytes; priv, qx, qy: 32 big-endian bytes each. */
int
ref_ecdsa_key_gen_be(int slot, uint8_t *rnd, uint8_t *priv, uint8_t *qx, uint8_t *qy)
{
	ec_curve_p c = curve_of(slot);
	size_t psz = 0, qsz = 0;

	if (c == NULL)
		return EINVAL;
	return ecdsa_key_gen_be(c, rnd, 32, 0, priv, &psz, qx, qy, &qsz);
}

/* All numbers 32 bytes, in the byte order of the form (le != 0: little-endian). */
int
ref_ecdsa_sign(int slot, int le, uint8_t *hash, size_t hash_size, uint8_t *priv,
    uint8_t *rnd, uint8_t *r, uint8_t *s)
{
	ec_curve_p c = curve_of(slot);
	size_t sz = 0;

	if (c == NULL)
		return EINVAL;
	if (le)
		return ecdsa_sign_le(c, hash, hash_size, priv, 32, rnd, 32, r, s, &sz);
	return ecdsa_sign_be(c, hash, hash_size, priv, 32, rnd, 32, r, s, &sz);
}

int
ref_ecdsa_verify(int slot, int le, uint8_t *hash, size_t hash_size, uint8_t *r,
    uint8_t *s, uint8_t *qx, uint8_t *qy)
{
	ec_curve_p c = curve_of(slot);

	if (c == NULL)
		return EINVAL;
	if (le)
		return ecdsa_verify_le(c, hash, hash_size, r, s, 32, qx, qy, 32);
	return ecdsa_verify_be(c, hash, hash_size, r, s, 32, qx, qy, 32);
}

/* The same call `reps` times over `count` records (timing aid): records are
 * hash[32] r[32] s[32] qx[32] qy[32]; returns the number of non-zero results. */
long
ref_ecdsa_verify_many(int slot, int le, uint8_t *recs, size_t count)
{
	size_t i;
	long bad = 0;

	for (i = 0; i < count; i++) {
		uint8_t *p = recs + 160 * i;

		if (ref_ecdsa_verify(slot, le, p, 32, p + 32, p + 64, p + 96, p + 128) != 0)
			bad++;
	}
	return bad;
}
