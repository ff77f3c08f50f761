/*
 * ref_ecdsa_wide_shim.c — C entry points around the reference's header-only
 * include/crypto/dsa/ecdsa.h for its 384- and 512-bit curves, for
 * tests/golden/make_golden_ecdsa_wide.py and tools/ecdsa_wide_bench.py
 * (compiled into oracle/_ref/libref_ecdsa_wide.so, only where the reference
 * sources exist).  The configuration is the one of ref_ecdsa_shim.c:
 * BN_BIT_LEN 1408 already covers 512-bit numbers.  Every number is B bytes,
 * B = (m + 7) / 8 of the loaded curve (ref_ecdsa_wide_params reports m).
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
ref_ecdsa_wide_load(const char *name)
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

static size_t
bytes_of(ec_curve_p c)
{
	return (c->m + 7) / 8;
}

/* The loaded curve's numbers: p, a, b, Gx, Gy, n as 6 x B big-endian bytes
 * (out holds 6 x 64). */
int
ref_ecdsa_wide_params(int slot, uint8_t *out, uint32_t *algo, uint32_t *h, uint32_t *bits)
{
	ec_curve_p c = curve_of(slot);
	bn_p v[6];
	size_t B;
	int i, error;

	if (c == NULL)
		return EINVAL;
	B = bytes_of(c);
	if (B > 64)
		return EINVAL;
	v[0] = &c->p; v[1] = &c->a; v[2] = &c->b;
	v[3] = &c->G.x; v[4] = &c->G.y; v[5] = &c->n;
	for (i = 0; i < 6; i++) {
		error = bn_export_be_bin(v[i], 0, out + B * i, B, NULL);
		if (error != 0)
			return error;
	}
	*algo = c->algo;
	*h = c->h;
	*bits = (uint32_t)c->m;
	return 0;
}

/* rnd, priv, qx, qy: B big-endian bytes each. */
int
ref_ecdsa_wide_key_gen_be(int slot, uint8_t *rnd, uint8_t *priv, uint8_t *qx, uint8_t *qy)
{
	ec_curve_p c = curve_of(slot);
	size_t psz = 0, qsz = 0;

	if (c == NULL)
		return EINVAL;
	return ecdsa_key_gen_be(c, rnd, bytes_of(c), 0, priv, &psz, qx, qy, &qsz);
}

/* All numbers B bytes, in the byte order of the form (le != 0: little-endian). */
int
ref_ecdsa_wide_sign(int slot, int le, uint8_t *hash, size_t hash_size, uint8_t *priv,
    uint8_t *rnd, uint8_t *r, uint8_t *s)
{
	ec_curve_p c = curve_of(slot);
	size_t sz = 0, B;

	if (c == NULL)
		return EINVAL;
	B = bytes_of(c);
	if (le)
		return ecdsa_sign_le(c, hash, hash_size, priv, B, rnd, B, r, s, &sz);
	return ecdsa_sign_be(c, hash, hash_size, priv, B, rnd, B, r, s, &sz);
}

int
ref_ecdsa_wide_verify(int slot, int le, uint8_t *hash, size_t hash_size, uint8_t *r,
    uint8_t *s, uint8_t *qx, uint8_t *qy)
{
	ec_curve_p c = curve_of(slot);
	size_t B;

	if (c == NULL)
		return EINVAL;
	B = bytes_of(c);
	if (le)
		return ecdsa_verify_le(c, hash, hash_size, r, s, B, qx, qy, B);
	return ecdsa_verify_be(c, hash, hash_size, r, s, B, qx, qy, B);
}

/* The same call over `count` records (timing aid): records are
 * hash[B] r[B] s[B] qx[B] qy[B]; returns the number of non-zero results. */
long
ref_ecdsa_wide_verify_many(int slot, int le, uint8_t *recs, size_t count)
{
	ec_curve_p c = curve_of(slot);
	size_t i, B;
	long bad = 0;

	if (c == NULL)
		return -1;
	B = bytes_of(c);
	for (i = 0; i < count; i++) {
		uint8_t *p = recs + 5 * B * i;

		if (ref_ecdsa_wide_verify(slot, le, p, B, p + B, p + 2 * B, p + 3 * B, p + 4 * B) != 0)
			bad++;
	}
	return bad;
}
