/*
 * ref_ecdsa_key_shim.c — C entry points around the public-key import and
 * export of the reference's header-only include/crypto/dsa/ecdsa.h
 * (ecdsa_pub_key_import_be / _le, ecdsa_pub_key_export_be / _le), for
 * tests/golden/make_golden_ecdsa_key.py and tools/ecdsa_key_bench.py (compiled
 * into oracle/_ref/, only where the reference sources exist).  The
 * configuration is the one of ref_ecdsa_dh_shim.c, the public key check on.
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
ref_key_load(const char *name)
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

static ec_curve_p
curve_of(int slot)
{
	return (slot >= 0 && slot < SLOTS) ? slots[slot] : NULL;
}

/*
 * The reference's import of key[0 .. size) (key_y may be NULL), and on 0 what
 * its export of the imported point writes: xy = x || y, 32 bytes each, in the
 * byte order of the form, *inf = 0; or *inf = 1 for the point at infinity
 * (xy untouched).  On any other status nothing is written.
 */
int
ref_key_import(int slot, int le, uint8_t *key, uint8_t *key_y, size_t size,
    uint8_t *xy, int *inf)
{
	ec_curve_p c = curve_of(slot);
	ec_point_t pt;
	uint8_t one[8];
	size_t out_size = 0;
	int st;

	if (c == NULL)
		return EINVAL;
	if (ec_point_init(&pt, c->m) != 0)
		return EINVAL;
	st = le ? ecdsa_pub_key_import_le(c, key, key_y, size, &pt) :
	    ecdsa_pub_key_import_be(c, key, key_y, size, &pt);
	if (st != 0)
		return st;
	*inf = 0;
	if (ec_point_is_at_infinity(&pt)) {
		st = le ? ecdsa_pub_key_export_le(c, 0, &pt, one, one + 4, &out_size) :
		    ecdsa_pub_key_export_be(c, 0, &pt, one, one + 4, &out_size);
		if (st != 0 || out_size != 1 || one[0] != 0)
			return 1000;
		*inf = 1;
		return 0;
	}
	st = le ? ecdsa_pub_key_export_le(c, 0, &pt, xy, xy + 32, &out_size) :
	    ecdsa_pub_key_export_be(c, 0, &pt, xy, xy + 32, &out_size);
	if (st != 0 || out_size != 32)
		return 1001;
	return 0;
}

/*
 * The reference's export of the point (x, y) = xy (32 bytes each, byte order
 * of the form; nothing is validated, as the reference validates nothing) or
 * of the point at infinity, in the one-buffer forms: compress != 0 the
 * compressed form, else the packed form.  out has room for 65 bytes.
 */
int
ref_key_export(int slot, int le, int compress, uint8_t *xy, int inf,
    uint8_t *out, size_t *size)
{
	ec_curve_p c = curve_of(slot);
	ec_point_t pt;

	if (c == NULL)
		return EINVAL;
	if (ec_point_init(&pt, c->m) != 0)
		return EINVAL;
	if (le) {
		if (bn_import_le_bin(&pt.x, xy, 32) != 0 ||
		    bn_import_le_bin(&pt.y, xy + 32, 32) != 0)
			return EINVAL;
	} else {
		if (bn_import_be_bin(&pt.x, xy, 32) != 0 ||
		    bn_import_be_bin(&pt.y, xy + 32, 32) != 0)
			return EINVAL;
	}
	pt.infinity = inf ? 1 : 0;
	if (le)
		return ecdsa_pub_key_export_le(c, compress, &pt, out, NULL, size);
	return ecdsa_pub_key_export_be(c, compress, &pt, out, NULL, size);
}

/* `count` imports (timing aid): keys of `size` bytes every `stride` bytes;
 * returns the number of non-zero results. */
long
ref_key_import_many(int slot, int le, uint8_t *keys, size_t stride, size_t size,
    size_t count)
{
	ec_curve_p c = curve_of(slot);
	ec_point_t pt;
	size_t i;
	long bad = 0;

	if (c == NULL || ec_point_init(&pt, c->m) != 0)
		return -1;
	for (i = 0; i < count; i++) {
		int st = le ?
		    ecdsa_pub_key_import_le(c, keys + i * stride, NULL, size, &pt) :
		    ecdsa_pub_key_import_be(c, keys + i * stride, NULL, size, &pt);

		if (st != 0)
			bad++;
	}
	return bad;
}
