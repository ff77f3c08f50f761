"""Python-int model of the per-item contract of include/lcb_ecdsa_wide_gpu.h:
tests/ecdsa_model.py with the number size B = (m + 7) / 8 (48 or 64) taken
from the curve instead of fixed at 32.  The group law, bn_mod_reduce and the
byte-order helpers are those of ecdsa_model; only what imports a hash or
writes a number is restated.  Curves are dicts {name, algo, h, p, a, b, Gx,
Gy, n, bytes} with ints, as load_curves() makes them from
tests/golden/ecdsa_wide.json.
"""
import json
import os

from tests.ecdsa_model import (ALGO_ECDSA, ALGO_GOST, EINVAL, NUMS, add, base, mod_reduce, mult, num,  # noqa: F401
                               on_curve, public_key)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ecdsa_wide.json")


# A group of the fixture stores every byte string once, in `nums`; a record is
# a row over these fields, the HEX_FIELDS as indices into `nums`.
CASE_FIELDS = ("name", "hash", "hash_size", "r", "s", "Qx", "Qy", "status")
MESSAGE_FIELDS = ("msg", "hash", "r", "s", "Qx", "Qy", "status")
HEX_FIELDS = ("msg", "hash", "r", "s", "Qx", "Qy")


def expand_group(g, fields):
    """The group with its records as dicts {field: value, le}, byte strings as hex."""
    recs = [dict({f: g["nums"][v] if f in HEX_FIELDS else v for f, v in zip(fields, row)}, le=g["le"])
            for row in g["records"]]
    return dict({f: v for f, v in g.items() if f not in ("nums", "records")}, records=recs)


def load_fixture():
    with open(FIXTURE) as f:
        fx = json.load(f)
    fx["cases"] = [expand_group(g, CASE_FIELDS) for g in fx["cases"]]
    fx["messages"] = [expand_group(g, MESSAGE_FIELDS) for g in fx["messages"]]
    return fx


def curve_from_json(c):
    out = {"name": c["name"], "algo": c["algo"], "h": c["h"], "bytes": c["bytes"]}
    for k in NUMS:
        out[k] = int(c[k], 16)
    return out


def load_curves(fx=None):
    return {c["name"]: curve_from_json(c) for c in (fx or load_fixture())["curves"]}


def to_bytes(c, v, le):
    return v.to_bytes(c["bytes"], "little" if le else "big")


def hash_number(c, h, hash_size, le):
    return mod_reduce(num(bytes(h)[:min(hash_size, c["bytes"])], le), c["n"])


def verify(c, h, hash_size, r, s, qx, qy, le=False):
    """Status of ecdsa_verify_{be,le}(curve, h, hash_size, r, s, B, qx, qy, B)."""
    p, n = c["p"], c["n"]
    x, y, r, s = num(qx, le), num(qy, le), num(r, le), num(s, le)
    if x >= p or y >= p or not on_curve(c, x, y):
        return -1  # h = 1 on every supported curve: n * Q = O follows
    e = hash_number(c, h, hash_size, le)
    if r >= n or s >= n:
        return EINVAL
    if c["algo"] == ALGO_ECDSA:
        if s == 0:
            return EINVAL  # no inverse of 0
        w = pow(s, -1, n)
        u1, u2 = e * w % n, r * w % n
    else:
        if e == 0:
            e = 1
        w = pow(e, -1, n)
        u1, u2 = s * w % n, (n - w) * r % n
    R = add(c, mult(c, u1, base(c)), mult(c, u2, (x, y)))
    if R is None:
        return -1
    return 0 if R[0] % n == r else -2


def sign(c, h, hash_size, d, k, le=False):
    """(r, s) as ints, as the reference's ecdsa_sign makes them from the
    nonce k (reduced as the reference reduces it); None where it fails."""
    n = c["n"]
    k = mod_reduce(k, n)
    R = mult(c, k, base(c))
    if R is None or R[0] % n == 0:
        return None
    r = R[0] % n
    e = hash_number(c, h, hash_size, le)
    if c["algo"] == ALGO_ECDSA:
        s = pow(k, -1, n) * (e + d * r) % n
    else:
        s = ((k * e if e else k) + d * r) % n
    return (r, s) if s else None
