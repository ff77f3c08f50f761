"""Python-int model of the per-item contract of include/lcb_ecdsa_gpu.h:
what the reference's ecdsa_verify_be / ecdsa_verify_le return for 256-bit
curves with bytes = 32, over affine arithmetic and pow(x, -1, m).  Also the
reference's ecdsa_sign (for tests and tools that need valid signatures
without the reference).  Curves are dicts {name, algo, h, p, a, b, Gx, Gy, n}
with ints, as load_curves() makes them from tests/golden/ecdsa.json.
"""
import errno
import json
import os

EINVAL = errno.EINVAL
ALGO_ECDSA, ALGO_GOST = 0, 1
NUMS = ("p", "a", "b", "Gx", "Gy", "n")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ecdsa.json")


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def curve_from_json(c):
    out = {"name": c["name"], "algo": c["algo"], "h": c["h"]}
    for k in NUMS:
        out[k] = int(c[k], 16)
    return out


def load_curves(fx=None):
    return {c["name"]: curve_from_json(c) for c in (fx or load_fixture())["curves"]}


# ---------------------------------------------------------------- the group
def on_curve(c, x, y):
    return (y * y - (x * x * x + c["a"] * x + c["b"])) % c["p"] == 0


def add(c, P, Q):
    """Affine addition; None is the point at infinity."""
    if P is None:
        return Q
    if Q is None:
        return P
    p = c["p"]
    (x1, y1), (x2, y2) = P, Q
    if x1 == x2:
        if (y1 + y2) % p == 0:
            return None
        lam = (3 * x1 * x1 + c["a"]) * pow(2 * y1, -1, p) % p
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
    x3 = (lam * lam - x1 - x2) % p
    return x3, (lam * (x1 - x3) - y1) % p


def mult(c, k, P):
    R = None
    while k:
        if k & 1:
            R = add(c, R, P)
        P = add(c, P, P)
        k >>= 1
    return R


def base(c):
    return c["Gx"], c["Gy"]


# ------------------------------------------------------------ the reference
def num(b, le):
    return int.from_bytes(b, "little" if le else "big")


def to_bytes(v, le, size=32):
    return v.to_bytes(size, "little" if le else "big")


def mod_reduce(v, m):
    """The reference's bn_mod_reduce: v itself below m, else (v mod (m - 1)) + 1."""
    return v if v < m else v % (m - 1) + 1


def hash_number(c, h, hash_size, le):
    return mod_reduce(num(bytes(h)[:min(hash_size, 32)], le), c["n"])


def verify(c, h, hash_size, r, s, qx, qy, le=False):
    """Status of ecdsa_verify_{be,le}(curve, h, hash_size, r, s, 32, qx, qy, 32)."""
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


def public_key(c, d):
    return mult(c, d, base(c))


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
