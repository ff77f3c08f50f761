"""tests/golden/ecdsa_wide_sign.json for its readers: the fixture of
include/lcb_ecdsa_wide_sign_gpu.h, expanded from its packed form, and the
Python-int model of the two key calls (signing is tests/ecdsa_wide_model.sign).

On disk a group stores every byte string once, in `nums`, and a record of its
`sign`, `key_gen` and `pub_key` lists is a row over the fields below with
indices into `nums`, as tests/golden/ecdsa_wide.json does it."""
import json
import os

from tests import ecdsa_wide_model as M

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ecdsa_wide_sign.json")

FIELDS = {"sign": ("name", "hash", "hash_size", "d", "rnd", "status", "r", "s"),
          "key_gen": ("name", "rnd", "status", "d", "Qx", "Qy"),
          "pub_key": ("name", "d", "status", "Qx", "Qy")}
HEX_FIELDS = ("hash", "d", "rnd", "r", "s", "Qx", "Qy")


def expand_group(g):
    """The group with its three record lists as dicts, byte strings as hex."""
    out = {f: v for f, v in g.items() if f != "nums" and f not in FIELDS}
    for kind, fields in FIELDS.items():
        out[kind] = [{f: g["nums"][v] if f in HEX_FIELDS else v for f, v in zip(fields, row)} for row in g[kind]]
    return out


def load_fixture():
    with open(FIXTURE) as f:
        fx = json.load(f)
    fx["groups"] = [expand_group(g) for g in fx["groups"]]
    return fx


def key_gen(c, rnd, le):
    """(status, d, Qx, Qy) as ecdsa_key_gen_{be,le}: bytes in, bytes out, zeros
    unless the status is 0."""
    B = c["bytes"]
    d = M.mod_reduce(M.num(rnd, le), c["n"])
    if d == 0:
        return -1, bytes(B), bytes(B), bytes(B)
    x, y = M.public_key(c, d)
    return 0, M.to_bytes(c, d, le), M.to_bytes(c, x, le), M.to_bytes(c, y, le)


def pub_key(c, d, le):
    """(status, Qx, Qy) as ecdsa_recover_pub_key_from_priv_key_{be,le}."""
    B = c["bytes"]
    d = M.num(d, le)
    if d >= c["n"]:
        return M.EINVAL, bytes(B), bytes(B)
    if d == 0:
        return -1, bytes(B), bytes(B)
    x, y = M.public_key(c, d)
    return 0, M.to_bytes(c, x, le), M.to_bytes(c, y, le)


def sign(c, h, hash_size, d, rnd, le):
    """(status, r, s) as ecdsa_sign_{be,le}."""
    B = c["bytes"]
    dv = M.num(d, le)
    if dv >= c["n"]:
        return M.EINVAL, bytes(B), bytes(B)
    m = M.sign(c, h, hash_size, dv, M.num(rnd, le), le)
    if m is None:
        return -1, bytes(B), bytes(B)
    return 0, M.to_bytes(c, m[0], le), M.to_bytes(c, m[1], le)

