#!/usr/bin/env python3
"""Generate tests/golden/ecdsa_wide_sign.json (run ONLY where the reference exists).

Pure data fixtures for the signing half of include/crypto/dsa/ecdsa.h on its
384- and 512-bit curves.  Every status and every output byte is produced by
the reference itself, compiled from its sources through
tests/golden/ref_ecdsa_wide_sign_shim.c into
oracle/_ref/libref_ecdsa_wide_sign.so (git-ignored).  tests/ecdsa_wide_model.py
is used only to choose inputs (the hash that makes s = 0); what those inputs
give is again asked of the reference, and where the model disagrees a NOTE is
printed.  The curves' numbers are those of tests/golden/ecdsa_wide.json.

groups
    Per (curve, form), the 8 groups of ecdsa_wide.json in that order:
    sign     {name, hash, hash_size, d, rnd, status, r, s}: the bytes passed to
             ecdsa_sign_be (le false) or ecdsa_sign_le (le true) with
             priv_key_size = rnd_size = B, and what it returned and wrote
    key_gen  {name, rnd, status, d, Qx, Qy} of ecdsa_key_gen_be / _le
    pub_key  {name, d, status, Qx, Qy} of ecdsa_recover_pub_key_from_priv_key_be / _le
    Outputs of a call that did not return 0 are recorded as zeros (the
    reference writes nothing there).  On disk a group stores every byte string
    once, in `nums`, and a record is a row of indices
    (tests/ecdsa_wide_sign_cases.py expands them again).
notes
    What cannot be exhibited on these curves.
ref_rate
    ecdsa_sign calls per second in the curve's natural form on one core of the
    generating machine.

Usage:  python3 tests/golden/make_golden_ecdsa_wide_sign.py <reference root>
"""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from tests import ecdsa_wide_model as M  # noqa: E402
from tests import ecdsa_wide_sign_cases as K  # noqa: E402

REF_SO = os.path.join(REPO, "oracle", "_ref", "libref_ecdsa_wide_sign.so")
OUT = K.FIXTURE


def build_ref(ref_root):
    hdr = os.path.join(ref_root, "include", "crypto", "dsa", "ecdsa.h")
    if not os.path.exists(hdr):
        raise SystemExit("%s is missing: this generator runs only where the reference exists" % hdr)
    os.makedirs(os.path.dirname(REF_SO), exist_ok=True)
    subprocess.check_call(["gcc", "-O2", "-w", "-fPIC", "-shared", "-I" + os.path.join(ref_root, "include"),
                           "-o", REF_SO, os.path.join(HERE, "ref_ecdsa_wide_sign_shim.c")])
    return load_ref()


def load_ref():
    L = ctypes.CDLL(REF_SO)
    L.ref_wide_sign_load.argtypes = [ctypes.c_char_p]
    L.ref_wide_sign_bytes.restype = ctypes.c_size_t
    L.ref_wide_sign_many.restype = ctypes.c_long
    return L


def buf(b):
    return (ctypes.c_uint8 * len(b)).from_buffer_copy(bytes(b))


class Ref:
    def __init__(self, L, name):
        self.L = L
        self.slot = L.ref_wide_sign_load(name.encode())
        assert self.slot >= 0, name
        self.B = L.ref_wide_sign_bytes(self.slot)
        assert self.B in (48, 64)

    def out(self, k):
        # A canary after each output: the reference must write B bytes and no more.
        return [(ctypes.c_uint8 * (self.B + 8))(*([0] * self.B + [0xA5] * 8)) for _ in range(k)]

    def take(self, st, bufs):
        for b in bufs:
            assert bytes(b)[self.B:] == b"\xa5" * 8
        return [bytes(b)[:self.B] if st == 0 else bytes(self.B) for b in bufs]

    def sign(self, le, h, hash_size, d, rnd):
        """(status, r, s): bytes in, bytes out; zeros unless the status is 0."""
        o = self.out(2)
        st = self.L.ref_wide_sign(self.slot, int(le), buf(h), ctypes.c_size_t(hash_size), buf(d), buf(rnd), *o)
        return (st, *self.take(st, o))

    def key_gen(self, le, rnd):
        o = self.out(3)
        sz = ctypes.c_size_t(0)
        st = self.L.ref_wide_key_gen(self.slot, int(le), buf(rnd), *o, ctypes.byref(sz))
        assert st != 0 or sz.value == self.B, sz.value
        return (st, *self.take(st, o))

    def pub_key(self, le, d):
        o = self.out(2)
        sz = ctypes.c_size_t(0)
        st = self.L.ref_wide_pub_key(self.slot, int(le), buf(d), *o, ctypes.byref(sz))
        assert st != 0 or sz.value == self.B, sz.value
        return (st, *self.take(st, o))

    def verify(self, le, h, hash_size, r, s, qx, qy):
        return self.L.ref_wide_verify(self.slot, int(le), buf(h), ctypes.c_size_t(hash_size), buf(r), buf(s), buf(qx),
                                      buf(qy))


def group_of(ref, c, le, rng):
    n, B = c["n"], c["bytes"]
    FF = (1 << (8 * B)) - 1
    rnd = lambda k=B: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    tb = lambda v: M.to_bytes(c, v, le)  # noqa: E731
    G = M.base(c)
    tag = "%s %s" % (c["name"], "le" if le else "be")
    sign, key_gen, pub_key = [], [], []

    def srec(name, h, d, k):
        """h, d, k: bytes as passed (h holds hash_size bytes)."""
        st, r, s = ref.sign(le, h, len(h), d, k)
        sign.append({"name": name, "hash": h.hex(), "hash_size": len(h), "d": d.hex(), "rnd": k.hex(), "status": st,
                     "r": r.hex(), "s": s.hex()})
        if st == 0 and M.num(d, le) != 0:  # a signature the reference itself accepts under the recovered key
            pst, qx, qy = ref.pub_key(le, d)
            assert pst == 0 and ref.verify(le, h, len(h), r, s, qx, qy) == 0, (tag, name)
        # the model chose inputs only: note where it disagrees with the reference
        if K.sign(c, h, len(h), d, k, le) != (st, r, s):
            print("NOTE model != reference: %s sign %s" % (tag, name))
        return st

    d0 = tb(M.num(rnd(), False) % (n - 1) + 1)
    for i in range(4):
        assert srec("valid_%d" % i, rnd(), tb(M.num(rnd(), False) % (n - 1) + 1), rnd()) == 0
    for hs in sorted({1, 20, B - 1, B, B + 1, 64, 65, 128}):
        assert srec("hash_size_%d" % hs, rnd(hs), d0, rnd()) == 0
    for nm, hv in (("hash_zero", 0), ("hash_eq_n", n), ("hash_n_minus_1", n - 1), ("hash_ff", FF)):
        assert srec(nm, tb(hv), d0, rnd()) == 0
    for nm, kv in (("k_zero", 0), ("k_one", 1), ("k_two", 2), ("k_n_minus_1", n - 1), ("k_eq_n", n),
                   ("k_n_plus_1", n + 1), ("k_ff", FF)):
        srec(nm, rnd(), d0, tb(kv))
    for nm, dv in (("d_zero", 0), ("d_one", 1), ("d_n_minus_1", n - 1), ("d_eq_n", n), ("d_ff", FF)):
        srec(nm, rnd(), tb(dv), rnd())
    assert srec("d_eq_n_k_zero", rnd(), tb(n), tb(0)) == M.EINVAL
    # s = 0: ECDSA e = -r d, GOST e = -r d k^-1 (mod n)
    while True:
        kv, dv = M.num(rnd(), False) % (n - 1) + 1, M.num(d0, le)
        r = M.mult(c, kv, G)[0] % n
        ev = (-r * dv) % n if c["algo"] == M.ALGO_ECDSA else (-r * dv * pow(kv, -1, n)) % n
        if r and ev:
            break
    assert srec("s_zero", tb(ev), d0, tb(kv)) == -1
    assert {0, -1, M.EINVAL} <= {k["status"] for k in sign}, tag

    for nm, v in (("rnd_zero", 0), ("rnd_one", 1), ("rnd_n_minus_1", n - 1), ("rnd_eq_n", n), ("rnd_ff", FF),
                  ("random_0", None), ("random_1", None), ("random_2", None)):
        k = rnd() if v is None else tb(v)
        st, d, qx, qy = ref.key_gen(le, k)
        key_gen.append({"name": nm, "rnd": k.hex(), "status": st, "d": d.hex(), "Qx": qx.hex(), "Qy": qy.hex()})
        if K.key_gen(c, k, le) != (st, d, qx, qy):
            print("NOTE model != reference: %s key_gen %s" % (tag, nm))
    for nm, v in (("d_zero", 0), ("d_one", 1), ("d_n_minus_1", n - 1), ("d_eq_n", n), ("d_ff", FF),
                  ("random_0", None), ("random_1", None), ("random_2", None)):
        d = tb(M.num(rnd(), False) % (n - 1) + 1) if v is None else tb(v)
        st, qx, qy = ref.pub_key(le, d)
        pub_key.append({"name": nm, "d": d.hex(), "status": st, "Qx": qx.hex(), "Qy": qy.hex()})
        if K.pub_key(c, d, le) != (st, qx, qy):
            print("NOTE model != reference: %s pub_key %s" % (tag, nm))
    return {"curve": c["name"], "le": le, "sign": sign, "key_gen": key_gen, "pub_key": pub_key}


def ref_rate(ref, grp, B):
    ok = [k for k in grp["sign"] if k["status"] == 0 and k["hash_size"] == B][:8]
    recs = b"".join(bytes.fromhex(k["hash"] + k["d"] + k["rnd"]) for k in ok) * 8
    b = buf(recs)
    t = time.perf_counter()
    assert ref.L.ref_wide_sign_many(ref.slot, int(grp["le"]), b, ctypes.c_size_t(len(recs) // (3 * B))) == 0
    return (len(recs) // (3 * B)) / (time.perf_counter() - t)


def pack_group(g):
    """The group with every byte string stored once, in `nums`, and its records
    as rows of indices into `nums`."""
    nums, where = [], {}
    out = {"curve": g["curve"], "le": g["le"]}
    for kind, fields in K.FIELDS.items():
        out[kind] = []
        for k in g[kind]:
            row = []
            for f in fields:
                v = k[f]
                if f in K.HEX_FIELDS:
                    if v not in where:
                        where[v] = len(nums)
                        nums.append(v)
                    v = where[v]
                row.append(v)
            out[kind].append(row)
    out["nums"] = nums
    return out


def write_fixture(fx, path):
    """JSON with one line per stored byte string and per record."""
    d = json.dumps
    out = ["{"] + ["%s: %s," % (d(k), d(fx[k])) for k in ("source", "ref_rate", "notes")]
    groups = []
    for g in fx["groups"]:
        parts = ['{"curve": %s, "le": %s' % (d(g["curve"]), d(g["le"])),
                 '"nums": [\n%s\n]' % ",\n".join(d(v) for v in g["nums"])]
        parts += ['"%s": [\n%s\n]' % (kind, ",\n".join(d(r) for r in g[kind])) for kind in K.FIELDS]
        groups.append(", ".join(parts) + "}")
    out += ['"groups": [', ",\n".join(groups), "]", "}"]
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref_root = sys.argv[1]
    L = build_ref(ref_root)
    vfx = M.load_fixture()
    curves = M.load_curves(vfx)
    rng = np.random.default_rng(0x5167EC05A512)
    groups, rates, notes = [], {}, {}
    for g in vfx["cases"]:  # the same (curve, form) groups, in the same order
        c = curves[g["curve"]]
        ref = Ref(L, g["curve"])
        assert ref.B == c["bytes"]
        grp = group_of(ref, c, bool(g["le"]), rng)
        groups.append(grp)
        if grp["le"] == (c["algo"] == M.ALGO_GOST):
            rates[g["curve"]] = round(ref_rate(ref, grp, ref.B), 1)
        assert c["Gx"] != 0
        notes[g["curve"]] = ("r = 0 is not exhibited: Gx != 0, so no small nonce gives it.  A valid signature with "
                             "R.x >= n is not exhibited: |p - n| < 2^%d against n > 2^%d; not searched."
                             % ((abs(c["p"] - c["n"])).bit_length(), c["n"].bit_length() - 1))
    write_fixture({"source": "include/crypto/dsa/ecdsa.h compiled from the reference (oracle/_ref), configuration of "
                             "tests/golden/ref_ecdsa_wide_shim.c",
                   "ref_rate": {"what": "ecdsa_sign calls per second in the curve's natural form, one core of the "
                                        "generating machine, gcc -O2",
                                "per_curve": rates},
                   "notes": notes, "groups": [pack_group(g) for g in groups]}, OUT)
    assert K.load_fixture()["groups"] == groups
    print("ecdsa_wide_sign.json: %d groups, %d sign, %d key_gen, %d pub_key records, %d bytes" % (
        len(groups), sum(len(g["sign"]) for g in groups), sum(len(g["key_gen"]) for g in groups),
        sum(len(g["pub_key"]) for g in groups), os.path.getsize(OUT)))
    for g in groups:
        print("%-45s %s" % (g["curve"], "le" if g["le"] else "be"),
              {k["name"]: k["status"] for k in g["sign"] if k["status"]},
              {k["name"]: k["status"] for k in g["key_gen"] + g["pub_key"] if k["status"]})
    print("reference signs/s:", rates)


if __name__ == "__main__":
    main()
