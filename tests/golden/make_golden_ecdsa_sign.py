#!/usr/bin/env python3
"""Generate tests/golden/ecdsa_sign.json (run ONLY where the reference exists).

Pure data fixtures for the signing half of include/crypto/dsa/ecdsa.h.  Every
status and every output byte is produced by the reference itself, compiled
from its sources through tests/golden/ref_ecdsa_sign_shim.c into
oracle/_ref/libref_ecdsa_sign.so (git-ignored).  tests/ecdsa_model.py is used
only to choose inputs (the hash that makes s = 0, a nonce whose R.x is >= n);
what those inputs give is again asked of the reference.  The curves' numbers
are those of tests/golden/ecdsa.json.

groups
    Per (curve, form), the 12 groups of ecdsa.json:
    sign     {name, hash, hash_size, d, rnd, status, r, s}: the bytes passed to
             ecdsa_sign_be (le false) or ecdsa_sign_le (le true) with
             priv_key_size = rnd_size = 32, and what it returned and wrote
    key_gen  {name, rnd, status, d, Qx, Qy} of ecdsa_key_gen_be / _le
    pub_key  {name, d, status, Qx, Qy} of ecdsa_recover_pub_key_from_priv_key_be / _le
    Outputs of a call that did not return 0 are recorded as zeros (the
    reference writes nothing there).
ref_rate
    ecdsa_sign_be calls per second on one core of the generating machine.

Usage:  python3 tests/golden/make_golden_ecdsa_sign.py [reference root]
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
from tests import ecdsa_model as M  # noqa: E402

REF_SO = os.path.join(REPO, "oracle", "_ref", "libref_ecdsa_sign.so")
OUT = os.path.join(HERE, "ecdsa_sign.json")
FF = (1 << 256) - 1
ZERO = "00" * 32


def build_ref(ref_root):
    hdr = os.path.join(ref_root, "include", "crypto", "dsa", "ecdsa.h")
    if not os.path.exists(hdr):
        raise SystemExit("%s is missing: this generator runs only where the reference exists" % hdr)
    os.makedirs(os.path.dirname(REF_SO), exist_ok=True)
    subprocess.check_call(["gcc", "-O2", "-w", "-fPIC", "-shared", "-I" + os.path.join(ref_root, "include"),
                           "-o", REF_SO, os.path.join(HERE, "ref_ecdsa_sign_shim.c")])
    return load_ref()


def load_ref():
    L = ctypes.CDLL(REF_SO)
    L.ref_sign_load.argtypes = [ctypes.c_char_p]
    L.ref_sign_many.restype = ctypes.c_long
    return L


def buf(b):
    return (ctypes.c_uint8 * len(b)).from_buffer_copy(bytes(b))


class Ref:
    def __init__(self, L, name):
        self.L = L
        self.slot = L.ref_sign_load(name.encode())
        assert self.slot >= 0, name

    def sign(self, le, h, hash_size, d, rnd):
        """(status, r, s): bytes in, bytes out; zeros unless the status is 0."""
        r, s = (ctypes.c_uint8 * 32)(), (ctypes.c_uint8 * 32)()
        st = self.L.ref_sign(self.slot, int(le), buf(h), ctypes.c_size_t(hash_size), buf(d), buf(rnd), r, s)
        return (st, bytes(r), bytes(s)) if st == 0 else (st, bytes(32), bytes(32))

    def key_gen(self, le, rnd):
        d, qx, qy = ((ctypes.c_uint8 * 32)() for _ in range(3))
        sz = ctypes.c_size_t(0)
        st = self.L.ref_key_gen(self.slot, int(le), buf(rnd), d, qx, qy, ctypes.byref(sz))
        if st != 0:
            return st, bytes(32), bytes(32), bytes(32)
        assert sz.value == 32, sz.value
        return st, bytes(d), bytes(qx), bytes(qy)

    def pub_key(self, le, d):
        qx, qy = (ctypes.c_uint8 * 32)(), (ctypes.c_uint8 * 32)()
        sz = ctypes.c_size_t(0)
        st = self.L.ref_pub_key(self.slot, int(le), buf(d), qx, qy, ctypes.byref(sz))
        if st != 0:
            return st, bytes(32), bytes(32)
        assert sz.value == 32, sz.value
        return st, bytes(qx), bytes(qy)

    def verify(self, le, h, hash_size, r, s, qx, qy):
        return self.L.ref_verify(self.slot, int(le), buf(h), ctypes.c_size_t(hash_size), buf(r), buf(s), buf(qx),
                                 buf(qy))


def group_of(ref, c, le, rng):
    n, p = c["n"], c["p"]
    rnd = lambda k=32: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    tb = lambda v: M.to_bytes(v, le)  # noqa: E731
    G = M.base(c)
    sign, key_gen, pub_key = [], [], []

    def srec(name, h, d, k):
        """h, d, k: bytes as passed (h holds hash_size bytes)."""
        st, r, s = ref.sign(le, h, len(h), d, k)
        sign.append({"name": name, "hash": h.hex(), "hash_size": len(h), "d": d.hex(), "rnd": k.hex(), "status": st,
                     "r": r.hex(), "s": s.hex()})
        dv = M.num(d, le)
        if st == 0 and dv != 0:  # a signature the reference itself accepts under the recovered key
            pst, qx, qy = ref.pub_key(le, d)
            assert pst == 0 and ref.verify(le, h, len(h), r, s, qx, qy) == 0, (c["name"], name)
        # the model chose inputs only: note where it disagrees with the reference
        if dv < n:
            m = M.sign(c, h, len(h), dv, M.num(k, le), le)
            if (m is None) != (st != 0) or (m is not None and (tb(m[0]), tb(m[1])) != (r, s)):
                print("NOTE model != reference: %s %s %s" % (c["name"], "le" if le else "be", name))
        return st

    d0 = tb(M.num(rnd(), False) % (n - 1) + 1)
    for i in range(4):
        assert srec("valid_%d" % i, rnd(), tb(M.num(rnd(), False) % (n - 1) + 1), rnd()) == 0
    for hs in (1, 20, 31, 33, 48, 64):
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
    if c["name"] == "id-GostR3410-2001-ParamSet-cc":  # p is well above n here
        for _ in range(64):
            kv = M.num(rnd(), False)
            if M.mult(c, M.mod_reduce(kv, n), G)[0] >= n:
                assert srec("valid_Rx_ge_n", rnd(), d0, tb(kv)) == 0
                break
        else:
            raise SystemExit("no nonce with R.x >= n found")
    assert {0, -1, M.EINVAL} <= {k["status"] for k in sign}, c["name"]

    for nm, v in (("rnd_zero", 0), ("rnd_one", 1), ("rnd_n_minus_1", n - 1), ("rnd_eq_n", n), ("rnd_ff", FF),
                  ("random_0", None), ("random_1", None), ("random_2", None)):
        k = rnd() if v is None else tb(v)
        st, d, qx, qy = ref.key_gen(le, k)
        key_gen.append({"name": nm, "rnd": k.hex(), "status": st, "d": d.hex(), "Qx": qx.hex(), "Qy": qy.hex()})
    for nm, v in (("d_zero", 0), ("d_one", 1), ("d_n_minus_1", n - 1), ("d_eq_n", n), ("d_ff", FF),
                  ("random_0", None), ("random_1", None), ("random_2", None)):
        d = tb(M.num(rnd(), False) % (n - 1) + 1) if v is None else tb(v)
        st, qx, qy = ref.pub_key(le, d)
        pub_key.append({"name": nm, "d": d.hex(), "status": st, "Qx": qx.hex(), "Qy": qy.hex()})
        if st == 0:
            assert (M.num(qx, le), M.num(qy, le)) == M.public_key(c, M.num(d, le)), (c["name"], nm)
    return {"curve": c["name"], "le": le, "sign": sign, "key_gen": key_gen, "pub_key": pub_key}


def ref_rate(ref, grp):
    ok = [k for k in grp["sign"] if k["status"] == 0 and k["hash_size"] == 32][:8]
    recs = b"".join(bytes.fromhex(k["hash"] + k["d"] + k["rnd"]) for k in ok) * 16
    b = buf(recs)
    t = time.perf_counter()
    assert ref.L.ref_sign_many(ref.slot, int(grp["le"]), b, ctypes.c_size_t(len(recs) // 96)) == 0
    return (len(recs) // 96) / (time.perf_counter() - t)


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    L = build_ref(ref_root)
    vfx = M.load_fixture()
    curves = M.load_curves(vfx)
    rng = np.random.default_rng(0x5167EC)
    groups, rates = [], {}
    for g in vfx["cases"]:  # the same (curve, form) groups, in the same order
        ref = Ref(L, g["curve"])
        grp = group_of(ref, curves[g["curve"]], bool(g["le"]), rng)
        groups.append(grp)
        if not grp["le"]:
            rates[g["curve"]] = round(ref_rate(ref, grp), 1)
    json.dump({"source": "include/crypto/dsa/ecdsa.h compiled from the reference (oracle/_ref), configuration of "
                         "tests/golden/ref_ecdsa_shim.c",
               "ref_rate": {"what": "ecdsa_sign_be calls per second, one core of the generating machine, gcc -O2",
                            "per_curve": rates},
               "groups": groups}, open(OUT, "w"), indent=0)
    print("ecdsa_sign.json: %d groups, %d sign, %d key_gen, %d pub_key records, %d bytes" % (
        len(groups), sum(len(g["sign"]) for g in groups), sum(len(g["key_gen"]) for g in groups),
        sum(len(g["pub_key"]) for g in groups), os.path.getsize(OUT)))
    for g in groups:
        print("%-45s %s" % (g["curve"], "le" if g["le"] else "be"),
              {k["name"]: k["status"] for k in g["sign"] if k["status"]},
              {k["name"]: k["status"] for k in g["key_gen"] + g["pub_key"] if k["status"]})
    print("reference signs/s:", rates)


if __name__ == "__main__":
    main()
