#!/usr/bin/env python3
"""Generate tests/golden/ecdsa.json (run ONLY where the reference exists).

Pure data fixtures for include/crypto/dsa/ecdsa.h.  Every status, every key
and every valid signature is produced by the reference itself, compiled from
its sources through tests/golden/ref_ecdsa_shim.c into
oracle/_ref/libref_ecdsa.so (git-ignored).  tests/ecdsa_model.py is used only
to choose inputs (a nonce whose R.x is >= n, the hash that makes R = O); what
those inputs give is again asked of the reference.

curves
    name, algo, h and p, a, b, Gx, Gy, n as the reference's loaded curve
    exports them.
cases
    Per (curve, form) the records {name, hash, hash_size, r, s, Qx, Qy, le,
    status}: all byte strings exactly as passed to ecdsa_verify_be (le false)
    or ecdsa_verify_le (le true) with sign_size = pub_key_size = 32.
notes
    Per curve whether a valid signature with R.x >= n was found.
ref_rate
    ecdsa_verify_be calls per second on one core of the generating machine.

Usage:  python3 tests/golden/make_golden_ecdsa.py [reference root]
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

REF_SO = os.path.join(REPO, "oracle", "_ref", "libref_ecdsa.so")

CURVE_NAMES = ["secp256k1", "secp256r1", "brainpoolP256r1", "id-GostR3410-2001-ParamSet-cc",
               "id-gostR3410-2001-Test_ParamSet", "id-gostR3410-2001-CryptoPro-A-ParamSet",
               "id-gostR3410-2001-CryptoPro-B-ParamSet", "id-gostR3410-2001-CryptoPro-C-ParamSet",
               "id-gostR3410-2001-CryptoPro-XchA-ParamSet", "id-gostR3410-2001-CryptoPro-XchB-ParamSet"]
# The second form of these two curves (every curve has its natural one:
# be for ECDSA, le for GOST).
EXTRA_FORM = {"secp256r1": True, "id-gostR3410-2001-CryptoPro-A-ParamSet": False}


def build_ref(ref_root):
    hdr = os.path.join(ref_root, "include", "crypto", "dsa", "ecdsa.h")
    if not os.path.exists(hdr):
        raise SystemExit("%s is missing: this generator runs only where the reference exists" % hdr)
    os.makedirs(os.path.dirname(REF_SO), exist_ok=True)
    subprocess.check_call(["gcc", "-O2", "-w", "-fPIC", "-shared", "-I" + os.path.join(ref_root, "include"),
                           "-o", REF_SO, os.path.join(HERE, "ref_ecdsa_shim.c")])
    return load_ref()


def load_ref():
    L = ctypes.CDLL(REF_SO)
    L.ref_ecdsa_load.argtypes = [ctypes.c_char_p]
    L.ref_ecdsa_verify_many.restype = ctypes.c_long
    return L


def buf(b):
    return (ctypes.c_uint8 * len(b)).from_buffer_copy(bytes(b))


class Ref:
    def __init__(self, L, name):
        self.L = L
        self.slot = L.ref_ecdsa_load(name.encode())
        assert self.slot >= 0, name

    def params(self):
        out = (ctypes.c_uint8 * 192)()
        algo, h, bits = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        assert self.L.ref_ecdsa_params(self.slot, out, ctypes.byref(algo), ctypes.byref(h), ctypes.byref(bits)) == 0
        assert bits.value == 256
        raw = bytes(out)
        return [raw[32 * i:32 * i + 32].hex() for i in range(6)], algo.value, h.value

    def key_gen(self, rnd):
        """(d, Qx, Qy) as ints from 32 random bytes."""
        priv, qx, qy = ((ctypes.c_uint8 * 32)() for _ in range(3))
        assert self.L.ref_ecdsa_key_gen_be(self.slot, buf(rnd), priv, qx, qy) == 0
        return tuple(int.from_bytes(bytes(v), "big") for v in (priv, qx, qy))

    def sign(self, le, h, hash_size, d, k):
        """(r, s) as bytes in the form's byte order."""
        r, s = (ctypes.c_uint8 * 32)(), (ctypes.c_uint8 * 32)()
        rc = self.L.ref_ecdsa_sign(self.slot, int(le), buf(h), ctypes.c_size_t(hash_size), buf(M.to_bytes(d, le)),
                                   buf(M.to_bytes(k, le)), r, s)
        assert rc == 0, rc
        return bytes(r), bytes(s)

    def verify(self, le, h, hash_size, r, s, qx, qy):
        return self.L.ref_ecdsa_verify(self.slot, int(le), buf(h), ctypes.c_size_t(hash_size), buf(r), buf(s),
                                       buf(qx), buf(qy))


def flip(b, bit):
    b = bytearray(b)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


def cases_of(ref, c, le, rng, notes):
    n, p = c["n"], c["p"]
    rnd = lambda k=32: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    tb = lambda v: M.to_bytes(v, le)  # noqa: E731
    out = []

    def rec(name, h, hash_size, r, s, qx, qy):
        st = ref.verify(le, h, hash_size, r, s, qx, qy)
        out.append({"name": name, "hash": bytes(h).hex(), "hash_size": hash_size, "r": r.hex(), "s": s.hex(),
                    "Qx": qx.hex(), "Qy": qy.hex(), "le": le, "status": st})
        return st

    d, Qx, Qy = ref.key_gen(rnd())
    qx, qy = tb(Qx), tb(Qy)
    h = rnd()
    r, s = ref.sign(le, h, 32, d, M.num(rnd(), False))
    assert rec("valid", h, 32, r, s, qx, qy) == 0
    d2, Q2x, Q2y = ref.key_gen(rnd())
    h2 = rnd()
    r2, s2 = ref.sign(le, h2, 32, d2, M.num(rnd(), False))
    assert rec("valid_key2", h2, 32, r2, s2, tb(Q2x), tb(Q2y)) == 0
    rec("valid_wrong_key", h, 32, r, s, tb(Q2x), tb(Q2y))
    rec("flip_hash", flip(h, 77), 32, r, s, qx, qy)
    rec("flip_r", h, 32, flip(r, 100), s, qx, qy)
    rec("flip_s", h, 32, r, flip(s, 131), qx, qy)
    assert rec("flip_Qy", h, 32, r, s, qx, flip(qy, 9)) == -1
    for nm, rv, sv in (("r_zero", 0, None), ("s_zero", None, 0), ("r_eq_n", n, None), ("s_eq_n", None, n),
                       ("r_n_minus_1", n - 1, None), ("s_n_minus_1", None, n - 1), ("r_s_zero", 0, 0)):
        rec(nm, h, 32, r if rv is None else tb(rv), s if sv is None else tb(sv), qx, qy)
    rec("offcurve_and_r_eq_n", h, 32, tb(n), s, qx, flip(qy, 200))
    rec("Qx_eq_p", h, 32, r, s, tb(p), qy)
    rec("Qy_eq_p", h, 32, r, s, qx, tb(p))
    for nm, hv in (("hash_zero", bytes(32)), ("hash_eq_n", tb(n)), ("hash_ff", b"\xff" * 32),
                   ("hash_n_plus_1", tb(n + 1) if n + 1 < 1 << 256 else tb(n))):
        rr, ss = ref.sign(le, hv, 32, d, M.num(rnd(), False))
        assert rec(nm, hv, 32, rr, ss, qx, qy) == 0
    # a signature over another representative of the same reduced hash must
    # not verify against the all-zero hash etc.: the zero-hash signature with
    # the hash n (differs between "mod n" and the reference's reduction)
    rr, ss = ref.sign(le, bytes(32), 32, d, M.num(rnd(), False))
    rec("hash_eq_n_sig_of_zero", tb(n), 32, rr, ss, qx, qy)
    for nm, hs in (("hash_size_20", 20), ("hash_size_64", 64), ("hash_size_1", 1), ("hash_size_33", 33)):
        hv = rnd(64)
        rr, ss = ref.sign(le, hv, hs, d, M.num(rnd(), False))
        assert rec(nm, hv, hs, rr, ss, qx, qy) == 0
        if hs == 20:  # bytes past hash_size are not read
            assert rec("hash_size_20_tail_changed", hv[:20] + rnd(44), 20, rr, ss, qx, qy) == 0
            rec("hash_size_20_as_32", hv, 32, rr, ss, qx, qy)
    G = (c["Gx"], c["Gy"])
    for nm, dd, Q in (("Q_eq_G", 1, G), ("Q_eq_minus_G", n - 1, (G[0], p - G[1]))):
        hv = rnd()
        rr, ss = ref.sign(le, hv, 32, dd, M.num(rnd(), False))
        assert rec(nm, hv, 32, rr, ss, tb(Q[0]), tb(Q[1])) == 0
        rec(nm + "_flip_hash", flip(hv, 3), 32, rr, ss, tb(Q[0]), tb(Q[1]))
    # R = O: ECDSA u1 G + u2 Q = s^-1 (e + r d) G, GOST e^-1 (s - r d) G.
    rv = M.num(rnd(), False) % (n - 1) + 1
    if c["algo"] == M.ALGO_ECDSA:
        sv = M.num(rnd(), False) % (n - 1) + 1
        ev = (-rv * d) % n
    else:
        ev = M.num(rnd(), False) % (n - 1) + 1
        sv = rv * d % n
    assert rec("R_at_infinity", tb(ev), 32, tb(rv), tb(sv), qx, qy) == -1
    # R = O with Q = G: u1 + u2 = 0, the sum G + Q of Shamir's trick is a doubling.
    if c["algo"] == M.ALGO_ECDSA:
        ev = (-rv) % n
    else:
        sv = rv
    assert rec("R_at_infinity_Q_eq_G", tb(ev), 32, tb(rv), tb(sv), tb(G[0]), tb(G[1])) == -1
    # A valid signature whose R.x is >= n (the reduction of R.x mod n is real work).
    found = False
    if p > n:
        for _ in range(64):
            k = M.num(rnd(), False)
            R = M.mult(c, M.mod_reduce(k, n), G)
            if R is not None and R[0] >= n:
                hv = rnd()
                rr, ss = ref.sign(le, hv, 32, d, k)
                assert rec("valid_Rx_ge_n", hv, 32, rr, ss, qx, qy) == 0
                found = True
                break
    notes.setdefault(c["name"], {})["Rx_ge_n_found_le" if le else "Rx_ge_n_found_be"] = found
    # the model chose inputs only: it must agree with what the reference said
    for k in out:
        got = M.verify(c, bytes.fromhex(k["hash"]), k["hash_size"], bytes.fromhex(k["r"]), bytes.fromhex(k["s"]),
                       bytes.fromhex(k["Qx"]), bytes.fromhex(k["Qy"]), le)
        if got != k["status"]:
            print("NOTE model %d != reference %d: %s %s" % (got, k["status"], c["name"], k["name"]))
    return out


def ref_rate(ref, cases, le):
    ok = [k for k in cases if k["status"] == 0 and k["hash_size"] == 32][:8]
    recs = b"".join(bytes.fromhex(k["hash"] + k["r"] + k["s"] + k["Qx"] + k["Qy"]) for k in ok) * 8
    b = buf(recs)
    t = time.perf_counter()
    assert ref.L.ref_ecdsa_verify_many(ref.slot, int(le), b, ctypes.c_size_t(len(recs) // 160)) == 0
    return (len(recs) // 160) / (time.perf_counter() - t)


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    L = build_ref(ref_root)
    rng = np.random.default_rng(0xEC05A)
    curves, cases, notes, rates = [], [], {}, {}
    for name in CURVE_NAMES:
        ref = Ref(L, name)
        nums, algo, h = ref.params()
        cj = dict(zip(M.NUMS, nums), name=name, algo=algo, h=h)
        curves.append(cj)
        c = M.curve_from_json(cj)
        natural = algo == M.ALGO_GOST
        forms = [natural] + ([EXTRA_FORM[name]] if name in EXTRA_FORM else [])
        for le in forms:
            cs = cases_of(ref, c, le, rng, notes)
            cases.append({"curve": name, "le": le, "records": cs})
            if not le:
                rates[name] = round(ref_rate(ref, cs, le), 1)
    json.dump({"source": "include/crypto/dsa/ecdsa.h compiled from the reference (oracle/_ref), configuration of "
                         "tests/ecdsa/main.c with the public key check on",
               "ref_rate": {"what": "ecdsa_verify_be calls per second, one core of the generating machine, gcc -O2",
                            "per_curve": rates},
               "curves": curves, "notes": notes, "cases": cases},
              open(os.path.join(HERE, "ecdsa.json"), "w"), indent=0)
    print("ecdsa.json: %d curves, %d records" % (len(curves), sum(len(c["records"]) for c in cases)))
    print("Rx >= n:", notes)
    print("reference verifies/s:", rates)


if __name__ == "__main__":
    main()
