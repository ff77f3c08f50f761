#!/usr/bin/env python3
"""Generate tests/golden/ecdsa_dh.json (run ONLY where the reference exists).

Pure data fixtures for the key agreement of include/crypto/dsa/ecdsa.h.  Every
status and every output byte is produced by the reference itself, compiled
from its sources through tests/golden/ref_ecdsa_dh_shim.c into
oracle/_ref/libref_ecdsa_dh.so (git-ignored).  tests/ecdsa_model.py is used
to choose inputs (multiples of G as public keys) and, for every record the
reference accepted, to assert that the bytes are the x coordinate of the plain
d Q; a disagreement is printed, the reference's record is kept.  The curves'
numbers are those of tests/golden/ecdsa.json.

groups
    Per (curve, form), the 12 groups of ecdsa.json:
    records  {name, Qx, Qy, d, use_cofactor, status, shared}: the bytes passed
             to ecdsa_dh_be (le false) or ecdsa_dh_le (le true) with
             pub_key_size = priv_key_size = 32, and what it returned and wrote
    The output of a call that did not return 0 is recorded as zeros (the
    reference writes nothing there).
ref_rate
    ecdsa_dh_be calls per second on one core of the generating machine.

Usage:  python3 tests/golden/make_golden_ecdsa_dh.py [reference root]
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

REF_SO = os.path.join(REPO, "oracle", "_ref", "libref_ecdsa_dh.so")
OUT = os.path.join(HERE, "ecdsa_dh.json")
FF = (1 << 256) - 1
PATTERNS = (("d_55", 0x55), ("d_aa", 0xAA), ("d_33", 0x33), ("d_0f", 0x0F))


def build_ref(ref_root):
    hdr = os.path.join(ref_root, "include", "crypto", "dsa", "ecdsa.h")
    if not os.path.exists(hdr):
        raise SystemExit("%s is missing: this generator runs only where the reference exists" % hdr)
    os.makedirs(os.path.dirname(REF_SO), exist_ok=True)
    subprocess.check_call(["gcc", "-O2", "-w", "-fPIC", "-shared", "-I" + os.path.join(ref_root, "include"),
                           "-o", REF_SO, os.path.join(HERE, "ref_ecdsa_dh_shim.c")])
    return load_ref()


def load_ref():
    L = ctypes.CDLL(REF_SO)
    L.ref_dh_load.argtypes = [ctypes.c_char_p]
    L.ref_dh_many.restype = ctypes.c_long
    return L


def buf(b):
    return (ctypes.c_uint8 * len(b)).from_buffer_copy(bytes(b))


class Ref:
    def __init__(self, L, name):
        self.L = L
        self.slot = L.ref_dh_load(name.encode())
        assert self.slot >= 0, name

    def dh(self, le, use_cofactor, qx, qy, d):
        """(status, shared): bytes in, bytes out; zeros unless the status is 0."""
        out = (ctypes.c_uint8 * 32)()
        sz = ctypes.c_size_t(0)
        st = self.L.ref_dh(self.slot, int(le), int(use_cofactor), buf(qx), buf(qy), buf(d), out, ctypes.byref(sz))
        if st != 0:
            return st, bytes(32)
        assert sz.value == 32, sz.value
        return st, bytes(out)


def group_of(ref, c, le, rng):
    n, p = c["n"], c["p"]
    rnd = lambda: M.num(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), False)  # noqa: E731
    tb = lambda v: M.to_bytes(v, le)  # noqa: E731
    G = M.base(c)
    ka, kb = rnd() % (n - 1) + 1, rnd() % (n - 1) + 1
    points = [("G", G), ("2G", M.mult(c, 2, G)), ("n_minus_1_G", M.mult(c, n - 1, G)),
              ("rand0", M.mult(c, ka, G)), ("rand1", M.mult(c, kb, G))]
    records = []

    def rec(name, q, dv, cof):
        """q: (x, y) as ints below 2^256, as passed; dv: the scalar as passed."""
        st, sh = ref.dh(le, cof, tb(q[0]), tb(q[1]), tb(dv))
        records.append({"name": name, "Qx": tb(q[0]).hex(), "Qy": tb(q[1]).hex(), "d": tb(dv).hex(),
                        "use_cofactor": cof, "status": st, "shared": sh.hex()})
        if st == 0:  # the plain d Q is the specification: say so where the reference differs
            R = M.mult(c, dv, q)
            if R is None or tb(R[0]) != sh:
                print("NOTE model != reference: %s %s %s" % (c["name"], "le" if le else "be", name))
        return st, sh

    top = 1 << 255 if (1 << 255) < n else 1 << 254
    scalars = [("d_%d" % v, v) for v in (1, 2, 3, 4, 5, 7, 8, 15, 16, 17)]
    scalars += [("d_n_minus_1", n - 1), ("d_n_minus_2", n - 2), ("d_n_minus_3", n - 3),
                ("d_n_minus_1_half", (n - 1) // 2), ("d_n_plus_1_half", (n + 1) // 2), ("d_top_bit", top),
                ("d_2_128", 1 << 128), ("d_2_128_minus_1", (1 << 128) - 1)]
    scalars += [(nm, int.from_bytes(bytes([b]) * 32, "big") % n) for nm, b in PATTERNS]
    scalars += [("d_random_%d" % i, rnd() % (n - 1) + 1) for i in range(3)]
    for i, (nm, dv) in enumerate(scalars):
        pn, q = points[i % len(points)]
        assert rec("%s_%s" % (nm, pn), q, dv, i & 1)[0] == 0, (c["name"], nm)
    # the last step of d = n - 1 meets R = -Q for every Q; once more against a random point
    assert rec("d_n_minus_1_rand1", points[4][1], n - 1, 0)[0] == 0
    # use_cofactor: the same inputs under both values
    dv = rnd() % (n - 1) + 1
    a0, a1 = rec("cofactor_0", points[3][1], dv, 0), rec("cofactor_1", points[3][1], dv, 1)
    assert a0 == a1 and a0[0] == 0, c["name"]
    # an agreement: (dA, QB) and (dB, QA)
    sa, sb = rec("agree_dA_QB", points[4][1], ka, 0), rec("agree_dB_QA", points[3][1], kb, 0)
    assert sa == sb and sa[0] == 0, c["name"]
    # refused scalars, against a good key
    Q = points[3][1]
    for nm, v in (("d_zero", 0), ("d_eq_n", n), ("d_n_plus_1", n + 1), ("d_ff", FF)):
        rec(nm, Q, v, 0)
    # refused keys, against a good scalar
    rec("Qx_eq_p", (p, Q[1]), dv, 0)
    rec("Qy_eq_p", (Q[0], p), dv, 0)
    for k in range(1, 65):  # x + p: the same residue, not below p; only where it fits in 256 bits
        S = M.mult(c, k, G)
        if S[0] + p <= FF:
            rec("Qx_plus_p", (S[0] + p, S[1]), dv, 0)
            break
    rec("Qy_plus_1", (Q[0], (Q[1] + 1) % p), dv, 0)
    rec("Q_zero_zero", (0, 0), dv, 1)
    rec("Q_off_curve_d_eq_n", (Q[0], (Q[1] + 1) % p), n, 0)
    assert {0, -1, M.EINVAL} <= {k["status"] for k in records}, c["name"]
    return {"curve": c["name"], "le": le, "records": records}


def ref_rate(ref, grp):
    ok = [k for k in grp["records"] if k["status"] == 0][:8]
    recs = b"".join(bytes.fromhex(k["Qx"] + k["Qy"] + k["d"]) for k in ok) * 16
    b = buf(recs)
    t = time.perf_counter()
    assert ref.L.ref_dh_many(ref.slot, int(grp["le"]), b, ctypes.c_size_t(len(recs) // 96)) == 0
    return (len(recs) // 96) / (time.perf_counter() - t)


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    L = build_ref(ref_root)
    vfx = M.load_fixture()
    curves = M.load_curves(vfx)
    rng = np.random.default_rng(0xD1FF1E)
    groups, rates = [], {}
    for g in vfx["cases"]:  # the same (curve, form) groups, in the same order
        ref = Ref(L, g["curve"])
        grp = group_of(ref, curves[g["curve"]], bool(g["le"]), rng)
        groups.append(grp)
        if not grp["le"]:
            rates[g["curve"]] = round(ref_rate(ref, grp), 1)
    json.dump({"source": "include/crypto/dsa/ecdsa.h compiled from the reference (oracle/_ref), configuration of "
                         "tests/golden/ref_ecdsa_shim.c",
               "ref_rate": {"what": "ecdsa_dh_be calls per second, one core of the generating machine, gcc -O2",
                            "per_curve": rates},
               "groups": groups}, open(OUT, "w"), indent=0)
    print("ecdsa_dh.json: %d groups, %d records, %d bytes" % (
        len(groups), sum(len(g["records"]) for g in groups), os.path.getsize(OUT)))
    for g in groups:
        print("%-45s %s %d" % (g["curve"], "le" if g["le"] else "be", len(g["records"])),
              {k["name"]: k["status"] for k in g["records"] if k["status"]})
    print("reference agreements/s:", rates)


if __name__ == "__main__":
    main()
