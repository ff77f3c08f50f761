#!/usr/bin/env python3
"""Generate tests/golden/ecdsa_wide.json (run ONLY where the reference exists).

Pure data fixtures for include/crypto/dsa/ecdsa.h on its 384- and 512-bit
curves.  Every status, every key and every valid signature is produced by the
reference itself, compiled from its sources through
tests/golden/ref_ecdsa_wide_shim.c into oracle/_ref/libref_ecdsa_wide.so
(git-ignored).  tests/ecdsa_wide_model.py is used only to choose inputs (the
hash that makes R = O, the search for R.x >= n); what those inputs give is
again asked of the reference, and where the model disagrees a NOTE is printed.

curves
    name, algo, h, bytes (B = 48 or 64) and p, a, b, Gx, Gy, n as the
    reference's loaded curve exports them.
cases
    Per (curve, form) the records {name, hash, hash_size, r, s, Qx, Qy,
    status}: all byte strings exactly as passed to ecdsa_verify_be (le false)
    or ecdsa_verify_le (le true) with sign_size = pub_key_size = B.  On disk a
    group stores every byte string once, in `nums`, and a record is a row
    over those fields with indices into `nums`;
    tests/ecdsa_wide_model.load_fixture() gives the records back as dicts.
messages
    Per natural pair (digest, curve, form) a handful of short messages:
    {msg, hash, r, s, Qx, Qy, status}.  `hash` is the oracle's digest of the
    message that was signed; every second stored message then has one byte
    altered, `hash` is the digest of the stored message and `status` what the
    reference returns for it.
notes
    Per curve whether a valid signature with R.x >= n was found.
ref_rate
    ecdsa_verify calls per second on one core of the generating machine.

Usage:  python3 tests/golden/make_golden_ecdsa_wide.py [reference root]
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

REF_SO = os.path.join(REPO, "oracle", "_ref", "libref_ecdsa_wide.so")

CURVE_NAMES = ["secp384r1", "brainpoolP384r1", "brainpoolP512r1", "id-tc26-gost-3410-12-512-paramSetA",
               "id-tc26-gost-3410-12-512-paramSetB", "id-tc26-gost-3410-2012-512-paramSetTest"]
# The second form of these two curves (every curve has its natural one:
# be for ECDSA, le for GOST).
EXTRA_FORM = {"secp384r1": True, "id-tc26-gost-3410-12-512-paramSetA": False}
# digest (include/lcb_hash_gpu.h id), curve, le
PAIRS = [("sha384", 5, "secp384r1", False), ("sha512", 6, "brainpoolP512r1", False),
         ("gost512", 8, "id-tc26-gost-3410-12-512-paramSetA", True)]


def build_ref(ref_root):
    hdr = os.path.join(ref_root, "include", "crypto", "dsa", "ecdsa.h")
    if not os.path.exists(hdr):
        raise SystemExit("%s is missing: this generator runs only where the reference exists" % hdr)
    os.makedirs(os.path.dirname(REF_SO), exist_ok=True)
    subprocess.check_call(["gcc", "-O2", "-w", "-fPIC", "-shared", "-I" + os.path.join(ref_root, "include"),
                           "-o", REF_SO, os.path.join(HERE, "ref_ecdsa_wide_shim.c")])
    return load_ref()


def load_ref():
    L = ctypes.CDLL(REF_SO)
    L.ref_ecdsa_wide_load.argtypes = [ctypes.c_char_p]
    L.ref_ecdsa_wide_verify_many.restype = ctypes.c_long
    return L


def buf(b):
    return (ctypes.c_uint8 * len(b)).from_buffer_copy(bytes(b))


class Ref:
    def __init__(self, L, name):
        self.L = L
        self.slot = L.ref_ecdsa_wide_load(name.encode())
        assert self.slot >= 0, name
        self.B = 0

    def params(self):
        out = (ctypes.c_uint8 * 384)()
        algo, h, bits = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        assert self.L.ref_ecdsa_wide_params(self.slot, out, ctypes.byref(algo), ctypes.byref(h),
                                            ctypes.byref(bits)) == 0
        assert bits.value in (384, 512)
        B = self.B = bits.value // 8
        raw = bytes(out)
        return [raw[B * i:B * i + B].hex() for i in range(6)], algo.value, h.value, B

    def key_gen(self, rnd):
        """(d, Qx, Qy) as ints from B random bytes."""
        priv, qx, qy = ((ctypes.c_uint8 * self.B)() for _ in range(3))
        assert self.L.ref_ecdsa_wide_key_gen_be(self.slot, buf(rnd), priv, qx, qy) == 0
        return tuple(int.from_bytes(bytes(v), "big") for v in (priv, qx, qy))

    def sign(self, le, h, hash_size, d, k):
        """(r, s) as bytes in the form's byte order."""
        o = "little" if le else "big"
        r, s = (ctypes.c_uint8 * self.B)(), (ctypes.c_uint8 * self.B)()
        rc = self.L.ref_ecdsa_wide_sign(self.slot, int(le), buf(h), ctypes.c_size_t(hash_size),
                                        buf(d.to_bytes(self.B, o)), buf(k.to_bytes(self.B, o)), r, s)
        assert rc == 0, rc
        return bytes(r), bytes(s)

    def verify(self, le, h, hash_size, r, s, qx, qy):
        return self.L.ref_ecdsa_wide_verify(self.slot, int(le), buf(h), ctypes.c_size_t(hash_size), buf(r), buf(s),
                                            buf(qx), buf(qy))


def flip(b, bit):
    b = bytearray(b)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


def cases_of(ref, c, le, rng, notes):
    n, p, B = c["n"], c["p"], c["bytes"]
    rnd = lambda k=B: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    tb = lambda v: M.to_bytes(c, v, le)  # noqa: E731
    nonce = lambda: M.num(rnd(), False)  # noqa: E731
    out = []

    def rec(name, h, hash_size, r, s, qx, qy):
        st = ref.verify(le, h, hash_size, r, s, qx, qy)
        out.append({"name": name, "hash": bytes(h).hex(), "hash_size": hash_size, "r": r.hex(), "s": s.hex(),
                    "Qx": qx.hex(), "Qy": qy.hex(), "le": le, "status": st})
        return st

    d, Qx, Qy = ref.key_gen(rnd())
    qx, qy = tb(Qx), tb(Qy)
    h = rnd()
    r, s = ref.sign(le, h, B, d, nonce())
    assert rec("valid", h, B, r, s, qx, qy) == 0
    d2, Q2x, Q2y = ref.key_gen(rnd())
    h2 = rnd()
    r2, s2 = ref.sign(le, h2, B, d2, nonce())
    assert rec("valid_key2", h2, B, r2, s2, tb(Q2x), tb(Q2y)) == 0
    rec("valid_wrong_key", h, B, r, s, tb(Q2x), tb(Q2y))
    assert rec("flip_hash", flip(h, 8 * B - 179), B, r, s, qx, qy) == -2
    rec("flip_r", h, B, flip(r, 8 * B - 156), s, qx, qy)
    rec("flip_s", h, B, r, flip(s, 8 * B - 125), qx, qy)
    assert rec("flip_Qy", h, B, r, s, qx, flip(qy, 9)) == -1
    for nm, rv, sv in (("r_zero", 0, None), ("s_zero", None, 0), ("r_eq_n", n, None), ("s_eq_n", None, n),
                       ("r_n_minus_1", n - 1, None), ("s_n_minus_1", None, n - 1), ("r_s_zero", 0, 0)):
        rec(nm, h, B, r if rv is None else tb(rv), s if sv is None else tb(sv), qx, qy)
    rec("offcurve_and_r_eq_n", h, B, tb(n), s, qx, flip(qy, 8 * B - 56))
    rec("Qx_eq_p", h, B, r, s, tb(p), qy)
    rec("Qy_eq_p", h, B, r, s, qx, tb(p))
    for nm, hv in (("hash_zero", bytes(B)), ("hash_eq_n", tb(n)), ("hash_ff", b"\xff" * B),
                   ("hash_n_plus_1", tb(n + 1))):
        rr, ss = ref.sign(le, hv, B, d, nonce())
        assert rec(nm, hv, B, rr, ss, qx, qy) == 0
    # the zero-hash signature with the hash n: differs between "mod n" and the
    # reference's reduction
    rr, ss = ref.sign(le, bytes(B), B, d, nonce())
    rec("hash_eq_n_sig_of_zero", tb(n), B, rr, ss, qx, qy)
    # every hash size the import treats differently, on both sides of B
    for hs in sorted({1, 20, B - 1, B, B + 1, 64, 65, 128}):
        hv = rnd(128)
        rr, ss = ref.sign(le, hv, hs, d, nonce())
        assert rec("hash_size_%d" % hs, hv[:hs], hs, rr, ss, qx, qy) == 0
        if hs in (20, B - 1):  # bytes past hash_size are not read; they count once hash_size says so
            assert rec("hash_size_%d_tail_changed" % hs, hv[:hs] + rnd(B - hs), hs, rr, ss, qx, qy) == 0
            rec("hash_size_%d_as_B" % hs, hv[:B], B, rr, ss, qx, qy)
        if hs in (B + 1, 128):  # bytes past B are read by nobody: the same signature verifies as B
            assert rec("hash_size_%d_as_B" % hs, hv[:B], B, rr, ss, qx, qy) == 0
            assert rec("hash_size_%d_past_B_changed" % hs, hv[:B] + rnd(hs - B), hs, rr, ss, qx, qy) == 0
    G = (c["Gx"], c["Gy"])
    for nm, dd, Q in (("Q_eq_G", 1, G), ("Q_eq_minus_G", n - 1, (G[0], p - G[1]))):
        hv = rnd()
        rr, ss = ref.sign(le, hv, B, dd, nonce())
        assert rec(nm, hv, B, rr, ss, tb(Q[0]), tb(Q[1])) == 0
        rec(nm + "_flip_hash", flip(hv, 3), B, rr, ss, tb(Q[0]), tb(Q[1]))
    # R = O: ECDSA u1 G + u2 Q = s^-1 (e + r d) G, GOST e^-1 (s - r d) G.
    rv = nonce() % (n - 1) + 1
    if c["algo"] == M.ALGO_ECDSA:
        sv = nonce() % (n - 1) + 1
        ev = (-rv * d) % n
    else:
        ev = nonce() % (n - 1) + 1
        sv = rv * d % n
    assert rec("R_at_infinity", tb(ev), B, tb(rv), tb(sv), qx, qy) == -1
    # R = O with Q = G: u1 + u2 = 0, the sum G + Q of Shamir's trick is a doubling.
    if c["algo"] == M.ALGO_ECDSA:
        ev = (-rv) % n
    else:
        sv = rv
    assert rec("R_at_infinity_Q_eq_G", tb(ev), B, tb(rv), tb(sv), tb(G[0]), tb(G[1])) == -1
    # A valid signature whose R.x is >= n.  |p - n| is below 2^(4 B + 1) on these
    # curves (Hasse), so the search is expected to find none; the outcome is recorded.
    found = False
    if p > n:
        for _ in range(64):
            k = nonce()
            R = M.mult(c, M.mod_reduce(k, n), G)
            if R is not None and R[0] >= n:
                hv = rnd()
                rr, ss = ref.sign(le, hv, B, d, k)
                assert rec("valid_Rx_ge_n", hv, B, rr, ss, qx, qy) == 0
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


def messages_of(ref, c, alg_id, le, rng, oracle):
    """Six short messages signed over the oracle's digest; the odd ones are
    then stored with one byte altered."""
    B = c["bytes"]
    rnd = lambda k=B: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    out = []
    keys = [ref.key_gen(rnd()) for _ in range(2)]

    def digest(m):
        a = np.frombuffer(m, np.uint8) if m else np.zeros(0, np.uint8)
        return oracle.batch(alg_id, a, np.array([0], np.uint64), np.array([len(m)], np.uint32))[0].tobytes()

    for i, ln in enumerate((0, 1, 47, 64, 129, 200)):
        msg = rnd(ln) if ln else b""
        d, Qx, Qy = keys[i % 2]
        hv = digest(msg)
        r, s = ref.sign(le, hv, len(hv), d, M.num(rnd(), False))
        if i % 2:
            msg = flip(msg, (5 * i) % (8 * ln))
            hv = digest(msg)
        qx, qy = M.to_bytes(c, Qx, le), M.to_bytes(c, Qy, le)
        st = ref.verify(le, hv, len(hv), r, s, qx, qy)
        assert st == (-2 if i % 2 else 0), st
        out.append({"msg": msg.hex(), "hash": hv.hex(), "r": r.hex(), "s": s.hex(), "Qx": qx.hex(), "Qy": qy.hex(),
                    "le": le, "status": st})
    return out


def ref_rate(ref, cases, le, B):
    ok = [k for k in cases if k["status"] == 0 and k["hash_size"] == B and len(k["hash"]) == 2 * B][:8]
    recs = b"".join(bytes.fromhex(k["hash"] + k["r"] + k["s"] + k["Qx"] + k["Qy"]) for k in ok) * 4
    b = buf(recs)
    t = time.perf_counter()
    assert ref.L.ref_ecdsa_wide_verify_many(ref.slot, int(le), b, ctypes.c_size_t(len(recs) // (5 * B))) == 0
    return (len(recs) // (5 * B)) / (time.perf_counter() - t)


def pack_group(g, fields):
    """The group with every byte string stored once, in `nums`, and its records
    as rows over `fields` that hold indices into `nums`
    (tests/ecdsa_wide_model.py expands them again)."""
    nums, where, rows = [], {}, []
    for k in g["records"]:
        row = []
        for f in fields:
            v = k[f]
            if f in M.HEX_FIELDS:
                if v not in where:
                    where[v] = len(nums)
                    nums.append(v)
                v = where[v]
            row.append(v)
        rows.append(row)
    return dict({f: v for f, v in g.items() if f != "records"}, nums=nums, records=rows)


def write_fixture(fx, path):
    """JSON with one line per curve, per stored byte string and per record."""
    d = json.dumps
    out = ["{"] + ["%s: %s," % (d(k), d(fx[k])) for k in ("source", "ref_rate", "notes")]
    out += ['"curves": [', ",\n".join(d(c) for c in fx["curves"]), "],"]
    for key in ("cases", "messages"):
        groups = []
        for g in fx[key]:
            head = d({f: v for f, v in g.items() if f not in ("nums", "records")})[:-1]
            groups.append('%s, "nums": [\n%s\n], "records": [\n%s\n]}' % (
                head, ",\n".join(d(v) for v in g["nums"]), ",\n".join(d(r) for r in g["records"])))
        out += ['"%s": [' % key, ",\n".join(groups), "]," if key == "cases" else "]"]
    out.append("}")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def main():
    from oracle import pyoracle
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    L = build_ref(ref_root)
    pyoracle.build()
    oracle = pyoracle.Oracle()
    rng = np.random.default_rng(0xEC05A512)
    curves, cases, messages, notes, rates = [], [], [], {}, {}
    by_name = {}
    for name in CURVE_NAMES:
        ref = Ref(L, name)
        nums, algo, h, B = ref.params()
        cj = dict(zip(M.NUMS, nums), name=name, algo=algo, h=h, bytes=B)
        curves.append(cj)
        c = M.curve_from_json(cj)
        by_name[name] = (ref, c)
        natural = algo == M.ALGO_GOST
        forms = [natural] + ([EXTRA_FORM[name]] if name in EXTRA_FORM else [])
        for le in forms:
            cs = cases_of(ref, c, le, rng, notes)
            cases.append({"curve": name, "le": le, "records": cs})
            if le == natural:
                rates[name] = round(ref_rate(ref, cs, le, B), 1)
    for alg, alg_id, name, le in PAIRS:
        ref, c = by_name[name]
        messages.append({"alg": alg, "alg_id": alg_id, "curve": name, "le": le,
                         "records": messages_of(ref, c, alg_id, le, rng, oracle)})
    write_fixture({"source": "include/crypto/dsa/ecdsa.h compiled from the reference (oracle/_ref), configuration of "
                             "tests/ecdsa/main.c with the public key check on",
                   "ref_rate": {"what": "ecdsa_verify calls per second in the curve's natural form, one core of the "
                                        "generating machine, gcc -O2",
                                "per_curve": rates},
                   "notes": notes, "curves": curves,
                   "cases": [pack_group(g, M.CASE_FIELDS) for g in cases],
                   "messages": [pack_group(g, M.MESSAGE_FIELDS) for g in messages]},
                  os.path.join(HERE, "ecdsa_wide.json"))
    assert M.load_fixture()["cases"] == cases and M.load_fixture()["messages"] == messages
    print("ecdsa_wide.json: %d curves, %d records, %d bytes" % (
        len(curves), sum(len(c["records"]) for c in cases), os.path.getsize(os.path.join(HERE, "ecdsa_wide.json"))))
    print("Rx >= n:", notes)
    print("reference verifies/s:", rates)


if __name__ == "__main__":
    main()
