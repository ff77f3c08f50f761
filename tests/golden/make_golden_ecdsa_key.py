#!/usr/bin/env python3
"""Generate tests/golden/ecdsa_key.json (run ONLY where the reference exists).

Pure data fixtures for the public-key import and export of
include/crypto/dsa/ecdsa.h.  Every status and every output byte is produced by
the reference itself, compiled from its sources through
tests/golden/ref_ecdsa_key_shim.c into oracle/_ref/libref_ecdsa_key.so
(git-ignored).  tests/ecdsa_model.py is used to choose inputs (multiples of G)
and, for every compressed key the reference accepted, to assert with on_curve
and Python's pow that y is the root of the stated parity; a disagreement is
printed, the reference's record is kept.  The curves' numbers are those of
tests/golden/ecdsa.json.

groups
    Per (curve, form): the 12 groups of ecdsa.json and the be form of the two
    curves with p = 1 (mod 8), whose le form is among the 12.
    nums     the 32-byte numbers the group's byte strings are made of, as hex
    import   rows of `import_columns`: the bytes passed to
             ecdsa_pub_key_import_be (le false) or _le (le true), the status,
             whether the imported point is the point at infinity, and x || y
             as the reference's export of the imported point writes them
             (empty: 64 zero bytes, for every status but 0 and for infinity)
    export   rows of `export_columns`: x || y and the infinity flag of a point
             (not validated), and what ecdsa_pub_key_export_be / _le writes
             with pub_key_y = NULL
    A byte string is a list of pieces: a string is hex, an integer i is
    nums[i]; key_y null is pub_key_y = NULL.
ref_rate
    compressed ecdsa_pub_key_import_be calls per second on one core of the
    generating machine.

Usage:  python3 tests/golden/make_golden_ecdsa_key.py [reference root]
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

REF_SO = os.path.join(REPO, "oracle", "_ref", "libref_ecdsa_key.so")
OUT = os.path.join(HERE, "ecdsa_key.json")
FF = (1 << 256) - 1
EXTRA_BE = ("id-gostR3410-2001-Test_ParamSet", "id-gostR3410-2001-CryptoPro-B-ParamSet")


def build_ref(ref_root):
    hdr = os.path.join(ref_root, "include", "crypto", "dsa", "ecdsa.h")
    if not os.path.exists(hdr):
        raise SystemExit("%s is missing: this generator runs only where the reference exists" % hdr)
    os.makedirs(os.path.dirname(REF_SO), exist_ok=True)
    subprocess.check_call(["gcc", "-O2", "-w", "-fPIC", "-shared", "-I" + os.path.join(ref_root, "include"),
                           "-o", REF_SO, os.path.join(HERE, "ref_ecdsa_key_shim.c")])
    return load_ref()


def load_ref():
    L = ctypes.CDLL(REF_SO)
    L.ref_key_load.argtypes = [ctypes.c_char_p]
    L.ref_key_import.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                 ctypes.c_void_p, ctypes.c_void_p]
    L.ref_key_export.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                 ctypes.c_void_p, ctypes.c_void_p]
    L.ref_key_import_many.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                      ctypes.c_size_t]
    L.ref_key_import_many.restype = ctypes.c_long
    return L


def buf(b):
    """An exact-size copy (one spare byte where b is empty: it is never read)."""
    return (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\xee")


class Ref:
    def __init__(self, L, name):
        self.L = L
        self.slot = L.ref_key_load(name.encode())
        assert self.slot >= 0, name

    def imp(self, le, key, key_y):
        """(status, infinity, x || y): zeros unless the status is 0 and the point is finite."""
        xy = (ctypes.c_uint8 * 64)()
        inf = ctypes.c_int(0)
        k, ky = buf(key), buf(key_y) if key_y is not None else None
        st = self.L.ref_key_import(self.slot, int(le), k, ky, len(key), xy, ctypes.byref(inf))
        assert st not in (1000, 1001), (st, key.hex())
        if st != 0 or inf.value:
            return st, int(st == 0 and inf.value != 0), bytes(64)
        return st, 0, bytes(xy)

    def exp(self, le, compress, xy, inf):
        out = (ctypes.c_uint8 * 65)(*([0xEE] * 65))
        sz = ctypes.c_size_t(0)
        st = self.L.ref_key_export(self.slot, int(le), int(compress), buf(xy), int(inf), out, ctypes.byref(sz))
        assert st == 0 and bytes(out)[sz.value:] == b"\xee" * (65 - sz.value), (st, sz.value)
        return bytes(out)[:sz.value]


class Pieces:
    """Byte strings as lists of pieces over a table of 32-byte numbers."""

    def __init__(self):
        self.nums, self.at = [], {}

    def idx(self, b):
        h = bytes(b).hex()
        if h not in self.at:
            self.at[h] = len(self.nums)
            self.nums.append(h)
        return self.at[h]

    def enc(self, b):
        b = bytes(b)
        if len(b) in (32, 64):
            return [self.idx(b[i:i + 32]) for i in range(0, len(b), 32)]
        if len(b) in (33, 65):
            return [b[:1].hex()] + [self.idx(b[i:i + 32]) for i in range(1, len(b), 32)]
        return [b.hex()] if b else []


def group_of(ref, c, le, rng):
    n, p = c["n"], c["p"]
    rnd = lambda: M.num(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), False)  # noqa: E731
    tb = lambda v: M.to_bytes(v, le)  # noqa: E731
    rhs = lambda x: (x * x * x + c["a"] * x + c["b"]) % p  # noqa: E731
    G = M.base(c)
    points = [("G", G), ("2G", M.mult(c, 2, G)), ("n_minus_1_G", M.mult(c, n - 1, G))]
    points += [("rand%d" % i, M.mult(c, rnd() % (n - 1) + 1, G)) for i in range(8)]
    P = Pieces()
    imports, exports = [], []

    def imp(name, key, key_y=None):
        st, inf, xy = ref.imp(le, key, key_y)
        imports.append([name, P.enc(key), None if key_y is None else P.enc(key_y), st, inf,
                        P.enc(xy) if st == 0 and not inf else []])
        if st == 0 and not inf and len(key) == 33:  # the stated root, by the model
            x, y = M.num(xy[:32], le), M.num(xy[32:], le)
            if not (M.on_curve(c, x, y) and x < p and y < p and pow(y, 2, p) == rhs(x) and y & 1 == key[0] & 1 and
                    x == M.num(key[1:], le)):
                print("NOTE model != reference: %s %s %s" % (c["name"], "le" if le else "be", name))
        return st, inf, xy

    def exp(name, compress, xy, inf=0):
        exports.append([name, int(compress), int(inf), P.enc(xy), P.enc(ref.exp(le, compress, xy, inf))])

    for nm, (x, y) in points:
        par = y & 1
        bx, by = tb(x), tb(y)
        st, _, xy = imp(nm + "/compressed", bytes([2 | par]) + bx)
        assert st == 0 and xy == bx + by, (c["name"], nm)
        st, _, xy = imp(nm + "/compressed_other", bytes([3 - par]) + bx)
        assert st == 0 and xy == bx + tb(p - y), (c["name"], nm)
        assert imp(nm + "/packed", b"\x04" + bx + by)[0] == 0
        imp(nm + "/hybrid_right", bytes([6 | par]) + bx + by)
        imp(nm + "/hybrid_wrong", bytes([7 - par]) + bx + by)
        assert imp(nm + "/raw", bx + by)[0] == 0
        assert imp(nm + "/xy", bx, by)[0] == 0
        imp(nm + "/x_without_y", bx)
        exp(nm + "/compressed", 1, bx + by)
        exp(nm + "/packed", 0, bx + by)
    # compressed keys without a root
    found = 0
    while found < 4:
        x = rnd() % p
        if pow(rhs(x), (p - 1) // 2, p) == p - 1:
            assert imp("non_residue_%d" % found, bytes([2 + (found & 1)]) + tb(x))[0] == -1, c["name"]
            found += 1
    for nm, x in (("x_eq_p", p), ("x_p_plus_1", p + 1), ("x_ff", FF), ("x_zero", 0)):
        for pre in (2, 3):
            imp("compressed_%s_%02x" % (nm, pre), bytes([pre]) + tb(x))
    x, y = points[3][1]
    bx, by = tb(x), tb(y)
    for size, body in ((33, bx), (65, bx + by)):
        for pre in (0, 1, 2, 3, 4, 5, 6, 7, 0xFF):
            imp("prefix_%02x_size_%d" % (pre, size), bytes([pre]) + body)
    imp("size_1_byte_0", b"\x00")
    imp("size_1_byte_1", b"\x01")
    long = b"\x04" + bx + by + b"\x00"
    for size in (0, 2, 31, 34, 63, 66):
        imp("size_%d" % size, long[:size])
        imp("size_%d_with_y" % size, long[1:1 + size], by)
    for form, pre in (("packed", b"\x04"), ("raw", b"")):
        imp("%s_y_bit" % form, pre + bx + tb(y ^ 1))
        imp("%s_y_high_bit" % form, pre + bx + tb(y ^ (1 << 200)))
        imp("%s_y_eq_p" % form, pre + bx + tb(p))
        imp("%s_x_eq_p" % form, pre + tb(p) + by)
        imp("%s_zero_zero" % form, pre + bytes(64))
    imp("xy_y_bit", bx, tb(y ^ 1))
    imp("xy_y_eq_p", bx, tb(p))
    # export: nothing is validated
    off = bx + tb(y ^ 1)
    exp("off_curve/compressed", 1, off)
    exp("off_curve/packed", 0, off)
    exp("above_p/compressed", 1, tb(FF) + tb(FF))
    exp("above_p/packed", 0, tb(FF) + tb(FF - 1))
    exp("infinity/compressed", 1, bx + by, 1)
    exp("infinity/packed", 0, bytes(64), 1)
    assert {0, -1, M.EINVAL} <= {k[3] for k in imports}, c["name"]
    return {"curve": c["name"], "le": le, "nums": P.nums, "import": imports, "export": exports}


def piece_bytes(g, pieces):
    return b"".join(bytes.fromhex(q) if isinstance(q, str) else bytes.fromhex(g["nums"][q]) for q in pieces)


def ref_rate(ref, grp):
    keys = [piece_bytes(grp, k[1]) for k in grp["import"] if k[0].endswith("/compressed")] * 8
    b = buf(b"".join(keys))
    t = time.perf_counter()
    assert ref.L.ref_key_import_many(ref.slot, int(grp["le"]), b, 33, 33, len(keys)) == 0
    return len(keys) / (time.perf_counter() - t)


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    L = build_ref(ref_root)
    vfx = M.load_fixture()
    curves = M.load_curves(vfx)
    rng = np.random.default_rng(0x6B6579)
    groups, rates = [], {}
    todo = [(g["curve"], bool(g["le"])) for g in vfx["cases"]]  # the same (curve, form) groups, in the same order
    todo += [(nm, False) for nm in EXTRA_BE if (nm, False) not in todo]
    for name, le in todo:
        ref = Ref(L, name)
        grp = group_of(ref, curves[name], le, rng)
        groups.append(grp)
        if not le:
            rates[name] = round(ref_rate(ref, grp), 1)
    with open(OUT, "w") as f:
        f.write('{"source": "include/crypto/dsa/ecdsa.h compiled from the reference (oracle/_ref), configuration of '
                'tests/golden/ref_ecdsa_key_shim.c",\n')
        f.write('"ref_rate": %s,\n' % json.dumps({
            "what": "compressed ecdsa_pub_key_import_be calls per second, one core of the generating machine, gcc -O2",
            "per_curve": rates}))
        f.write('"import_columns": ["name", "key", "key_y", "status", "infinity", "xy"],\n')
        f.write('"export_columns": ["name", "compress", "infinity", "xy", "out"],\n"groups": [\n')
        for i, g in enumerate(groups):
            f.write('{"curve": %s, "le": %s,\n"nums": %s,\n"import": [\n%s],\n"export": [\n%s]}%s\n' % (
                json.dumps(g["curve"]), json.dumps(g["le"]), json.dumps(g["nums"], separators=(",", ":")),
                ",\n".join(json.dumps(k, separators=(",", ":")) for k in g["import"]),
                ",\n".join(json.dumps(k, separators=(",", ":")) for k in g["export"]),
                "," if i + 1 < len(groups) else ""))
        f.write("]}\n")
    json.load(open(OUT))
    print("ecdsa_key.json: %d groups, %d import and %d export records, %d bytes" % (
        len(groups), sum(len(g["import"]) for g in groups), sum(len(g["export"]) for g in groups),
        os.path.getsize(OUT)))
    for g in groups:
        by = {}
        for k in g["import"]:
            by[k[3]] = by.get(k[3], 0) + 1
        print("%-45s %s" % (g["curve"], "le" if g["le"] else "be"), by,
              {k[0]: k[3] for k in g["import"] if k[0].startswith(("prefix", "compressed_x"))})
    print("reference compressed imports/s:", rates)


if __name__ == "__main__":
    main()
