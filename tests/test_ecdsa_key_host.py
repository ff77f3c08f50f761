"""The key import / export kernels' arithmetic without a GPU:
liblcb_amd/csrc/ecdsa_key_math.hpp compiled for the host as a stand-alone
program (tests/c/ecdsa_key_host.cpp) with AddressSanitizer and UBSan.  Nothing
is loaded into Python and nothing is preloaded.

1. The fixture tests/golden/ecdsa_key.json holds what the issue of this
   library lists: 14 (curve, form) groups, both forms of the two curves with
   p = 1 (mod 8) among them, every key form and every way to refuse one.
2. Every record through key_import_one<8>() / key_export_one<8>() in the
   record's own form and, with the bytes of every number reversed, in the
   other form: the same status, the same bytes, zeros on rejection, the
   infinity flag, canaries around the outputs untouched.
3. mont_sqrt() against pow() on random residues and on the edge values.
4. key_setup()'s constants against Python ints."""
import os
import random
import subprocess

import pytest

from tests import ecdsa_key_cases as KC
from tests import ecdsa_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VFX = M.load_fixture()
FX = KC.load()
BY_NAME = {c["name"]: c for c in VFX["curves"]}
CURVES = M.load_curves(VFX)
P1MOD8 = ("id-gostR3410-2001-Test_ParamSet", "id-gostR3410-2001-CryptoPro-B-ParamSet")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ecdsa_key_host") / "ecdsa_key_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "ecdsa_key_host.cpp"),
                           "-o", out])
    return out


def run(exe, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([exe], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, env=env)
    assert res.returncode == 0, (res.returncode, res.stderr.decode()[-2000:])
    out = res.stdout.decode().splitlines()
    assert len(out) == len(lines)
    return out


def curve_line(c):
    return "C %d %s" % (c["algo"], " ".join(c[k] for k in M.NUMS))


def two_adic(p):
    s, q = 0, p - 1
    while q % 2 == 0:
        s, q = s + 1, q // 2
    return s, q


def test_fixture_shape():
    assert os.path.getsize(KC.PATH) < 200 * 1024
    ids = [(g["curve"], g["le"]) for g in FX["groups"]]
    assert ids[:12] == [(g["curve"], bool(g["le"])) for g in VFX["cases"]] and len(set(ids)) == len(ids) == 14
    for nm in P1MOD8:
        assert CURVES[nm]["p"] % 8 == 1 and (nm, False) in ids and (nm, True) in ids
    assert sorted(two_adic(CURVES[nm]["p"])[0] for nm in P1MOD8) == [3, 4]
    assert all(c["p"] % 4 == 3 for nm, c in CURVES.items() if nm not in P1MOD8)
    for g in FX["groups"]:
        c, le = CURVES[g["curve"]], g["le"]
        p, n = c["p"], c["n"]
        rec = {k["name"]: k for k in g["imports"]}
        assert len(rec) == len(g["imports"]) >= 140
        num = lambda b: M.num(b, le)  # noqa: E731
        rhs = lambda x: (x * x * x + c["a"] * x + c["b"]) % p  # noqa: E731
        G = M.base(c)
        points = [nm[:-len("/packed")] for nm in rec if nm.endswith("/packed")]
        assert len(points) >= 11 and points[:3] == ["G", "2G", "n_minus_1_G"]
        assert (num(rec["G/packed"]["xy"][:32]), num(rec["G/packed"]["xy"][32:])) == G
        assert (num(rec["2G/raw"]["xy"][:32]), num(rec["2G/raw"]["xy"][32:])) == M.mult(c, 2, G)
        assert (num(rec["n_minus_1_G/xy"]["xy"][:32]), num(rec["n_minus_1_G/xy"]["xy"][32:])) == M.mult(c, n - 1, G)
        for pt in points:
            k = rec[pt + "/packed"]
            x, y = num(k["xy"][:32]), num(k["xy"][32:])
            bx, by = k["xy"][:32], k["xy"][32:]
            assert M.on_curve(c, x, y) and k["key"] == b"\x04" + bx + by and k["status"] == 0
            k = rec[pt + "/compressed"]
            assert (k["key"], k["status"], k["xy"]) == (bytes([2 | y & 1]) + bx, 0, bx + by)
            k = rec[pt + "/compressed_other"]                  # the other root
            assert (k["key"], k["status"], k["xy"]) == (bytes([3 - (y & 1)]) + bx, 0, bx + M.to_bytes(p - y, le))
            k = rec[pt + "/hybrid_right"]
            assert (k["key"], k["status"], k["xy"]) == (bytes([6 | y & 1]) + bx + by, 0, bx + by)
            k = rec[pt + "/hybrid_wrong"]                      # the prefix's parity is not compared
            assert (k["key"], k["status"], k["xy"]) == (bytes([7 - (y & 1)]) + bx + by, 0, bx + by)
            k = rec[pt + "/raw"]
            assert (k["key"], k["key_y"], k["status"], k["xy"]) == (bx + by, None, 0, bx + by)
            k = rec[pt + "/xy"]
            assert (k["key"], k["key_y"], k["status"], k["xy"]) == (bx, by, 0, bx + by)
            k = rec[pt + "/x_without_y"]
            assert (k["key"], k["key_y"], k["status"], k["xy"]) == (bx, None, M.EINVAL, KC.ZERO64)
        nres = [k for nm, k in rec.items() if nm.startswith("non_residue_")]
        assert len(nres) >= 4 and {k["key"][0] for k in nres} == {2, 3}
        for k in nres:
            x = num(k["key"][1:])
            assert k["status"] == -1 and x < p and pow(rhs(x), (p - 1) // 2, p) == p - 1
        for nm, v in (("x_eq_p", p), ("x_p_plus_1", p + 1), ("x_ff", (1 << 256) - 1)):
            for pre in (2, 3):
                k = rec["compressed_%s_%02x" % (nm, pre)]
                assert k["status"] == -1 and k["key"] == bytes([pre]) + M.to_bytes(v, le)
        if c["Gx"] == 0:
            for pre in (2, 3):
                k = rec["compressed_x_zero_%02x" % pre]
                assert k["status"] == 0 and num(k["xy"][:32]) == 0 and num(k["xy"][32:]) & 1 == pre & 1
        for size, good in ((33, (2, 3)), (65, (4, 6, 7))):
            for pre in (0, 1, 2, 3, 4, 5, 6, 7, 0xFF):
                k = rec["prefix_%02x_size_%d" % (pre, size)]
                assert len(k["key"]) == size and k["key"][0] == pre and k["status"] == (0 if pre in good else -1)
        assert (rec["size_1_byte_0"]["status"], rec["size_1_byte_0"]["infinity"]) == (0, 1)
        assert (rec["size_1_byte_1"]["status"], rec["size_1_byte_1"]["infinity"]) == (M.EINVAL, 0)
        assert rec["size_0"]["status"] == rec["size_0_with_y"]["status"] == M.EINVAL
        for size in (2, 31, 34, 63, 66):
            assert len(rec["size_%d" % size]["key"]) == size
            assert rec["size_%d" % size]["status"] == rec["size_%d_with_y" % size]["status"] == -1
        for form in ("packed", "raw"):
            for what in ("y_bit", "y_high_bit", "y_eq_p", "x_eq_p", "zero_zero"):
                assert rec["%s_%s" % (form, what)]["status"] == -1
            assert num(rec[form + "_y_eq_p"]["key"][-32:]) == p and num(rec[form + "_x_eq_p"]["key"][-64:-32]) == p
        assert rec["xy_y_bit"]["status"] == rec["xy_y_eq_p"]["status"] == -1
        for k in g["imports"]:
            assert k["status"] in (0, -1, M.EINVAL) and k["infinity"] in (0, 1)
            if k["status"] != 0 or k["infinity"]:
                assert k["xy"] == KC.ZERO64
            else:                                              # accepted: on the curve, and for a compressed key
                x, y = num(k["xy"][:32]), num(k["xy"][32:])    # the root of the stated parity
                assert x < p and y < p and M.on_curve(c, x, y), (g["curve"], k["name"])
                if len(k["key"]) == 33:
                    assert pow(y, 2, p) == rhs(x) and y & 1 == k["key"][0] & 1 and num(k["key"][1:]) == x
        ex = {k["name"]: k for k in g["exports"]}
        assert len(ex) == len(g["exports"]) >= 2 * 11 + 4
        for k in g["exports"]:
            if k["infinity"]:
                assert k["out"] == b"\x00"
            elif k["compress"]:
                assert k["out"] == bytes([2 | num(k["xy"][32:]) & 1]) + k["xy"][:32]
            else:
                assert k["out"] == b"\x04" + k["xy"]
        k = ex["off_curve/compressed"]
        assert not M.on_curve(c, num(k["xy"][:32]), num(k["xy"][32:])) and len(k["out"]) == 33
        assert {(k["compress"], k["infinity"]) for k in g["exports"]} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_every_fixture_record_in_both_forms(exe):
    lines, want, ids = [], [], []
    h = lambda b: b.hex() if b else "-"  # noqa: E731
    for g in FX["groups"]:
        lines.append(curve_line(BY_NAME[g["curve"]]))
        want.append(None)
        ids.append((g["curve"], "curve"))
        le = int(g["le"])
        for k in g["imports"]:
            ky = k["key_y"]
            lines.append("I %d %d %s %s" % (le, len(k["key"]), h(k["key"]), "-" if ky is None else ky.hex()))
            want.append("%d %d %s" % (k["status"], k["infinity"], k["xy"].hex()))
            ids.append((g["curve"], le, k["name"]))
            lines.append("I %d %d %s %s" % (1 - le, len(k["key"]), h(KC.flip_key(k["key"])),
                                            "-" if ky is None else ky[::-1].hex()))
            want.append("%d %d %s" % (k["status"], k["infinity"], KC.flip_xy(k["xy"]).hex()))
            ids.append((g["curve"], 1 - le, k["name"]))
        for k in g["exports"]:
            lines.append("E %d %d %d %s" % (le, k["compress"], k["infinity"], k["xy"].hex()))
            want.append("%d %s" % (len(k["out"]), k["out"].hex()))
            ids.append((g["curve"], le, "export", k["name"]))
            lines.append("E %d %d %d %s" % (1 - le, k["compress"], k["infinity"], KC.flip_xy(k["xy"]).hex()))
            want.append("%d %s" % (len(k["out"]), KC.flip_key(k["out"]).hex()))
            ids.append((g["curve"], 1 - le, "export", k["name"]))
    got = run(exe, lines)
    bad = [(i, g, w) for i, g, w in zip(ids, got, want) if w is not None and g != w]
    assert not bad, bad[:10]
    assert all(g.startswith("C ok ") for g, w in zip(got, want) if w is None)
    assert len(lines) == 14 + 2 * sum(len(g["imports"]) + len(g["exports"]) for g in FX["groups"]) > 4000


def test_square_root_against_pow(exe):
    rng = random.Random(0x5172)
    lines, want = [], []
    for name, c in CURVES.items():
        p = c["p"]
        lines.append(curve_line(BY_NAME[name]))
        want.append(None)
        vals = [(0, True), (1, True), (4, True), (p - 1, p % 4 == 1)]
        for _ in range(64):
            r = rng.randrange(1, p)
            vals.append((r * r % p, True))
        for _ in range(16):
            v = rng.randrange(1, p)
            vals.append((v, pow(v, (p - 1) // 2, p) == 1))
        assert sum(1 for _, sq in vals if not sq) >= 2 or p % 4 == 1
        for v, sq in vals:
            lines.append("S %064x" % v)
            want.append((name, v, sq))
    got = run(exe, lines)
    checked = 0
    for g, w in zip(got, want):
        if w is None:
            assert g.startswith("C ok "), g
            continue
        name, v, sq = w
        p = CURVES[name]["p"]
        r, ok = int(g.split()[0], 16), int(g.split()[1])
        assert ok == int(sq), (name, hex(v), g)
        if sq:
            assert r < p and r * r % p == v, (name, hex(v), g)
            checked += 1
    assert checked >= 10 * 67


def test_host_derived_constants(exe):
    got = run(exe, [curve_line(BY_NAME[name]) for name in CURVES])
    for name, g in zip(CURVES, got):
        p = CURVES[name]["p"]
        s, q = two_adic(p)
        z = next(z for z in range(2, 256) if pow(z, (p - 1) // 2, p) == p - 1)
        assert g == "C ok %d %064x %064x" % (s, (q - 1) // 2, pow(z, q, p)), (name, g)
        if s == 1:                                             # the candidate is v^((p + 1) / 4)
            assert (q - 1) // 2 + 1 == (p + 1) // 4
        assert pow(pow(z, q, p), 1 << (s - 1), p) == p - 1     # order exactly 2^s
