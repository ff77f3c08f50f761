"""The key agreement kernel's arithmetic without a GPU:
liblcb_amd/csrc/ecdsa_dh_math.hpp compiled for the host as a stand-alone
program (tests/c/ecdsa_dh_host.cpp) with AddressSanitizer and UBSan.  Nothing
is loaded into Python and nothing is preloaded.

1. The fixture tests/golden/ecdsa_dh.json holds what the issue of this
   library lists: the 12 (curve, form) groups, every kind of scalar and key,
   and for every accepted record the x coordinate of the plain d Q
   (tests/ecdsa_model.mult).
2. Every record through dh_one<8>() in the record's own form and, with the
   bytes of every number reversed, in the other form: the same status and the
   same 32 bytes, zeros where the status is not 0, canaries around the output
   untouched."""
import json
import os
import subprocess

import pytest

from tests import ecdsa_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VFX = M.load_fixture()
with open(os.path.join(ROOT, "tests", "golden", "ecdsa_dh.json")) as f:
    FX = json.load(f)
BY_NAME = {c["name"]: c for c in VFX["curves"]}
CURVES = M.load_curves(VFX)
ZERO = "00" * 32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ecdsa_dh_host") / "ecdsa_dh_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "ecdsa_dh_host.cpp"),
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


def flip(h):
    """The same number in the other byte order."""
    return bytes.fromhex(h)[::-1].hex()


def test_fixture_shape():
    assert [(g["curve"], g["le"]) for g in FX["groups"]] == [(g["curve"], g["le"]) for g in VFX["cases"]]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ecdsa_dh.json")) < 200 * 1024
    for g in FX["groups"]:
        c, le = CURVES[g["curve"]], g["le"]
        n, p = c["n"], c["p"]
        recs = {k["name"]: k for k in g["records"]}
        assert len(recs) == len(g["records"]) >= 39
        num = lambda h: M.num(bytes.fromhex(h), le)  # noqa: E731
        ds = {num(k["d"]) for k in g["records"] if k["status"] == 0}
        top = 1 << 255 if (1 << 255) < n else 1 << 254
        want = {1, 2, 3, 4, 5, 7, 8, 15, 16, 17, n - 1, n - 2, n - 3, (n - 1) // 2, (n + 1) // 2, top, 1 << 128,
                (1 << 128) - 1} | {int.from_bytes(bytes([b]) * 32, "big") % n for b in (0x55, 0xAA, 0x33, 0x0F)}
        assert want <= ds, (g["curve"], [hex(v) for v in want - ds])
        G = M.base(c)
        qs = {(num(k["Qx"]), num(k["Qy"])) for k in g["records"] if k["status"] == 0}
        assert {G, M.mult(c, 2, G), M.mult(c, n - 1, G)} <= qs and len(qs) >= 5
        # the statuses the reference gave, by kind
        assert recs["d_zero"]["status"] == -1 and num(recs["d_zero"]["d"]) == 0
        for nm, v in (("d_eq_n", n), ("d_n_plus_1", n + 1), ("d_ff", (1 << 256) - 1)):
            assert recs[nm]["status"] == M.EINVAL and num(recs[nm]["d"]) == v
        assert recs["Qx_eq_p"]["status"] == -1 and num(recs["Qx_eq_p"]["Qx"]) == p
        assert recs["Qy_eq_p"]["status"] == -1 and num(recs["Qy_eq_p"]["Qy"]) == p
        assert recs["Qy_plus_1"]["status"] == -1
        assert recs["Q_zero_zero"]["status"] == -1 and (recs["Q_zero_zero"]["Qx"], recs["Q_zero_zero"]["Qy"]) == (
            ZERO, ZERO)
        k = recs["Q_off_curve_d_eq_n"]                 # a bad key wins over d >= n
        assert k["status"] == -1 and num(k["d"]) == n and not M.on_curve(c, num(k["Qx"]), num(k["Qy"]))
        if "Qx_plus_p" in recs:
            k = recs["Qx_plus_p"]
            assert k["status"] == -1 and M.on_curve(c, num(k["Qx"]) - p, num(k["Qy"]))
        else:
            assert min(x for x, _ in qs) + p > (1 << 256) - 1
        assert recs["agree_dA_QB"]["shared"] == recs["agree_dB_QA"]["shared"] != ZERO
        assert recs["agree_dA_QB"]["d"] != recs["agree_dB_QA"]["d"]
        assert recs["cofactor_0"]["shared"] == recs["cofactor_1"]["shared"] != ZERO
        assert (recs["cofactor_0"]["use_cofactor"], recs["cofactor_1"]["use_cofactor"]) == (0, 1)
        assert {k["use_cofactor"] for k in g["records"]} == {0, 1}
        for k in g["records"]:
            assert k["status"] in (0, -1, M.EINVAL)
            if k["status"] != 0:
                assert k["shared"] == ZERO
            else:                                      # the plain d Q is the specification
                R = M.mult(c, num(k["d"]), (num(k["Qx"]), num(k["Qy"])))
                assert R is not None and M.to_bytes(R[0], le).hex() == k["shared"], (g["curve"], k["name"])
    assert len([g for g in FX["groups"] if any(k["name"] == "Qx_plus_p" for k in g["records"])]) >= 6


def test_every_fixture_record_in_both_forms(exe):
    lines, want, ids = [], [], []
    for g in FX["groups"]:
        lines.append(curve_line(BY_NAME[g["curve"]]))
        want.append("C ok")
        ids.append((g["curve"], "curve"))
        for k in g["records"]:
            le = int(g["le"])
            lines.append("D %d %s %s %s" % (le, k["Qx"], k["Qy"], k["d"]))
            want.append("%d %s" % (k["status"], k["shared"]))
            ids.append((g["curve"], le, k["name"]))
            lines.append("D %d %s %s %s" % (1 - le, flip(k["Qx"]), flip(k["Qy"]), flip(k["d"])))
            want.append("%d %s" % (k["status"], flip(k["shared"])))
            ids.append((g["curve"], 1 - le, k["name"]))
    got = run(exe, lines)
    bad = [(i, g, w) for i, g, w in zip(ids, got, want) if g != w]
    assert not bad, bad[:10]
    assert len(lines) == 12 + 2 * sum(len(g["records"]) for g in FX["groups"]) > 900
