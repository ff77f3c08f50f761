"""The wide signing kernels' arithmetic without a GPU:
liblcb_amd/csrc/ecdsa_sign_math.hpp at 12 and 16 limbs compiled for the host as
a stand-alone program (tests/c/ecdsa_wide_sign_host.cpp) with AddressSanitizer and UBSan.
Nothing is loaded into Python and nothing is preloaded.

1. Every record of tests/golden/ecdsa_wide_sign.json (what the reference
   returned and wrote) through sign_one<12 | 16>() and key_one<12 | 16>() over
   MulInline, the wide kernels' multiply-reduce: the same status and the same
   bytes, zeros where the status is not 0; the same again from the same
   formulas over MulCall, the other multiply-reduce; every status-0 signature
   with d != 0 accepted by verify_one() under key_one()'s key.
2. Window table entries T[j][v] = v 16^j G against Python ints
   (tests/ecdsa_model.mult): the four corners, all of window 0 and of the last
   window, and 64 more per curve."""
import os
import random
import subprocess

import pytest

from tests import ecdsa_wide_model as M
from tests import ecdsa_wide_sign_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VFX = M.load_fixture()
FX = K.load_fixture()
BY_NAME = {c["name"]: c for c in VFX["curves"]}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ecdsa_wide_sign_host") / "ecdsa_wide_sign_host")
    # -O0: every product is inlined at two limb counts and over two
    # multiply-reduces, and optimising that costs more time than it saves here
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "ecdsa_wide_sign_host.cpp"),
                           "-o", out])
    return out


def run(exe, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([exe], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, env=env)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    out = res.stdout.decode().splitlines()
    assert len(out) == len(lines)
    return out


def curve_line(c):
    return "C %d %s" % (c["algo"], " ".join(c[k] for k in M.NUMS))


def test_fixture_shape():
    assert [(g["curve"], g["le"]) for g in FX["groups"]] == [(g["curve"], g["le"]) for g in VFX["cases"]]
    for g in FX["groups"]:
        B = BY_NAME[g["curve"]]["bytes"]
        assert {0, -1, M.EINVAL} <= {k["status"] for k in g["sign"]}
        assert {k["hash_size"] for k in g["sign"]} >= {1, 20, B - 1, B, B + 1, 64, 65, 128}
        assert len(g["sign"]) >= 28 and len(g["key_gen"]) == 8 and len(g["pub_key"]) == 8
        for k in g["sign"]:
            assert len(k["hash"]) == 2 * k["hash_size"]
            assert len(k["d"]) == len(k["rnd"]) == len(k["r"]) == len(k["s"]) == 2 * B
            assert k["status"] == 0 or (k["r"], k["s"]) == ("00" * B, "00" * B)
        for k in g["key_gen"] + g["pub_key"]:
            assert k["status"] == 0 or (k["Qx"], k["Qy"]) == ("00" * B, "00" * B)
    assert set(FX["ref_rate"]["per_curve"]) == set(BY_NAME) == set(FX["notes"])


def test_every_fixture_record(exe):
    lines, want, ids = [], [], []
    for g in FX["groups"]:
        le = int(g["le"])
        lines.append(curve_line(BY_NAME[g["curve"]]))
        want.append("C ok")
        ids.append((g["curve"], le, "curve"))
        for k in g["sign"]:
            lines.append("S %d %d %s %s %s" % (le, k["hash_size"], k["hash"], k["d"], k["rnd"]))
            verified = "0" if k["status"] == 0 and int(k["d"], 16) != 0 else "-"
            want.append("%d %s %s 1 %s" % (k["status"], k["r"], k["s"], verified))
            ids.append((g["curve"], le, "sign", k["name"]))
        for k in g["key_gen"]:
            lines.append("K %d %s" % (le, k["rnd"]))
            want.append("%d %s %s %s 1" % (k["status"], k["d"], k["Qx"], k["Qy"]))
            ids.append((g["curve"], le, "key_gen", k["name"]))
        for k in g["pub_key"]:
            lines.append("P %d %s" % (le, k["d"]))
            want.append("%d %s %s 1" % (k["status"], k["Qx"], k["Qy"]))
            ids.append((g["curve"], le, "pub_key", k["name"]))
    got = run(exe, lines)
    bad = [(i, g, w) for i, g, w in zip(ids, got, want) if g != w]
    assert not bad, bad[:10]
    assert sum(1 for i in ids if i[2] == "sign") == sum(len(g["sign"]) for g in FX["groups"]) >= 224
    assert sum(1 for w in want if w.endswith(" 1 0")) > 150  # signatures that went through verify_one


def test_table_entries(exe):
    rng = random.Random(0x7AB1E512)
    lines, want = [], []
    for cj in VFX["curves"]:
        c = M.curve_from_json(cj)
        B = c["bytes"]
        W = 2 * B  # 8 L windows
        lines.append(curve_line(cj))
        want.append("C ok")
        sample = [(0, 1), (W - 1, 15), (0, 15), (W - 1, 1)]
        sample += [(0, v) for v in range(1, 16)] + [(W - 1, v) for v in range(1, 16)]
        sample += [(rng.randrange(W), rng.randrange(1, 16)) for _ in range(64)]
        for j, v in sample:
            x, y = M.mult(c, (v << (4 * j)) % c["n"], M.base(c))
            lines.append("T %d %d" % (j, v))
            want.append("%0*x %0*x" % (2 * B, x, 2 * B, y))
    got = run(exe, lines)
    bad = [(ln, g, w) for ln, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:3]
