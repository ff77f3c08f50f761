"""The signing kernels' arithmetic without a GPU:
liblcb_amd/csrc/ecdsa_sign_math.hpp compiled for the host as a stand-alone
program (tests/c/ecdsa_sign_host.cpp) with AddressSanitizer and UBSan.
Nothing is loaded into Python and nothing is preloaded.

1. Every record of tests/golden/ecdsa_sign.json (what the reference returned
   and wrote) through sign_one(), keygen_one() and pubkey_one(): the same
   status and the same bytes, zeros where the status is not 0.
2. Window table entries T[j][v] = v 16^j G against Python ints
   (tests/ecdsa_model.mult): the four corners and 64 more per curve."""
import json
import os
import random
import subprocess

import pytest

from tests import ecdsa_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VFX = M.load_fixture()
with open(os.path.join(ROOT, "tests", "golden", "ecdsa_sign.json")) as f:
    FX = json.load(f)
BY_NAME = {c["name"]: c for c in VFX["curves"]}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ecdsa_sign_host") / "ecdsa_sign_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "ecdsa_sign_host.cpp"),
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
        assert {0, -1, M.EINVAL} <= {k["status"] for k in g["sign"]}
        assert len(g["key_gen"]) == 8 and len(g["pub_key"]) == 8
        for k in g["sign"]:
            assert len(k["hash"]) == 2 * k["hash_size"]
            assert k["status"] == 0 or (k["r"], k["s"]) == ("00" * 32, "00" * 32)


def test_every_fixture_record(exe):
    lines, want, ids = [], [], []
    for g in FX["groups"]:
        le = int(g["le"])
        lines.append(curve_line(BY_NAME[g["curve"]]))
        want.append("C ok")
        ids.append((g["curve"], le, "curve"))
        for k in g["sign"]:
            lines.append("S %d %d %s %s %s" % (le, k["hash_size"], k["hash"], k["d"], k["rnd"]))
            want.append("%d %s %s" % (k["status"], k["r"], k["s"]))
            ids.append((g["curve"], le, "sign", k["name"]))
        for k in g["key_gen"]:
            lines.append("K %d %s" % (le, k["rnd"]))
            want.append("%d %s %s %s" % (k["status"], k["d"], k["Qx"], k["Qy"]))
            ids.append((g["curve"], le, "key_gen", k["name"]))
        for k in g["pub_key"]:
            lines.append("P %d %s" % (le, k["d"]))
            want.append("%d %s %s" % (k["status"], k["Qx"], k["Qy"]))
            ids.append((g["curve"], le, "pub_key", k["name"]))
    got = run(exe, lines)
    bad = [(i, g, w) for i, g, w in zip(ids, got, want) if g != w]
    assert not bad, bad[:10]
    assert sum(1 for i in ids if i[2] == "sign") == sum(len(g["sign"]) for g in FX["groups"]) > 300


def test_table_entries(exe):
    rng = random.Random(0x7AB1E)
    lines, want = [], []
    for cj in VFX["curves"]:
        c = M.curve_from_json(cj)
        lines.append(curve_line(cj))
        want.append("C ok")
        sample = [(0, 1), (63, 15), (0, 15), (63, 1)]
        sample += [(rng.randrange(64), rng.randrange(1, 16)) for _ in range(64)]
        for j, v in sample:
            x, y = M.mult(c, v << (4 * j), M.base(c))
            lines.append("T %d %d" % (j, v))
            want.append("%064x %064x" % (x, y))
    got = run(exe, lines)
    bad = [(ln, g, w) for ln, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:3]
