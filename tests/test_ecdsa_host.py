"""The kernel's arithmetic without a GPU: liblcb_amd/csrc/ecdsa_math.hpp
compiled for the host as a stand-alone program (tests/c/ecdsa_verify_host.cpp)
with AddressSanitizer and UBSan.  Nothing is loaded into Python and nothing is
preloaded.

1. The per-curve Montgomery constants (R mod m, R^2 mod m, -m^-1 mod 2^32 for
   p and n) equal what Python ints give.
2. 1,000 random Montgomery products and 20 inverses per modulus (p and n of
   every curve) equal a b R^-1 mod m and a^-1 mod m over Python ints; the
   operands include 0, 1 and m - 1.  Every product is computed by both
   multiply-reduces of the header (MulCall, the kernel's at 8 limbs, and
   MulInline, the wide kernels') and both must give that number.
3. verify_one() gives the reference's status for every case of
   tests/golden/ecdsa.json, reading exactly hash_size / 32 bytes."""
import os
import random
import subprocess

import pytest

from tests import ecdsa_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = M.load_fixture()
R = 1 << 256


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ecdsa_host") / "ecdsa_verify_host")
    # -g1: line tables for the sanitizers' reports; full -g triples the build time (variable tracking)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "ecdsa_verify_host.cpp"),
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


def h64(v):
    return "%064x" % v


def test_montgomery_products_and_inverses(exe):
    rng = random.Random(0xEC)
    lines, want = [], []
    for cj in FX["curves"]:
        c = M.curve_from_json(cj)
        lines.append(curve_line(cj))
        exp = ["ok"]
        for m in (c["p"], c["n"]):
            exp += ["%08x" % ((-pow(m, -1, 1 << 32)) % (1 << 32)), h64(R % m), h64(R * R % m)]
        want.append("C " + " ".join(exp))
        for which, m in (("p", c["p"]), ("n", c["n"])):
            edge = [0, 1, m - 1, m - 2, R % m]
            pairs = [(a, b) for a in edge for b in edge]
            pairs += [(rng.randrange(m), rng.randrange(m)) for _ in range(500 - len(pairs))]
            for a, b in pairs:
                lines.append("M %s %s %s" % (which, h64(a), h64(b)))
                want.append("%s %s" % ((h64(a * b * pow(R, -1, m) % m),) * 2))  # MulCall, MulInline
            for a in [1, 2, m - 1] + [rng.randrange(1, m) for _ in range(17)]:
                lines.append("I %s %s" % (which, h64(a)))
                want.append(h64(pow(a, -1, m)))
    got = run(exe, lines)
    bad = [(ln, g, w) for ln, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:3]


def test_setup_refuses_what_verify_cannot_take(exe):
    cj = dict(FX["curves"][0])
    even = dict(cj, n=h64(int(cj["n"], 16) - 1))
    short = dict(cj, n=h64(int(cj["n"], 16) >> 3 | 1))
    big_a = dict(cj, a=cj["p"])
    assert run(exe, [curve_line(even), curve_line(short), curve_line(big_a),
                     "C 2 " + " ".join(cj[k] for k in M.NUMS)]) == ["C bad"] * 4


def test_every_fixture_status(exe):
    by_name = {c["name"]: c for c in FX["curves"]}
    lines, want, ids = [], [], []
    for grp in FX["cases"]:
        lines.append(curve_line(by_name[grp["curve"]]))
        want.append(None)
        ids.append(None)
        for k in grp["records"]:
            lines.append("V %d %d %s %s %s %s %s" % (k["le"], k["hash_size"], k["hash"], k["r"], k["s"], k["Qx"],
                                                     k["Qy"]))
            want.append(str(k["status"]))
            ids.append((grp["curve"], k["le"], k["name"]))
    got = run(exe, lines)
    bad = [(i, g, w) for i, g, w in zip(ids, got, want) if w is not None and g != w]
    assert not bad, bad[:10]
