"""The wide kernels' arithmetic without a GPU:
liblcb_amd/csrc/ecdsa_math.hpp at 12 and 16 limbs compiled for the host as a
stand-alone program (tests/c/ecdsa_wide_host.cpp) with AddressSanitizer and UBSan, over
the library's own curve table.  Nothing is loaded into Python and nothing is
preloaded.

1. The Montgomery constants of all twelve moduli (R mod m, R^2 mod m,
   -m^-1 mod 2^32 for p and n of the six curves) equal what Python ints give.
2. Random Montgomery products and inverses per modulus equal a b R^-1 mod m
   and a^-1 mod m over Python ints, from the rolled multiply-reduce (MulInline)
   and from the out-of-line one (MulCall); the operands include 0, 1 and m - 1.
3. For every record of tests/golden/ecdsa_wide.json three statuses agree:
   verify_one<12 | 16>() over MulInline (the wide kernels'), over MulCall, and
   the reference's; exactly hash_size / B bytes are read."""
import os
import random
import subprocess

import pytest

from tests import ecdsa_wide_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = M.load_fixture()
IDS = {c["name"]: i for i, c in enumerate(FX["curves"])}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ecdsa_wide_host") / "ecdsa_wide_host")
    # -g1: line tables for the sanitizers' reports; full -g triples the build time (variable tracking)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "ecdsa_wide_host.cpp"),
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


def test_montgomery_constants_products_and_inverses(exe):
    rng = random.Random(0xEC512)
    lines, want = [], []
    for cid, cj in enumerate(FX["curves"]):
        c = M.curve_from_json(cj)
        B = c["bytes"]
        R = 1 << (8 * B)
        hx = lambda v: "%0*x" % (2 * B, v)  # noqa: E731
        lines.append("K %d" % cid)
        exp = [str(B)]
        for m in (c["p"], c["n"]):
            exp += ["%08x" % ((-pow(m, -1, 1 << 32)) % (1 << 32)), hx(R % m), hx(R * R % m)]
        want.append("K " + " ".join(exp))
        for which, m in (("p", c["p"]), ("n", c["n"])):
            edge = [0, 1, m - 1, m - 2, R % m]
            pairs = [(a, b) for a in edge for b in edge]
            pairs += [(rng.randrange(m), rng.randrange(m)) for _ in range(200 - len(pairs))]
            for a, b in pairs:
                lines.append("M %d %s %s %s" % (cid, which, hx(a), hx(b)))
                v = hx(a * b * pow(R, -1, m) % m)
                want.append(v + " " + v)
            for a in [1, 2, m - 1] + [rng.randrange(1, m) for _ in range(5)]:
                lines.append("I %d %s %s" % (cid, which, hx(a)))
                want.append(hx(pow(a, -1, m)))
    lines.append("K 6")
    want.append("K bad")
    got = run(exe, lines)
    bad = [(ln, g, w) for ln, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:3]
    assert sum(1 for ln in lines if ln.startswith("K")) == 7      # twelve moduli and the id past the table


def test_every_fixture_status_from_both_headers(exe):
    lines, want, ids = [], [], []
    for grp in FX["cases"]:
        for k in grp["records"]:
            lines.append("V %d %d %d %s %s %s %s %s" % (IDS[grp["curve"]], k["le"], k["hash_size"], k["hash"],
                                                        k["r"], k["s"], k["Qx"], k["Qy"]))
            want.append("%d %d" % (k["status"], k["status"]))
            ids.append((grp["curve"], k["le"], k["name"]))
    for grp in FX["messages"]:
        for i, k in enumerate(grp["records"]):
            lines.append("V %d %d %d %s %s %s %s %s" % (IDS[grp["curve"]], grp["le"], len(k["hash"]) // 2, k["hash"],
                                                        k["r"], k["s"], k["Qx"], k["Qy"]))
            want.append("%d %d" % (k["status"], k["status"]))
            ids.append((grp["curve"], grp["le"], "message_%d" % i))
    got = run(exe, lines)
    bad = [(i, g, w) for i, g, w in zip(ids, got, want) if g != w]
    assert not bad, bad[:10]
