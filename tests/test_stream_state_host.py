"""The record of include/lcb_hash_stream_gpu.h without a GPU.

1. liblcb_amd/csrc/stream_state.hpp (import validation, record <-> context
   words, index check) as a stand-alone program built with AddressSanitizer
   and UBSan (tests/c/stream_state_host.cpp): every record of
   tests/golden/stream.json is accepted and survives the round trip through
   the context words byte for byte; a wrong algorithm, used == B and
   used != count % B are refused.  Nothing is loaded into Python and nothing
   is preloaded.
2. tests/c/stream_resume.c, built against the drop-in headers of
   include/crypto/hash: a drop-in context filled from each fixture record,
   fed the rest of the message, must give the fixture's digest: the mapping
   INTEGRATION.md documents."""
import errno
import json
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = json.load(open(os.path.join(ROOT, "tests", "golden", "stream.json")))
DT = np.dtype([("alg", "<u4"), ("used", "<u4"), ("count", "<u8"), ("count_hi", "<u8"),
               ("h", "u1", (64,)), ("n", "u1", (64,)), ("sigma", "u1", (64,)), ("buf", "u1", (128,))])


def message(case):
    from oracle.pyoracle import gen_stream
    return gen_stream(FX["seed"], case["length"]).tobytes()


def test_fixture_shape():
    assert [c["name"] for c in FX["cases"]] == ["md5", "sha1", "sha224", "sha256", "sha384", "sha512", "gost256",
                                                "gost512", "hmac_md5", "hmac_sha256"]
    for c in FX["cases"]:
        B = c["block"]
        assert B == (128 if c["alg"] in (5, 6) else 64) and c["length"] == 3 * B + 5
        assert [r["prefix"] for r in c["records"]] == [0, 1, B - 1, B, B + 1, 2 * B, 3 * B + 5]
        assert (c["key"] is None) == (not c["name"].startswith("hmac_")) and (c["key"] is None or len(c["key"]) == 20)
        msg = message(c)
        for r in c["records"]:
            rec = np.frombuffer(bytes.fromhex(r["record"]), DT)[0]
            n = r["prefix"] + (B if c["key"] else 0)     # HMAC: the ipad block counts
            assert rec["alg"] == c["alg"] and rec["used"] == r["prefix"] % B and rec["count"] == n
            assert bytes(rec["buf"][:rec["used"]]) == msg[r["prefix"] - rec["used"]:r["prefix"]]
            assert not rec["buf"][rec["used"]:].any() and rec["count_hi"] == 0
            if c["alg"] >= 7:                            # N counts the bits of the whole blocks
                assert int.from_bytes(bytes(rec["n"]), "little") == 8 * (n - rec["used"])
            else:
                assert not rec["n"].any() and not rec["sigma"].any()


@pytest.fixture(scope="module")
def state_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("stream_state") / "stream_state_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "stream_state_host.cpp"),
                           "-o", out])
    return out


def test_import_validation_under_sanitizers(state_exe):
    E = errno.EINVAL
    cases = []   # (set alg, record bytes, expected rc)
    for c in FX["cases"]:
        B = c["block"]
        for r in c["records"]:
            raw = bytes.fromhex(r["record"])
            cases.append((c["alg"], raw, 0))
            cases.append((c["alg"] % 8 + 1, raw, E))                 # a set of another algorithm
            rec = np.frombuffer(raw, DT).copy()
            bad = rec.copy(); bad["alg"] = 0
            cases.append((c["alg"], bad.tobytes(), E))
            bad = rec.copy(); bad["used"] = B                        # a full buffer is never kept
            if c["alg"] < 7:
                bad["count"] = B
            cases.append((c["alg"], bad.tobytes(), E))
            bad = rec.copy(); bad["used"] = 200
            cases.append((c["alg"], bad.tobytes(), E))
            bad = rec.copy(); bad["used"] = (int(rec["used"][0]) + 1) % B   # used != count % B
            cases.append((c["alg"], bad.tobytes(), E if c["alg"] < 7 else 0))
        cases.append((0, bytes.fromhex(c["records"][0]["record"]), E))
        cases.append((9, bytes.fromhex(c["records"][0]["record"]), E))
    blob = b"".join(struct.pack("<i", a) + raw for a, raw, _ in cases)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([state_exe], input=blob, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    lines = res.stdout.decode().splitlines()
    assert len(lines) == len(cases) + 1
    for (alg, raw, want), line in zip(cases, lines):
        got = line.split()
        assert int(got[0]) == want, (alg, raw.hex(), line)
        if want == 0:
            rec = np.frombuffer(raw, DT)[0]
            back = np.frombuffer(bytes.fromhex(got[1]), DT)[0]
            # bytes of buf at or past `used` are dropped, GOST's count is N / 8 + used; everything else survives
            exp = rec.copy()
            exp["buf"][int(rec["used"]):] = 0
            if alg >= 7:
                exp["count"] = (int.from_bytes(bytes(rec["n"][:16]), "little") // 8 + int(rec["used"])) % (1 << 64)
            assert back.tobytes() == exp.tobytes(), (alg, raw.hex(), got[1])
    # ok list, an index past the set, one twice, reversed, no list, no list past the set; `seen` is zero again
    assert lines[-1].split() == ["index", "0", str(E), str(E), "0", "0", str(E), "0", "0", "0", "0", "0"]


def test_dropin_context_resumes_from_record(tmp_path):
    exe = str(tmp_path / "stream_resume")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "stream_resume.c"), "-o", exe])
    blob, want = b"", []
    for c in FX["cases"]:
        msg = message(c)
        key = bytes.fromhex(c["key"]) if c["key"] is not None else None
        for r in c["records"]:
            rest = msg[r["prefix"]:]
            blob += struct.pack("<ii", c["alg"], len(key) if key is not None else -1) + (key or b"")
            blob += bytes.fromhex(r["record"]) + struct.pack("<i", len(rest)) + rest
            want.append(c["digest"])
    out = subprocess.run([exe], input=blob, stdout=subprocess.PIPE, check=True).stdout.decode().split()
    assert out == want
