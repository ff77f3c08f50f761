"""The packet walk the RADIUS parse kernel compiles
(liblcb_amd/csrc/radius_parse.hpp) as a stand-alone host program built with
AddressSanitizer and UBSan (tests/c/radius_parse_host.cpp).  Every packet sits
in a heap block of exactly its buffer size, so a read outside the buffer ends
the program with a report; the records it prints are compared with a small
Python model: a find_attr-style walk plus the guard rules of
include/lcb_radius_gpu.h, and the step plan from liblcb_amd.radius's code
tables.  The packets of tests/golden/radius_matrix.json (every code, layout
and request, the 4096-byte ones and a list of 2038 two-byte attributes) go
through the same program, and its verdicts for them are also held against the
REFERENCE's result codes in that fixture, with no Python model in between.
Nothing is loaded into Python and nothing is preloaded."""
import errno
import json
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
E = errno.EBADMSG
REQ_AUTH = b"\x01" * 16


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("radius_parse") / "radius_parse_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "radius_parse_host.cpp"),
                           "-o", out])
    return out


def model(pkt, key_index, nkeys, req_code):
    """The 16 numbers radius_parse_host prints for one record."""
    from liblcb_amd import radius as R
    bad = lambda e: [e] + [0] * 15  # noqa: E731
    n = len(pkt)
    if n < 20:
        return bad(E)
    L = int.from_bytes(pkt[2:4], "big")
    if L < 20 or L > n or L > 4096:
        return bad(E)
    i, ma, pw = 20, None, None
    while i < L:
        if L - i < 2:
            return bad(E)
        t, ln = pkt[i], pkt[i + 1]
        if ln < 2 or t == 0 or i + ln > L:
            return bad(E)
        if t == 80 and ma is None:
            ma = (i, ln)
        if t == 2 and pw is None:
            pw = (i, ln - 2)
        i += ln
    if key_index >= nkeys:
        return bad(errno.EINVAL)
    assert (ma[0] if ma else None) == R.find_attr(pkt, 80) and (pw[0] if pw else None) == R.find_attr(pkt, 2)
    rec = [0, L, ma[0] if ma else 0, ma[1] if ma else 0, pw[0] if pw else 0, pw[1] if pw else 0, key_index]
    sign = (R._pw_check(pw[1]) if pw else 0) or (E if ma and ma[1] != 18 else 0)
    code = pkt[0]
    req = bytes([req_code, 0, 0, 20]) + REQ_AUTH if req_code else None
    mode = lambda a: 0 if a is None else 1 if a == bytes(16) else 2  # noqa: E731
    e1 = e2 = e3 = ma_mode = au_mode = 0
    if ma:
        a = E if ma[1] != 18 else R._ma_authenticator(code, req)
        if isinstance(a, int):
            e1 = a
        else:
            ma_mode = mode(a)
    if code not in R.RANDOM_AUTH:
        a = R._auth_authenticator(code, req)
        if isinstance(a, int):
            e2 = a
        else:
            au_mode = mode(a)
    if pw and (pw[1] == 0 or pw[1] % 16 or pw[1] > 128):
        e3 = errno.EINVAL
    p_ma = int(bool(ma) and not e1)
    p_au = int(code not in R.RANDOM_AUTH and not e1 and not e2)
    p_pw = int(bool(pw) and not (e1 or e2 or e3))
    return rec + [sign, e1, e2, e3, p_ma, p_au, p_pw, ma_mode if p_ma else None, au_mode if p_au else None]


@pytest.fixture(scope="module")
def matrix(oracle):
    """The packets of radius_matrix.json as verify sees them (signed; as built
    where sign refuses), checked against the fixture's hashes, each with its
    request's code: (fixture cases, records)."""
    from tests.test_radius_matrix import Matrix
    mx = Matrix(oracle, verify=False)
    return mx.cases, [(b, c["key"], len(mx.secrets), c["request"]) for b, c in zip(mx.inputs("verify"), mx.cases)]


def walk(exe, recs):
    """The program's 16 numbers for every record, under the sanitizers."""
    blob = b"".join(struct.pack("<IIII", len(b), k, n, r) + b for b, k, n, r in recs)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([exe], input=blob, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    lines = res.stdout.decode().splitlines()
    assert len(lines) == len(recs)
    return [[int(x) for x in line.split()] for line in lines]


def records(matrix=()):
    """(packet buffer, key_index, nkeys, req_code) for every case; `matrix`:
    the records of radius_matrix.json, appended with the longest attribute list
    a packet can hold (2038 two-byte attributes) under three codes."""
    P = json.load(open(os.path.join(G, "radius.json")))["packets"]
    base = [(bytes.fromhex(p["signed"]), p["key"], 5, bytes.fromhex(p["request"])[0] if p["kind"] == "reply" else 0)
            for p in P]
    edge = json.load(open(os.path.join(G, "radius_edge.json")))["cases"]
    base += [(bytes.fromhex(c["pre"]), c["key"], 5, 0) for c in edge]
    out = list(base)
    # a reply without its request, under another request's code, a bad key index
    out += [(b, k, n, 0) for b, k, n, r in base[::7] if r]
    out += [(b, k, n, 12) for b, k, n, r in base[::5]]
    out += [(b, 5 + k, 5, r) for b, k, n, r in base[::9]]
    # codes radius.h does not know, and a Message-Authenticator one byte short (the last attribute)
    out += [(bytes([99 if m % 2 else 6]) + b[1:], k, n, r) for m, (b, k, n, r) in enumerate(base[::11])]
    for b, k, n, r in base:
        L = int.from_bytes(b[2:4], "big")
        if L == len(b) and L > 38 and b[L - 18] == 80 and b[L - 17] == 18:
            out.append((b[:2] + (L - 1).to_bytes(2, "big") + b[4:L - 17] + b"\x11" + b[L - 16:], k, n, r))
    # the first 60 truncated at every length below Length, and with a buffer one short
    for b, k, n, r in base[:60]:
        L = int.from_bytes(b[2:4], "big")
        out += [(b[:m], k, n, r) for m in range(L)]
        out.append((b[:len(b) - 1], k, n, r))
    # seeded single-byte mutations of attribute type / len bytes and of the Length field
    rng = np.random.default_rng(0x5AD)
    for m in range(900):
        b, k, n, r = base[int(rng.integers(0, len(base)))]
        b = bytearray(b)
        L = int.from_bytes(b[2:4], "big")
        spots = [2, 3]
        i = 20
        while i + 2 <= min(L, len(b)) and b[i + 1] >= 2:
            spots += [i, i + 1]
            i += b[i + 1]
        at = spots[int(rng.integers(0, len(spots)))] if m % 3 else 3
        b[at] = int(rng.integers(0, 256)) if m % 5 else (b[at] + int(rng.integers(-2, 3))) & 0xFF
        out.append((bytes(b), k, n, r))
    if matrix:
        from tests.radius_matrix_util import full_two_byte_only
        out += list(matrix)
        out += [(full_two_byte_only(code), 1, 4, r) for code, r in ((4, 0), (2, 1), (99, 12))]
    return out


def test_parse_records_match_model_under_sanitizers(exe, matrix):
    recs = records(matrix[1])
    assert len(recs) > 5000 + len(matrix[1])
    assert sum(1 for b, _, _, _ in recs if len(b) == 4096) >= 280 + 3
    seen = set()
    for (b, k, n, r), got in zip(recs, walk(exe, recs)):
        want = model(b, k, n, r)
        assert len(got) == 16
        for g, w in zip(got, want):
            assert w is None or g == w, (b.hex(), k, n, r, got, want)
        seen.add((got[0], got[7], got[8], got[9], got[10]))
    # the cases reach every verdict the guard and the step plan can give
    assert {0, E, errno.EINVAL} <= {s[0] for s in seen}
    assert {0, errno.EINVAL, errno.EOVERFLOW} <= {s[1] for s in seen}
    assert {0, E, errno.EINVAL} <= {s[2] for s in seen}
    assert {0, errno.EINVAL} <= {s[3] for s in seen} and {0, errno.EINVAL} <= {s[4] for s in seen}


def test_matrix_verdicts_consistent_with_reference(exe, matrix):
    """No Python model: what the compiled walk decides without a hash must
    agree with what the reference returned for the same packet and request
    (radius_matrix.json; verify as built, untampered)."""
    cases, recs = matrix
    n_e1 = n_inval = n_ok = 0
    for c, rec, got in zip(cases, recs, walk(exe, recs)):
        err, sign, e1, e2, e3 = got[0], got[7], got[8], got[9], got[10]
        what = (c, got)
        assert err == 0, what
        assert sign == c["sign"], what
        if e1:
            assert c["verify"] == e1, what
            n_e1 += 1
        elif c["verify"] == errno.EINVAL:
            assert errno.EINVAL in (e2, e3), what
            n_inval += 1
        elif c["verify"] == 0:
            assert (e1, e2, e3) == (0, 0, 0), what
            n_ok += 1
    assert n_e1 > 100 and n_inval > 100 and 3 * n_ok >= len(cases)
