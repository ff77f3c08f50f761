"""Rebuild the packets of tests/golden/radius_matrix.json from a case's
parameters (code, layout, request, key).

The fixture holds parameters, result codes and hashes, not packets: the
generator (tests/golden/make_golden_radius_matrix.py) and the tests both build
the packets here.  Every seeded byte comes from oracle.pyoracle.gen_stream.

  codes     every code radius.h's switches name, their neighbours, unknowns
  requests  0 = no request, else a 20-byte header with that code: the matching
            family, a foreign family, Status-Server (for code 5) and a reply
            code in the request's place
  layouts   LAYOUTS below; every packet passes the structural guard of
            include/lcb_radius_gpu.h and its last byte is attribute data (or
            the authenticator), so XORing it with 0x40 leaves the structure
  keys      secrets of 1, 10, 64 and 100 bytes (MD5's block is 64)
"""
import errno

import numpy as np

from oracle.pyoracle import gen_stream

SEED = 0x7261646D61747278         # "radmatrx"
CODES = [0, 1, 2, 3, 4, 5, 6, 11, 12, 13, 14, 39, 40, 41, 42, 43, 44, 45, 46, 255]
REQUESTS = [0, 1, 4, 12, 40, 43, 2]
SECRET_LENS = [1, 10, 64, 100]
LAYOUTS = [
    "plain",              # no Message-Authenticator, no User-Password
    "ma_first",           # Message-Authenticator as the first attribute
    "ma_last",            # ... as the last attribute
    "two_ma",             # two of them; the second holds nonzero bytes that stay
    "pw16",               # User-Password of 16 bytes
    "pw128_ma",           # User-Password of 128 bytes in front of a Message-Authenticator
    "ma_pw_pw",           # Message-Authenticator, then two User-Passwords (the first is coded)
    "ma17",               # Message-Authenticator of length 17
    "badpw17_ma",         # User-Password of 17 data bytes, good Message-Authenticator
    "badpw20_ma17",       # User-Password of 20 data bytes, Message-Authenticator of length 17
    "full_two_byte",      # 4096 bytes: Message-Authenticator, 2020 two-byte attributes, User-Password
    "full_255",           # 4096 bytes: 255-byte attributes, 128-byte User-Password in the middle,
                          # Message-Authenticator last
    "minimal",            # exactly 20 bytes
]
FULL_LAYOUTS = ("full_two_byte", "full_255")
ZERO_AUTH = (4, 40, 43)
REQ_AUTH = (2, 3, 5, 11, 41, 42, 44, 45)   # radius_pkt_init copies the request's authenticator
TAMPER = 0x40                               # XORed into the packet's last byte


def secrets():
    return [gen_stream(SEED ^ (0xA000 + k), n).tobytes() for k, n in enumerate(SECRET_LENS)]


def cases():
    """Every (code, layout index, request code, key index), in fixture order."""
    out = []
    for li in range(len(LAYOUTS)):
        for code in CODES:
            for req in REQUESTS:
                out.append((code, li, req, len(out) % len(SECRET_LENS)))
    return out


class _Bytes:
    """Successive byte runs of one case's own stream."""

    def __init__(self, index):
        self.b = gen_stream(SEED ^ ((index + 1) << 20), 8192).tobytes()
        self.at = 0

    def take(self, n):
        self.at += n
        return self.b[self.at - n:self.at]


def _attr(t, data):
    return bytes([t, 2 + len(data)]) + data


def request_header(index, req):
    """The 20 bytes of case `index`'s request, None for req == 0."""
    if not req:
        return None
    return bytes([req, index & 0xFF, 0, 20]) + gen_stream(SEED ^ ((index + 1) << 20) ^ (1 << 12), 16).tobytes()


def build(index, case):
    """-> (unsigned packet, request header or None) of cases()[index]."""
    code, li, req, _ = case
    name = LAYOUTS[li]
    s = _Bytes(index)
    rq = request_header(index, req)
    seeded = s.take(16)
    if code in ZERO_AUTH:
        auth = bytes(16)
    elif code in REQ_AUTH and rq is not None:
        auth = rq[4:20]
    else:
        auth = seeded
    a = lambda t, n: _attr(t, s.take(n))                      # noqa: E731
    ma = lambda: _attr(80, bytes(16))                         # noqa: E731
    pw = lambda n: _attr(2, s.take(n))                        # noqa: E731
    if name == "plain":
        at = [a(1, 9), a(32, 13), a(26, 30)]
    elif name == "ma_first":
        at = [ma(), a(1, 5), a(4, 4)]
    elif name == "ma_last":
        at = [a(1, 11), a(31, 17), ma()]
    elif name == "two_ma":
        at = [a(1, 6), ma(), a(5, 4), _attr(80, bytes(x | 1 for x in s.take(16)))]
    elif name == "pw16":
        at = [a(1, 7), pw(16), a(6, 4)]
    elif name == "pw128_ma":
        at = [a(1, 3), pw(128), a(61, 4), ma()]
    elif name == "ma_pw_pw":
        at = [ma(), pw(16), a(1, 8), pw(16)]
    elif name == "ma17":
        at = [a(1, 10), _attr(80, bytes(15)), a(8, 4)]
    elif name == "badpw17_ma":
        at = [pw(17), a(1, 5), ma()]
    elif name == "badpw20_ma17":
        at = [a(1, 4), pw(20), _attr(80, bytes(15))]
    elif name == "full_two_byte":
        two = np.frombuffer(s.take(2020), np.uint8) % 70 + 3              # types 3..72
        at = [ma(), np.stack([two, np.full(2020, 2)], 1).astype(np.uint8).tobytes(), pw(16)]
    elif name == "full_255":
        at = [a(3 + k, 253) for k in range(8)] + [pw(128)] + [a(20 + k, 253) for k in range(7)] + [a(79, 101), ma()]
    else:
        at = []
    body = b"".join(at)
    pkt = bytes([code, index & 0xFF]) + (20 + len(body)).to_bytes(2, "big") + auth + body
    return pkt, rq


def full_two_byte_only(code=4):
    """The longest possible attribute list: 2038 two-byte attributes, 4096 bytes."""
    t = gen_stream(SEED ^ 0x2038, 2038) % 70 + 3
    body = np.stack([t, np.full(2038, 2)], 1).astype(np.uint8).tobytes()
    return bytes([code, 0]) + (4096).to_bytes(2, "big") + bytes(16) + body


def tampered(pkt):
    return pkt[:-1] + bytes([pkt[-1] ^ TAMPER])


def walk(pkt):
    """The structural guard of include/lcb_radius_gpu.h over a buffer that is
    exactly the packet: [(offset, type, len)] of every attribute, None where
    the guard refuses."""
    n = len(pkt)
    if n < 20:
        return None
    end = int.from_bytes(pkt[2:4], "big")
    if end < 20 or end > n or end > 4096:
        return None
    i, out = 20, []
    while i < end:
        if end - i < 2:
            return None
        t, ln = pkt[i], pkt[i + 1]
        if ln < 2 or t == 0 or ln > end - i:
            return None
        out.append((i, t, ln))
        i += ln
    return out


def conditions(rows):
    """What the generator and tests/test_radius_matrix.py both require of the
    reference's result codes; rows: (sign, verify, tampered) per case."""
    E, I, O = errno.EBADMSG, errno.EINVAL, errno.EOVERFLOW
    assert {r[0] for r in rows} == {0, E, O}
    assert {r[1] for r in rows} == {0, I, E}
    assert 3 * sum(1 for r in rows if r[1] == 0) >= len(rows)
    assert any(r[2] == 0 for r in rows)
    assert any(r[1] == 0 and r[2] == E for r in rows)


def load(path):
    """The fixture with its secrets as bytes and its cases as dicts carrying
    their index: code, layout, request, key, sign, verify, tampered (result
    codes) and signed_sha256, verified_sha256, tampered_sha256 (None: the
    reference left that call's input buffer as it was)."""
    import json
    fx = json.load(open(path))
    fx["secrets"] = [bytes.fromhex(s) for s in fx["secrets"]]
    fx["cases"] = [dict(zip(fx["columns"], row), index=i) for i, row in enumerate(fx["cases"])]
    return fx
