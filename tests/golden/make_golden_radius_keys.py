#!/usr/bin/env python3
"""Generate tests/golden/radius_keys.json (run ONLY in the build container).

RADIUS packets built, signed and verified by the REFERENCE's own packet code
(include/proto/radius.h compiled into oracle/_ref/libref_radius.so by
oracle/Makefile; wrapper oracle/ref_radius.c), as make_golden_radius.py does,
but with shared secrets whose lengths sit on MD5's block and padding
boundaries:

  1, 39, 40, 47, 48, 49, 55, 56, 63, 64, 65, 103, 104, 111, 112, 128, 200

The User-Password chain hashes MD5(secret || 16 bytes): 39/40 put its 0x80
terminator and bit length in the first block or push the length into a second
one (55/56 bytes hashed), 47/48/49 end the data at 63/64/65 bytes, 103/104/
111/112/128 repeat that one block later, 55..65 and 128 are the same edges of
the secret itself (HMAC key of one block exactly, one more, and the key-prefix
mid-state after one or two whole blocks), 200 is longer than three blocks.
radius_pkt_sign of the reference refused NONE of these lengths (it has no
limit on key_len: radius.h:1487-1532); a refused length would be dropped and
reported by this script.

Per secret: an Access-Request with a User-Password of 1, 16, 17 and 128 bytes,
each with and without a Message-Authenticator; an Accounting-Request; and one
reply to each of the nine.  Every packet keeps `pre`, `signed`, `verified`,
for replies `request`, for passwords `password`, as radius.json does.  Pure
data: packet bytes as hex.  306 packets, about 170 KB: the 128-byte passwords
are kept four times over (pre, signed, verified and the reply's request), so
the packets are otherwise as small as radius_pkt_chk allows (a 1..3-byte
User-Name, at most one 3-byte attribute in a reply).

Usage:  python3 tests/golden/make_golden_radius_keys.py   (needs `make -C oracle`)
"""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_radius import SO, lib  # noqa: E402

LENGTHS = (1, 39, 40, 47, 48, 49, 55, 56, 63, 64, 65, 103, 104, 111, 112, 128, 200)
PASSWORDS = (1, 16, 17, 128)
REPLY_TO = {1: (2, 3, 11), 4: (5,)}


def main():
    if not os.path.exists(SO):
        sys.exit("oracle/_ref/libref_radius.so missing: make -C oracle (needs the reference sources)")
    L = lib()
    rng = np.random.default_rng(2866)
    pre = ctypes.create_string_buffer(4096)
    out = ctypes.create_string_buffer(4096)
    chk = ctypes.create_string_buffer(4096)
    pl, ol = ctypes.c_size_t(), ctypes.c_size_t()
    secrets, packets, refused = [], [], []
    for n in LENGTHS:
        key = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        mine = []
        shapes = [(1, pw, ma) for pw in PASSWORDS for ma in (0, 1)] + [(4, None, 0)]
        for j, (code, pwn, add_ma) in enumerate(shapes):
            auth = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
            pwd = rng.integers(0x21, 0x7F, pwn, dtype=np.uint8).tobytes() if pwn else None
            un = int(rng.integers(1, 4))
            t = bytes([1, un]) + rng.integers(0x61, 0x7B, un, dtype=np.uint8).tobytes()
            rc = L.ref_rad_request(code, int(rng.integers(0, 256)), auth, pwd, len(pwd) if pwd else 0, t, len(t),
                                   key, n, add_ma, pre, ctypes.byref(pl), out, ctypes.byref(ol))
            if rc != 0:
                refused.append((n, "request", code, rc))
                break
            req_pre, req = pre.raw[:pl.value], out.raw[:ol.value]
            vr = L.ref_rad_verify(req, len(req), key, n, None, chk)
            assert vr == 0, (n, code, vr)
            mine.append({"kind": "request", "code": code, "key": len(secrets), "msg_authr": add_ma,
                         "password": pwd.hex() if pwd else None, "pre": req_pre.hex(), "signed": req.hex(),
                         "verified": chk.raw[:len(req)].hex()})
            rcode = REPLY_TO[code][j % len(REPLY_TO[code])]
            rma = (j // 2 + j) % 2
            t = b"" if j % 3 else bytes([18, 3]) + rng.integers(0x20, 0x7F, 3, dtype=np.uint8).tobytes()
            rc = L.ref_rad_reply(rcode, req, t, len(t), key, n, rma, pre, ctypes.byref(pl), out, ctypes.byref(ol))
            if rc != 0:
                refused.append((n, "reply", rcode, rc))
                break
            rep = out.raw[:ol.value]
            vr = L.ref_rad_verify(rep, len(rep), key, n, req, chk)
            assert vr == 0, (n, rcode, vr)
            mine.append({"kind": "reply", "code": rcode, "key": len(secrets), "msg_authr": rma, "request": req.hex(),
                         "pre": pre.raw[:pl.value].hex(), "signed": rep.hex(), "verified": chk.raw[:len(rep)].hex()})
        else:
            secrets.append(key)
            packets += mine
    path = os.path.join(HERE, "radius_keys.json")
    json.dump({"source": "reference include/proto/radius.h compiled from the reference tree (oracle/ref_radius.c)",
               "secret_lengths": [len(s) for s in secrets], "secrets": [s.hex() for s in secrets],
               "packets": packets}, open(path, "w"), indent=0)
    print("radius_keys.json: %d secrets, %d packets (%d replies), %d bytes; refused by the reference: %s"
          % (len(secrets), len(packets), sum(p["kind"] == "reply" for p in packets), os.path.getsize(path),
             refused or "none"))


if __name__ == "__main__":
    main()
