#!/usr/bin/env python3
"""Generate tests/golden/radius_matrix.json (run ONLY in the build container).

The REFERENCE's radius_pkt_sign and radius_pkt_verify (include/proto/radius.h,
through oracle/_ref/libref_radius.so: ref_rad_sign, ref_rad_verify_raw) over
the packet matrix of tests/radius_matrix_util.py: 20 codes x 13 attribute
layouts x 7 requests, four secrets in rotation.  ref_rad_verify_raw calls
radius_pkt_verify WITHOUT radius_pkt_chk, whose semantic rules would drop most
of these packets; every packet is first put through the structural walk of
radius_matrix_util.walk, so the reference's find loop stays in bounds.

Per case: ref_rad_sign of the built packet; ref_rad_verify_raw of the signed
packet (of the unsigned one where sign refused) with the case's request, as it
is and with its last byte XORed with 0x40.

Pure data: the secrets, and per case [code, layout, request, key, sign, verify,
tampered, signed_sha256, verified_sha256, tampered_sha256]: the parameters,
the three result codes, and SHA-256 of the buffer each call left, null where
the call left its input buffer byte for byte as it was (every refused sign,
and every verify that decoded no User-Password).

Result codes of the committed fixture (1820 cases):
  sign              0 / EBADMSG / EOVERFLOW     1400 / 140 / 280
  verify as built   0 / EINVAL / EBADMSG         865 / 206 / 749
  verify tampered   0 / EINVAL / EBADMSG          63 / 206 / 1551
(A first scratch run of 1680 cases, without the `minimal` layout, gave
1260 / 140 / 280, 775 / 156 / 749 and 42 tampered packets that verify; the 140
`minimal` cases add 140 / 0 / 0, 90 / 50 / 0 and 21.)

Usage:  python3 tests/golden/make_golden_radius_matrix.py   (needs `make -C oracle`)
"""
import ctypes
import errno
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from tests import radius_matrix_util as M  # noqa: E402

SO = os.path.join(REPO, "oracle", "_ref", "libref_radius.so")
MAX_BYTES = 256 << 10


def main():
    L = ctypes.CDLL(SO)
    u8p, sz = ctypes.c_char_p, ctypes.c_size_t
    L.ref_rad_verify_raw.argtypes = [u8p, sz, u8p, sz, u8p, ctypes.c_void_p]
    L.ref_rad_sign.argtypes = [u8p, sz, u8p, sz, ctypes.c_void_p, ctypes.POINTER(sz)]
    secrets = M.secrets()
    sha = lambda b: hashlib.sha256(b).hexdigest()  # noqa: E731

    def sign(pkt, key):
        assert M.walk(pkt) is not None
        out, ol = ctypes.create_string_buffer(4096), sz(0)
        rc = L.ref_rad_sign(pkt, len(pkt), key, len(key), out, ctypes.byref(ol))
        if rc:
            return rc, pkt          # ref_rad_sign copies nothing out for a refused packet
        assert ol.value == len(pkt)
        return 0, out.raw[:len(pkt)]

    def verify(pkt, key, req):
        assert M.walk(pkt) is not None
        out = ctypes.create_string_buffer(4096)
        rc = L.ref_rad_verify_raw(pkt, len(pkt), key, len(key), req, out)
        return rc, out.raw[:len(pkt)]

    rows = []
    for n, case in enumerate(M.cases()):
        code, li, req, k = case
        pkt, rq = M.build(n, case)
        if M.LAYOUTS[li] in M.FULL_LAYOUTS:
            assert len(pkt) == 4096
        key = secrets[k]
        rs, signed = sign(pkt, key)
        if rs:
            # Nothing in the matrix pairs a refused Message-Authenticator with a User-Password the
            # reference would already have encoded (include/lcb_radius_gpu.h, difference 1).
            pws = [a for a in M.walk(pkt) if a[1] == 2]
            assert not pws or rs in (errno.EINVAL, errno.EOVERFLOW)
        rv, out_v = verify(signed, key, rq)
        tam = M.tampered(signed)
        rt, out_t = verify(tam, key, rq)
        if rv:
            assert out_v == signed
        if rt:
            assert out_t == tam
        rows.append([code, li, req, k, rs, rv, rt, sha(signed) if signed != pkt else None,
                     sha(out_v) if out_v != signed else None, sha(out_t) if out_t != tam else None])
    M.conditions([r[4:7] for r in rows])

    path = os.path.join(HERE, "radius_matrix.json")
    dump = lambda x: json.dumps(x, separators=(",", ":"))  # noqa: E731
    with open(path, "w") as f:
        f.write('{"source": "reference radius_pkt_sign / radius_pkt_verify without radius_pkt_chk (oracle/ref_radius.c '
                'ref_rad_sign, ref_rad_verify_raw) on the packets of tests/radius_matrix_util.py",\n')
        f.write(' "secrets": %s,\n "codes": %s,\n "requests": %s,\n "layouts": %s,\n'
                % (dump([s.hex() for s in secrets]), dump(M.CODES), dump(M.REQUESTS), dump(M.LAYOUTS)))
        f.write(' "columns": ["code", "layout", "request", "key", "sign", "verify", "tampered", "signed_sha256", '
                '"verified_sha256", "tampered_sha256"],\n "cases": [\n')
        f.write(",\n".join("  " + dump(r) for r in rows))
        f.write("\n ]\n}\n")
    json.load(open(path))
    size = os.path.getsize(path)
    assert size < MAX_BYTES, size
    print("%s: %d cases, %d bytes" % (path, len(rows), size))
    for col, what in ((4, "sign"), (5, "verify as built"), (6, "verify tampered")):
        by = {}
        for r in rows:
            by[r[col]] = by.get(r[col], 0) + 1
        print("  %-16s %s" % (what, "  ".join("%s x %d" % (errno.errorcode.get(c, c), by[c]) for c in sorted(by))))


if __name__ == "__main__":
    main()
