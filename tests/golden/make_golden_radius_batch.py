#!/usr/bin/env python3
"""Generate tests/golden/radius_batch.json (run ONLY in the build container).

Error codes and output buffers of the REFERENCE's radius_pkt_verify /
radius_pkt_sign (include/proto/radius.h, through oracle/_ref/libref_radius.so:
ref_rad_verify, ref_rad_sign) for tampered and mismatched packets, for the
batched sign/verify of include/lcb_radius_gpu.h to reproduce.  For every third
packet of tests/golden/radius.json:

  msg_authr      one flipped byte in the Message-Authenticator data
  authenticator  one flipped byte in the authenticator
  attribute      one flipped byte in another attribute's data
  password       one flipped byte in the encoded User-Password
  no_request     a reply verified with req == NULL
  other_request  a reply verified with another packet's request
  wrong_secret   verified under the next secret of the table
  sign_other     the unsigned packet signed under the next secret

ref_rad_verify runs radius_pkt_chk first, and its semantic rejections are not
the batch API's contract.  radius_pkt_chk reads only the code, the Length and
every attribute's type and len byte; a case is kept only if its unmodified
packet passes ref_rad_verify (so radius_pkt_chk) and the flipped byte is
attribute DATA or the authenticator, so radius_pkt_chk passes for it too.

Pure data, kept small: a case is six integers, [kind, base, flip, key, req,
rc]: the index into `kinds`; the packet of radius.json it starts from (its
`signed` form, `pre` for sign_other); the byte that is XORed with 0x40 (-1:
none); the secret's index; the packet of radius.json whose `request` is passed
(-1: NULL); the reference's result.  `diffs` holds, for the few cases where the
reference changed the buffer, the changed byte runs as [offset, hex].

Usage:  python3 tests/golden/make_golden_radius_batch.py   (needs `make -C oracle`)
"""
import ctypes
import errno
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SO = os.path.join(REPO, "oracle", "_ref", "libref_radius.so")


def attrs(pkt):
    """(offset, type, len) of every attribute."""
    end, i, out = int.from_bytes(pkt[2:4], "big"), 20, []
    while i + 2 <= end:
        out.append((i, pkt[i], pkt[i + 1]))
        i += pkt[i + 1]
    return out


def main():
    L = ctypes.CDLL(SO)
    u8p, sz = ctypes.c_char_p, ctypes.c_size_t
    L.ref_rad_verify.argtypes = [u8p, sz, u8p, sz, u8p, ctypes.c_void_p]
    L.ref_rad_sign.argtypes = [u8p, sz, u8p, sz, ctypes.c_void_p, ctypes.POINTER(sz)]
    fx = json.load(open(os.path.join(HERE, "radius.json")))
    secrets = [bytes.fromhex(s) for s in fx["secrets"]]
    P = fx["packets"]

    def verify(pkt, key, req):
        out = ctypes.create_string_buffer(4096)
        rc = L.ref_rad_verify(pkt, len(pkt), secrets[key], len(secrets[key]), req, out)
        return rc, out.raw[:len(pkt)]

    KINDS = ["authenticator", "msg_authr", "attribute", "password", "no_request", "other_request", "wrong_secret",
             "sign_other"]
    reply_idx = [i for i, p in enumerate(P) if p["kind"] == "reply"]
    cases, diffs = [], {}

    def add(what, base, flip_at, key, req_of, rc, out, pkt):
        if rc:
            assert out == pkt, what      # the reference leaves a refused packet alone
        if out != pkt:
            runs, i = [], 0
            while i < len(pkt):
                if out[i] != pkt[i]:
                    j = i
                    while j < len(pkt) and out[j] != pkt[j]:
                        j += 1
                    runs.append([i, out[i:j].hex()])
                    i = j
                else:
                    i += 1
            diffs[str(len(cases))] = runs
        cases.append([KINDS.index(what), base, flip_at, key, req_of, rc])

    def flip(pkt, at):
        b = bytearray(pkt)
        b[at] ^= 0x40
        return bytes(b)

    picked = 0
    for n, p in enumerate(P):
        if n % 3:
            continue
        picked += 1
        pkt, key = bytes.fromhex(p["signed"]), p["key"]
        req = bytes.fromhex(p["request"]) if p["kind"] == "reply" else None
        own = n if req is not None else -1
        rc, out = verify(pkt, key, req)
        assert rc == 0 and out.hex() == p["verified"]    # radius_pkt_chk passes
        A = attrs(pkt)
        ma = [a for a in A if a[1] == 80]
        pw = [a for a in A if a[1] == 2]
        other = [a for a in A if a[1] not in (2, 80) and a[2] > 2]
        flips = [("authenticator", 4 + n % 16)]
        if ma:
            flips.append(("msg_authr", ma[0][0] + 2 + n % 16))
        if other:
            a = other[n % len(other)]
            flips.append(("attribute", a[0] + 2 + n % (a[2] - 2)))
        if pw:
            flips.append(("password", pw[0][0] + 2 + n % (pw[0][2] - 2)))
        for what, at in flips:
            assert at >= 4 and (at < 20 or any(o + 2 <= at < o + ln for o, _, ln in A))   # data, not structure
            m = flip(pkt, at)
            add(what, n, at, key, own, *verify(m, key, req), m)
        if req is not None:
            add("no_request", n, -1, key, -1, *verify(pkt, key, None), pkt)
            m2 = reply_idx[(n * 7 + 1) % len(reply_idx)]
            o = bytes.fromhex(P[m2]["request"])
            if o[4:20] != req[4:20]:
                add("other_request", n, -1, key, m2, *verify(pkt, key, o), pkt)
        k2 = (key + 1) % len(secrets)
        add("wrong_secret", n, -1, k2, own, *verify(pkt, k2, req), pkt)
        if n % 12 == 0:
            pre = bytes.fromhex(p["pre"])
            out, ol = ctypes.create_string_buffer(4096), sz(0)
            rc = L.ref_rad_sign(pre, len(pre), secrets[k2], len(secrets[k2]), out, ctypes.byref(ol))
            assert rc == 0 and ol.value == len(pre)
            add("sign_other", n, -1, k2, -1, rc, out.raw[:len(pre)], pre)

    codes = {c[5] for c in cases}
    assert picked >= 150 and len(cases) >= 100, (picked, len(cases))
    assert {0, errno.EBADMSG, errno.EINVAL} <= codes, codes
    assert {c[0] for c in cases} == set(range(len(KINDS)))
    path = os.path.join(HERE, "radius_batch.json")
    row = lambda xs: ", ".join(json.dumps(x, separators=(",", ":")) for x in xs)  # noqa: E731
    with open(path, "w") as f:
        f.write('{"source": "reference radius_pkt_verify / radius_pkt_sign (oracle/ref_radius.c ref_rad_verify, '
                'ref_rad_sign) on packets of radius.json",\n')
        f.write(' "kinds": %s,\n "columns": ["kind", "base", "flip", "key", "req", "rc"],\n "cases": [\n'
                % json.dumps(KINDS))
        f.write(",\n".join("  " + row(cases[i:i + 5]) for i in range(0, len(cases), 5)))
        f.write('\n ],\n "diffs": {\n')
        f.write(",\n".join('  "%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in diffs.items()))
        f.write("\n }\n}\n")
    json.load(open(path))
    by = {}
    for c in cases:
        by[(KINDS[c[0]], c[5])] = by.get((KINDS[c[0]], c[5]), 0) + 1
    print("%s: %d cases (%d with a changed buffer) from %d packets, %d bytes" % (path, len(cases), len(diffs), picked,
                                                                                 os.path.getsize(path)))
    for k in sorted(by):
        print("  %-14s rc %-3d x %d" % (k[0], k[1], by[k]))


if __name__ == "__main__":
    main()
