#!/usr/bin/env python3
"""Generate tests/golden/stream.json (run ONLY where the reference exists).

Pure data fixtures for the streaming digests of include/lcb_hash_stream_gpu.h.
Every value is produced by the reference itself, compiled from its sources
through tests/golden/ref_stream_shim.c into oracle/_ref/libref_stream.so
(git-ignored).

For each of the 8 algorithms (block size B), and for HMAC-MD5 and HMAC-SHA-256
with a 10-byte key: the reference context's fields (the 344-byte record of
include/lcb_hash_stream_gpu.h: h, count, leftover bytes; N and Sigma for GOST)
after *_init (hmac_*_init) and *_update of each of these prefixes of the
SURVEY.md 8d byte stream:

    0, 1, B-1, B, B+1, 2B and 3B+5 bytes,

and the *_final digest of the whole 3B+5-byte message.

Usage:  python3 tests/golden/make_golden_stream.py [reference root]
"""
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from oracle.pyoracle import DSIZE, SEED, gen_stream  # noqa: E402

REF_SO = os.path.join(REPO, "oracle", "_ref", "libref_stream.so")
NAMES = {1: "md5", 2: "sha1", 3: "sha224", 4: "sha256", 5: "sha384", 6: "sha512", 7: "gost256", 8: "gost512"}
KEY = b"Jefe-lcb10"   # 10 bytes


def build_ref(ref_root):
    hdr = os.path.join(ref_root, "include", "crypto", "hash", "md5.h")
    if not os.path.exists(hdr):
        raise SystemExit("%s is missing: this generator runs only where the reference exists" % hdr)
    os.makedirs(os.path.dirname(REF_SO), exist_ok=True)
    subprocess.check_call(["gcc", "-O2", "-w", "-fPIC", "-shared", "-fno-strict-aliasing",
                           "-I" + os.path.join(ref_root, "include"), "-o", REF_SO,
                           os.path.join(HERE, "ref_stream_shim.c")])
    return ctypes.CDLL(REF_SO)


def prefixes(B):
    return [0, 1, B - 1, B, B + 1, 2 * B, 3 * B + 5]


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    L = build_ref(ref_root)
    args = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
            ctypes.c_char_p]
    L.ref_stream_record.argtypes = args
    L.ref_stream_digest.argtypes = args
    cases = []
    for alg, key in [(a, None) for a in range(1, 9)] + [(1, KEY), (4, KEY)]:
        B = 128 if alg in (5, 6) else 64
        msg = gen_stream(SEED, 3 * B + 5).tobytes()
        keyed = int(key is not None)
        recs = []
        for n in prefixes(B):
            out = ctypes.create_string_buffer(344)
            assert L.ref_stream_record(alg, keyed, key or b"", len(key or b""), msg, n, out) == 0
            recs.append({"prefix": n, "record": out.raw.hex()})
        dig = ctypes.create_string_buffer(64)
        assert L.ref_stream_digest(alg, keyed, key or b"", len(key or b""), msg, len(msg), dig) == 0
        cases.append({"alg": alg, "name": ("hmac_" if keyed else "") + NAMES[alg], "block": B,
                      "key": key.hex() if key is not None else None, "length": len(msg),
                      "records": recs, "digest": dig.raw[:DSIZE[alg]].hex()})
    json.dump({"source": "include/crypto/hash/*.h compiled from the reference (oracle/_ref/libref_stream.so)",
               "seed": SEED, "record": "lcb_hash_stream_state_t, 344 bytes, little-endian", "cases": cases},
              open(os.path.join(HERE, "stream.json"), "w"), indent=0)
    print("stream.json: %d cases x %d prefixes" % (len(cases), len(prefixes(64))))


if __name__ == "__main__":
    main()
