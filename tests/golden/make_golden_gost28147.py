#!/usr/bin/env python3
"""Generate tests/golden/gost28147.json (run ONLY where the reference exists).

Pure data fixtures for include/crypto/cipher/gost28147.h.  Every expected
output is produced by the reference itself, compiled from its sources through
tests/golden/ref_gost28147_shim.c into oracle/_ref/libref_gost28147.so
(git-ignored) after its own gost28147_self_test() returned 0.  Every reference
call is made on a 4-byte aligned copy, one buffer at a time: the aligned path
is the one the batch API reproduces (the reference's unaligned decrypt
branches use the other form's byte order).

kat_ecb / kat_mac
    The self test's vector tables (12 LE + 1 BE ECB, 2 LE + 1 BE MAC), decoded
    by the reference's own gost28147_import_le_hex.
packed_tables
    Per parameter-set id, the OR of the reference's four expanded tables
    (gost28147_init, gost28147.h:494-507): each carries one byte of the
    rotated word, so the OR is the packed table the kernels use.
ragged
    300 buffers of 0..1199 bytes packed back to back over the SURVEY.md 8d
    stream, every sbox id x LE/BE: SHA-256 of the encrypt output, of the
    decrypt output and of the 8-byte MACs; the first 16 buffers' encrypt
    output and MACs in full for two of the combinations.
big
    64 Ki x 1 KiB, SHA-256 of the encrypt output only.

The six sboxes themselves are not fixture material: the library carries its
own restatement of those public parameter sets, referred to here by id.

Usage:  python3 tests/golden/make_golden_gost28147.py [reference root]
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from oracle.pyoracle import SEED, gen_stream  # noqa: E402
from tests.gost28147_model import ragged  # noqa: E402

REF_SO = os.path.join(REPO, "oracle", "_ref", "libref_gost28147.so")
STREAM_SEED = SEED ^ 0x28147


def build_ref(ref_root):
    hdr = os.path.join(ref_root, "include", "crypto", "cipher", "gost28147.h")
    if not os.path.exists(hdr):
        raise SystemExit("%s is missing: this generator runs only where the reference exists" % hdr)
    os.makedirs(os.path.dirname(REF_SO), exist_ok=True)
    subprocess.check_call(["gcc", "-O2", "-w", "-fPIC", "-shared", "-DGOST28147_SELF_TEST",
                           "-I" + os.path.join(ref_root, "include"), "-o", REF_SO,
                           os.path.join(HERE, "ref_gost28147_shim.c")])
    return ctypes.CDLL(REF_SO)


class Ref:
    def __init__(self, L):
        self.L = L
        L.ref_gost28147_kat.restype = ctypes.c_long

    def crypt(self, op, be, key, sbox_id, src, offs, lens):
        """Aligned reference calls, one buffer at a time, into a zeroed flat array."""
        out = np.zeros(src.size, np.uint8)
        for o, n in zip(offs, lens):
            o, nb = int(o), int(n) >> 3
            buf = np.ascontiguousarray(src[o:o + 8 * nb])
            res = np.zeros(8 * nb + 8, np.uint8)
            assert self.L.ref_gost28147_crypt(op, be, key, sbox_id, buf.ctypes.data_as(ctypes.c_void_p),
                                              ctypes.c_size_t(nb), res.ctypes.data_as(ctypes.c_void_p)) == 0
            out[o:o + 8 * nb] = res[:8 * nb]
        return out

    def mac(self, be, key, sbox_id, src, offs, lens):
        out = np.zeros((len(offs), 8), np.uint8)
        for i, (o, n) in enumerate(zip(offs, lens)):
            o, nb = int(o), int(n) >> 3
            buf = np.ascontiguousarray(src[o:o + 8 * nb])
            m = np.zeros(8, np.uint8)
            assert self.L.ref_gost28147_mac(be, key, sbox_id, buf.ctypes.data_as(ctypes.c_void_p),
                                            ctypes.c_size_t(nb), m.ctypes.data_as(ctypes.c_void_p),
                                            ctypes.c_size_t(8)) == 0
            out[i] = m
        return out

    def kats(self, tbl):
        rows, idx = [], 0
        while True:
            key, plain, out = (ctypes.create_string_buffer(n) for n in (32, 2048, 2048))
            sid = ctypes.c_int(-1)
            n = self.L.ref_gost28147_kat(tbl, ctypes.c_size_t(idx), key, ctypes.byref(sid), plain, out)
            if n == -1:
                return rows
            assert n > 0 and sid.value >= 0, (tbl, idx, n)
            rows.append((idx, key.raw.hex(), sid.value, plain.raw[:n].hex(), out.raw))
            idx += 1


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    L = build_ref(ref_root)
    assert L.ref_gost28147_self_test() == 0, "the reference's gost28147_self_test() fails"
    ref = Ref(L)
    kat_ecb, kat_mac = [], []
    for tbl, be in ((0, False), (1, True)):
        for idx, key, sid, plain, out in ref.kats(tbl):
            kat_ecb.append({"name": "tst1v%s[%d]" % ("_be" if be else "", idx), "be": be, "sbox": sid, "key": key,
                            "plain": plain, "encrypted": out[:len(plain) // 2].hex()})
    for tbl, be in ((2, False), (3, True)):
        for idx, key, sid, plain, out in ref.kats(tbl):
            kat_mac.append({"name": "tst2v%s[%d]" % ("_be" if be else "", idx), "be": be, "sbox": sid, "key": key,
                            "plain": plain, "mac": out[:8].hex()})
    assert (len(kat_ecb), len(kat_mac)) == (13, 3), (len(kat_ecb), len(kat_mac))
    packed = []
    for sid in range(6):
        t = np.zeros((4, 256), np.uint32)
        assert L.ref_gost28147_tables(sid, t.ctypes.data_as(ctypes.c_void_p)) == 0
        packed.append((t[0] | t[1] | t[2] | t[3]).astype("<u4").tobytes().hex())
    n = 300
    offs, lens = ragged(11, n, 1200)
    total = int((offs + lens).max())
    src = gen_stream(STREAM_SEED, total)
    rng = np.random.default_rng(28147)
    rag = []
    for sid in range(6):
        for be in (False, True):
            key = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
            enc = ref.crypt(0, int(be), key, sid, src, offs, lens)
            dec = ref.crypt(1, int(be), key, sid, src, offs, lens)
            macs = ref.mac(int(be), key, sid, src, offs, lens)
            row = {"name": "ragged%d_s%d_%s" % (n, sid, "be" if be else "le"), "sbox": sid, "be": be,
                   "key": key.hex(), "enc_sha256": hashlib.sha256(enc.tobytes()).hexdigest(),
                   "dec_sha256": hashlib.sha256(dec.tobytes()).hexdigest(),
                   "mac_sha256": hashlib.sha256(macs.tobytes()).hexdigest()}
            if (sid, be) in ((1, False), (5, True)):
                end = int(offs[15] + lens[15])
                row["first16_enc"] = enc[:end].tobytes().hex()
                row["first16_mac"] = macs[:16].tobytes().hex()
            rag.append(row)
    cnt = 1 << 16
    bsrc = gen_stream(SEED, cnt * 1024)
    key = bytes(range(32))
    out = np.zeros(8 * 128 + 8, np.uint8)
    h = hashlib.sha256()
    for i in range(cnt):  # one aligned call per buffer
        assert L.ref_gost28147_crypt(0, 0, key, 5, bsrc[i * 1024:].ctypes.data_as(ctypes.c_void_p),
                                     ctypes.c_size_t(128), out.ctypes.data_as(ctypes.c_void_p)) == 0
        h.update(out[:1024].tobytes())
    big = {"name": "64k_x_1k_s5_le", "sbox": 5, "be": False, "key": key.hex(), "seed": SEED, "count": cnt,
           "stride": 1024, "enc_sha256": h.hexdigest()}
    json.dump({"source": "include/crypto/cipher/gost28147.h compiled from the reference (oracle/_ref), aligned calls",
               "kat_ecb": kat_ecb, "kat_mac": kat_mac, "packed_tables": packed,
               "ragged": {"seed": STREAM_SEED, "layout": "ragged(11, 300, 1200)", "batches": rag}, "big": big},
              open(os.path.join(HERE, "gost28147.json"), "w"), indent=0)
    print("gost28147.json: %d ecb + %d mac vectors, %d ragged batches" % (len(kat_ecb), len(kat_mac), len(rag)))


if __name__ == "__main__":
    main()
