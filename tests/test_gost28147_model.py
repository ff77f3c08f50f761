"""tests/gost28147_model.py (the numpy restatement the GPU tests compare
against) reproduces every entry of the reference-generated fixture
tests/golden/gost28147.json, and the library's own sbox data and packed-table
construction agree with it."""
import hashlib
import json
import os

import numpy as np
import pytest

from tests import gost28147_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "gost28147.json")))


@pytest.fixture(scope="module")
def G():
    from liblcb_amd import gost28147
    return gost28147


def u8(h):
    return np.frombuffer(bytes.fromhex(h), np.uint8)


def test_fixture_shape(fx):
    assert [sum(1 for v in fx["kat_ecb"] if v["be"] == be) for be in (False, True)] == [12, 1]
    assert [sum(1 for v in fx["kat_mac"] if v["be"] == be) for be in (False, True)] == [2, 1]
    assert len(fx["packed_tables"]) == 6 and len(fx["ragged"]["batches"]) == 12


def test_model_reproduces_ecb_vectors(fx, G):
    for v in fx["kat_ecb"]:
        sb, key = G.sbox(v["sbox"]), bytes.fromhex(v["key"])
        plain, enc = u8(v["plain"]).reshape(-1, 8), u8(v["encrypted"]).reshape(-1, 8)
        assert np.array_equal(M.crypt_blocks(0, key, sb, plain, v["be"]), enc), v["name"]
        assert np.array_equal(M.crypt_blocks(1, key, sb, enc, v["be"]), plain), v["name"]


def test_model_reproduces_mac_vectors(fx, G):
    for v in fx["kat_mac"]:
        data = u8(v["plain"])
        got = M.mac_batch(bytes.fromhex(v["key"]), G.sbox(v["sbox"]), data, [0], [data.size], v["be"])
        assert got.tobytes().hex() == v["mac"], v["name"]


def test_library_sboxes_and_packed_tables_match_reference(fx, G):
    """lcb_gost28147_sbox / lcb_gost28147_gpu_table against the OR of the
    reference's four expanded tables, for all six parameter sets."""
    for sid, h in enumerate(fx["packed_tables"]):
        want = np.frombuffer(bytes.fromhex(h), "<u4")
        assert np.array_equal(G.packed_table(sid), want), sid
        assert np.array_equal(M.packed_table(G.sbox(sid)), want), sid
        t = M.tables(G.sbox(sid))
        assert np.array_equal(t[0] | t[1] | t[2] | t[3], want), sid
    with pytest.raises(ValueError):
        G.sbox(6)
    with pytest.raises(ValueError):
        G.sbox(-1)
    with pytest.raises(OSError):
        G.packed_table(bytes([16]) + bytes(127))  # an entry above 15


def test_model_reproduces_ragged_batches(fx, G):
    from oracle.pyoracle import gen_stream
    offs, lens = M.ragged(11, 300, 1200)
    src = gen_stream(fx["ragged"]["seed"], int((offs + lens).max()))
    # the layout covers what the GPU tests rely on it for
    assert (lens == 0).any() and ((lens >= 8) & (lens < 16)).any() and (lens % 8 != 0).any()
    assert set(int(o) % 16 for o in offs) == set(range(16))
    for b in fx["ragged"]["batches"]:
        sb, key = G.sbox(b["sbox"]), bytes.fromhex(b["key"])
        enc = M.crypt_batch(0, key, sb, src, offs, lens, b["be"])
        dec = M.crypt_batch(1, key, sb, src, offs, lens, b["be"])
        macs = M.mac_batch(key, sb, src, offs, lens, b["be"])
        assert hashlib.sha256(enc.tobytes()).hexdigest() == b["enc_sha256"], b["name"]
        assert hashlib.sha256(dec.tobytes()).hexdigest() == b["dec_sha256"], b["name"]
        assert hashlib.sha256(macs.tobytes()).hexdigest() == b["mac_sha256"], b["name"]
        if "first16_enc" in b:
            end = int(offs[15] + lens[15])
            assert enc[:end].tobytes().hex() == b["first16_enc"], b["name"]
            assert macs[:16].tobytes().hex() == b["first16_mac"], b["name"]
        # decrypt inverts encrypt on every whole block, tails stay zero
        back = M.crypt_batch(1, key, sb, enc, offs, lens, b["be"])
        want = M.crypt_batch(0, key, sb, dec, offs, lens, b["be"])
        assert np.array_equal(back, want)
        for o, n in zip(offs[:32], lens[:32]):
            o, n = int(o), int(n)
            assert np.array_equal(back[o:o + (n & ~7)], src[o:o + (n & ~7)])
            assert not back[o + (n & ~7):o + n].any()


def test_model_reproduces_big_batch(fx, G):
    from oracle.pyoracle import gen_stream
    b = fx["big"]
    src = gen_stream(b["seed"], b["count"] * b["stride"])
    h = hashlib.sha256()
    step = 1 << 22  # 4 MiB of whole blocks at a time
    for at in range(0, src.size, step):
        h.update(M.crypt_blocks(0, bytes.fromhex(b["key"]), G.sbox(b["sbox"]),
                                src[at:at + step].reshape(-1, 8), b["be"]).tobytes())
    assert h.hexdigest() == b["enc_sha256"]
