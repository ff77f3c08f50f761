"""Batched GOST 28147-89 on the MI355X (include/lcb_gost28147_gpu.h) against
the reference-generated fixture tests/golden/gost28147.json and the numpy
model tests/gost28147_model.py (itself pinned to that fixture on the CPU).

Shapes are the smallest at which the kernels can go wrong: every byte offset
mod 16, buffers of zero / one block, len % 8 tails, an odd block count (the
last lane pair half full), a partial last wave, more tiles than waves (the
grid-stride step of fixed and ragged layouts), and MAC counts around the
64-buffer wave tile."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from tests import gost28147_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5


@pytest.fixture(scope="module")
def fx():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "gost28147.json")))


@pytest.fixture(scope="module")
def G(gpu):
    from liblcb_amd import gost28147
    gost28147.gost28147_lib()
    return gost28147


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


@pytest.fixture(scope="module")
def rag(fx):
    """The fixture's ragged layout, its source stream, the mask of the bytes
    that belong to whole blocks, and one guarded device copy."""
    from oracle.pyoracle import gen_stream
    offs, lens = M.ragged(11, 300, 1200)
    total = int((offs + lens).max())
    src = gen_stream(fx["ragged"]["seed"], total)
    mask = np.zeros(total + 64, bool)
    for o, n in zip(offs, lens):
        mask[int(o):int(o) + (int(n) & ~7)] = True
    return {"offs": offs, "lens": lens, "total": total, "src": src, "mask": mask}


def dev(torch, a, dtype=None):
    a = np.ascontiguousarray(a)
    return torch.as_tensor(a if dtype is None else a.astype(dtype), device="cuda:0")


def u8(h):
    return np.frombuffer(bytes.fromhex(h), np.uint8).copy()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_kats_through_all_six_wrappers(G, fx, torch_):
    torch = torch_
    L = G.gost28147_lib()
    stream = torch.cuda.current_stream().cuda_stream
    ecb = {(0, False): L.gost28147_blocks_encrypt_batch, (0, True): L.gost28147_blocks_encrypt_be_batch,
           (1, False): L.gost28147_blocks_decrypt_batch, (1, True): L.gost28147_blocks_decrypt_be_batch}
    mac = {False: L.gost28147_blocks_mac_batch, True: L.gost28147_blocks_mac_be_batch}
    seen = set()
    for v in fx["kat_ecb"]:
        key, sb = u8(v["key"]), np.frombuffer(G.sbox(v["sbox"]), np.uint8).copy()
        for op, src, want in ((0, v["plain"], v["encrypted"]), (1, v["encrypted"], v["plain"])):
            s, d = dev(torch, u8(src)), torch.full((len(src) // 2 + 8,), GUARD, dtype=torch.uint8, device="cuda:0")
            rc = ecb[(op, v["be"])](key.ctypes.data, 32, sb.ctypes.data, s.data_ptr(), d.data_ptr(), None, None,
                                    1, 0, s.numel(), 1, stream)
            assert rc == 0
            torch.cuda.synchronize()
            got = d.cpu().numpy()
            assert got[:s.numel()].tobytes().hex() == want, (v["name"], op)
            assert (got[s.numel():] == GUARD).all()
            seen.add((op, v["be"]))
    for v in fx["kat_mac"]:
        key, sb = u8(v["key"]), np.frombuffer(G.sbox(v["sbox"]), np.uint8).copy()
        s, m = dev(torch, u8(v["plain"])), torch.full((16,), GUARD, dtype=torch.uint8, device="cuda:0")
        rc = mac[v["be"]](key.ctypes.data, 256, sb.ctypes.data, s.data_ptr(), None, None, 1, 0, s.numel(),
                          m.data_ptr(), 8, 1, stream)
        assert rc == 0
        torch.cuda.synchronize()
        got = m.cpu().numpy()
        assert got[:8].tobytes().hex() == v["mac"], v["name"]
        assert (got[8:] == GUARD).all()
        seen.add(("mac", v["be"]))
    assert len(seen) == 6


@pytest.mark.parametrize("be", [False, True])
@pytest.mark.parametrize("sid", [1, 5])
def test_ragged_fixture_batches(G, fx, rag, torch_, sid, be):
    """300 buffers, 0..1199 bytes, back to back (every offset mod 16, zero and
    one block, tails): encrypt, decrypt and MAC hashes of the reference; no
    byte outside the whole blocks changes."""
    torch = torch_
    b = next(x for x in fx["ragged"]["batches"] if x["sbox"] == sid and x["be"] == be)
    key = bytes.fromhex(b["key"])
    src = dev(torch, np.concatenate([rag["src"], np.full(64, 0x3C, np.uint8)]))
    offs, lens = dev(torch, rag["offs"], np.int64), dev(torch, rag["lens"], np.int32)
    for fn, want in ((G.encrypt_batch, b["enc_sha256"]), (G.decrypt_batch, b["dec_sha256"])):
        dst = torch.full((rag["total"] + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
        fn(key, src, sbox=sid, be=be, dst=dst, offsets=offs, lengths=lens)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert (got[~rag["mask"]] == GUARD).all(), "a byte outside the whole blocks was written"
        got[~rag["mask"]] = 0
        assert sha(got[:rag["total"]]) == want, b["name"]
        if fn is G.encrypt_batch and "first16_enc" in b:
            end = int(rag["offs"][15] + rag["lens"][15])
            assert got[:end].tobytes().hex() == b["first16_enc"]
    macs = G.mac_batch(key, src, sbox=sid, be=be, offsets=offs, lengths=lens)
    torch.cuda.synchronize()
    assert sha(macs.cpu().numpy()) == b["mac_sha256"], b["name"]
    assert (src.cpu().numpy()[:rag["total"]] == rag["src"]).all()


@pytest.fixture(scope="module")
def dense():
    """257 x 4104 B: 513 blocks per buffer (odd: the last lane pair is half
    full, the last wave partial); the model's output, computed once."""
    from oracle.pyoracle import gen_stream
    n, ln = 257, 4104
    key, sid = bytes(range(7, 39)), 3
    src = gen_stream(0xD15E, n * ln).reshape(n, ln)
    from liblcb_amd import gost28147
    sb = gost28147.sbox(sid)
    out = {(op, be): M.crypt_blocks(op, key, sb, src.reshape(-1, 8), be).reshape(n, ln)
           for op in (0, 1) for be in (False, True)}
    return {"n": n, "len": ln, "key": key, "sid": sid, "src": src, "out": out}


@pytest.mark.parametrize("stride,base", [(4104, 0), (4112, 0), (4104, 4), (4112, 4), (4104, 1)])
def test_dense_fixed_stride(G, dense, torch_, stride, base):
    torch = torch_
    n, ln = dense["n"], dense["len"]
    host = np.full(base + n * stride + 32, GUARD, np.uint8)
    rows = np.lib.stride_tricks.as_strided(host[base:], (n, ln), (stride, 1))
    rows[:] = dense["src"]
    buf = dev(torch, host)
    for op, fn in ((0, G.encrypt_batch), (1, G.decrypt_batch)):
        for be in (False, True):
            dst = torch.full_like(buf, GUARD)
            fn(dense["key"], buf[base:], sbox=dense["sid"], be=be, dst=dst[base:], count=n, stride=stride,
               fixed_len=ln)
            torch.cuda.synchronize()
            got = dst.cpu().numpy()
            grows = np.lib.stride_tricks.as_strided(got[base:], (n, ln), (stride, 1))
            assert np.array_equal(grows, dense["out"][(op, be)]), (op, be)
            grows[:] = GUARD  # everything else is untouched
            assert (got == GUARD).all(), (op, be)


def test_in_place(G, dense, rag, torch_):
    torch = torch_
    n, ln = dense["n"], dense["len"]
    buf = dev(torch, dense["src"].reshape(-1))
    out = G.encrypt_batch(dense["key"], buf, sbox=dense["sid"], dst=buf, count=n, stride=ln, fixed_len=ln)
    assert out is buf
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().reshape(n, ln), dense["out"][(0, False)])
    G.decrypt_batch(dense["key"], buf, sbox=dense["sid"], dst=buf, count=n, stride=ln, fixed_len=ln)
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().reshape(n, ln), dense["src"])
    # ragged, misaligned, in place: neighbours share edge dwords
    key, sb = bytes(range(32)), G.sbox(2)
    r = dev(torch, rag["src"])
    offs, lens = dev(torch, rag["offs"], np.int64), dev(torch, rag["lens"], np.int32)
    G.encrypt_batch(key, r, sbox=2, be=True, dst=r, offsets=offs, lengths=lens)
    torch.cuda.synchronize()
    want = M.crypt_batch(0, key, sb, rag["src"], rag["offs"], rag["lens"], True, dst=rag["src"].copy())
    assert np.array_equal(r.cpu().numpy(), want)


def test_more_tiles_than_waves(G, fx, torch_):
    """Fixed layouts step buffer / pair indices per grid pass: 64 Ki x 64 B
    (one pass) and the fixture's 64 Ki x 1 KiB (8 tiles per wave)."""
    torch = torch_
    from oracle.pyoracle import gen_stream
    b = fx["big"]
    key, sb = bytes.fromhex(b["key"]), G.sbox(b["sbox"])
    host = gen_stream(b["seed"], b["count"] * b["stride"])
    src = dev(torch, host)
    out = G.encrypt_batch(key, src, sbox=b["sbox"], count=b["count"], stride=b["stride"], fixed_len=b["stride"])
    torch.cuda.synchronize()
    assert sha(out.cpu().numpy()) == b["enc_sha256"]
    back = G.decrypt_batch(key, out, sbox=b["sbox"], count=b["count"], stride=b["stride"], fixed_len=b["stride"])
    torch.cuda.synchronize()
    assert torch.equal(back, src)
    small = host[:65536 * 64]
    got = G.encrypt_batch(key, src[:small.size], sbox=b["sbox"], be=True, count=65536, stride=64, fixed_len=64)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy().reshape(-1, 8), M.crypt_blocks(0, key, sb, small.reshape(-1, 8), True))


def test_ragged_more_tiles_than_waves(G, torch_):
    """A ragged batch of more 1 KiB tiles than the launch has waves."""
    torch = torch_
    from oracle.pyoracle import gen_stream
    offs, lens = M.ragged(5, 24000, 1200)
    total = int((offs + lens).max())
    assert total > 12 << 20  # > 2 x 5 x 256 CUs x 4 waves of 1 KiB tiles
    host = gen_stream(0x7A66, total)
    key, sb = bytes(range(100, 132)), G.sbox(4)
    dst = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda:0")
    G.decrypt_batch(key, dev(torch, host), sbox=4, dst=dst, offsets=dev(torch, offs, np.int64),
                    lengths=dev(torch, lens, np.int32))
    torch.cuda.synchronize()
    want = M.crypt_batch(1, key, sb, host, offs, lens, False, dst=np.full(total, GUARD, np.uint8))
    assert np.array_equal(dst.cpu().numpy(), want)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 4097])
def test_mac_counts_and_sizes(G, torch_, count):
    torch = torch_
    from oracle.pyoracle import gen_stream
    offs, lens = M.ragged(count, count, 400)
    lens[0] = 0 if count > 1 else 24
    if count > 2:
        lens[count // 2] = 7  # no whole block
    total = int((offs + lens).max()) + 8
    host = gen_stream(0x3AC + count, total)
    key, sb = bytes(range(200, 232)), G.sbox(count % 6)
    data, doffs, dlens = dev(torch, host), dev(torch, offs, np.int64), dev(torch, lens, np.int32)
    for be in (False, True):
        want = M.mac_batch(key, sb, host, offs, lens, be)
        for mac_size in (1, 4, 8):
            out = torch.full((count * mac_size + 8,), GUARD, dtype=torch.uint8, device="cuda:0")
            got = G.mac_batch(key, data, sbox=count % 6, be=be, mac_size=mac_size, out=out, offsets=doffs,
                              lengths=dlens)
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy(), want[:, :mac_size]), (be, mac_size)
            assert (out.cpu().numpy()[count * mac_size:] == GUARD).all()
        if count > 1:
            assert not want[0].any()  # zero blocks: the initial state
    # fixed stride, 24-byte buffers 4 bytes off a 16-byte boundary
    n = min(count, 65)
    got = G.mac_batch(key, data[4:], sbox=count % 6, count=n, stride=0, fixed_len=24)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), M.mac_batch(key, sb, host[4:], [0] * n, [24] * n))


def test_host_mode(G, fx, rag, monkeypatch):
    b = next(x for x in fx["ragged"]["batches"] if x["sbox"] == 5 and x["be"])
    key = bytes.fromhex(b["key"])

    def run():
        for fn, want in ((G.encrypt_batch, b["enc_sha256"]), (G.decrypt_batch, b["dec_sha256"])):
            dst = np.full(rag["total"] + 64, GUARD, np.uint8)
            fn(key, rag["src"], sbox=5, be=True, dst=dst, offsets=rag["offs"], lengths=rag["lens"])
            assert (dst[~rag["mask"]] == GUARD).all()
            dst[~rag["mask"]] = 0
            assert sha(dst[:rag["total"]]) == want
        macs = G.mac_batch(key, rag["src"], sbox=5, be=True, offsets=rag["offs"], lengths=rag["lens"])
        assert sha(macs) == b["mac_sha256"]

    run()
    # the same batch forced across many staging chunk boundaries
    monkeypatch.setenv("LCB_GOST28147_CHUNK_BYTES", "8192")
    run()
    # fixed stride from host memory, in place, with a gap between buffers
    src = rag["src"][:64 * 200].copy()
    want = M.crypt_batch(0, key, G.sbox(5), src, np.arange(64) * 200, [160] * 64, True, dst=src.copy())
    G.encrypt_batch(key, src, sbox=5, be=True, dst=src, count=64, stride=200, fixed_len=160)
    assert np.array_equal(src, want)


def test_device_mode_key_and_sbox_reusable_after_the_call(G, fx, rag, torch_):
    """Device mode only enqueues; the caller may overwrite key and sbox the
    moment the call returns."""
    torch = torch_
    L = G.gost28147_lib()
    b = next(x for x in fx["ragged"]["batches"] if x["sbox"] == 1 and not x["be"])
    key, sb = u8(b["key"]), np.frombuffer(G.sbox(1), np.uint8).copy()
    src = dev(torch, rag["src"])
    offs, lens = dev(torch, rag["offs"], np.int64), dev(torch, rag["lens"], np.int32)
    dst = torch.zeros(rag["total"], dtype=torch.uint8, device="cuda:0")
    macs = torch.zeros(300 * 8, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    big = torch.empty(1 << 28, dtype=torch.uint8, device="cuda:0")
    with torch.cuda.stream(s):
        for _ in range(8):
            big.fill_(1)  # keeps the stream busy while the calls below return
        assert L.lcb_gost28147_crypt_batch(0, 0, key.ctypes.data, 32, sb.ctypes.data, src.data_ptr(),
                                           dst.data_ptr(), offs.data_ptr(), lens.data_ptr(), 300, 0, 0, 1,
                                           s.cuda_stream) == 0
        assert L.lcb_gost28147_mac_batch(0, key.ctypes.data, 32, sb.ctypes.data, src.data_ptr(), offs.data_ptr(),
                                         lens.data_ptr(), 300, 0, 0, macs.data_ptr(), 8, 1, s.cuda_stream) == 0
    key[:] = 0xFF
    sb[:] = 0
    s.synchronize()
    assert sha(dst.cpu().numpy()) == b["enc_sha256"]
    assert sha(macs.cpu().numpy()) == b["mac_sha256"]
