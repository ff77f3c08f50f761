"""Host-side mirror of liblcb's include/crypto/cipher/gost28147.h, batched:
GOST 28147-89 ECB encrypt / decrypt and the MAC (imitovstavka).

encrypt_batch(key, src, sbox=...) returns dst where buffer i holds exactly
what the reference's gost28147_init[_be] + gost28147_blocks_encrypt[_be]
write for blocks_count = len_i // 8 on aligned memory (gost28147.h:336-407);
decrypt_batch the same for gost28147_blocks_decrypt[_be]; mac_batch returns
count x mac_size bytes, what gost28147_blocks_mac[_be] + gost28147_final[_be]
leave (gost28147.h:288-333, 534-566).  Buffer description as liblcb_amd.hash
(offsets/lengths or stride/fixed_len).  torch CUDA tensors run in device mode
on torch's current stream; numpy / bytes run in host mode through page-locked
staging.  Every byte is produced by the HIP kernels of
liblcb_gost28147_gpu.so; there is no CPU path.
"""
import ctypes
import os

import numpy as np
import torch

from ._lib import F_DEVICE, HERE, c_sz, c_u32, c_u64, c_vp, check, load_satellite
from .hash import _check_extent, _is_dev, _layout

__all__ = ["encrypt_batch", "decrypt_batch", "mac_batch", "sbox", "packed_table", "gost28147_lib",
           "SBOX_TEST", "SBOX_CRYPTOPRO_A", "SBOX_CRYPTOPRO_B", "SBOX_CRYPTOPRO_C", "SBOX_CRYPTOPRO_D",
           "SBOX_TC26_Z", "SBOX_NAMES", "GOST28147_SIGNATURES"]

LIB_PATH = os.path.join(HERE, "liblcb_gost28147_gpu.so")

# Parameter-set ids of lcb_gost28147_sbox (gost28147.h:74-139).
SBOX_TEST, SBOX_CRYPTOPRO_A, SBOX_CRYPTOPRO_B, SBOX_CRYPTOPRO_C, SBOX_CRYPTOPRO_D, SBOX_TC26_Z = range(6)
SBOX_NAMES = {SBOX_TEST: "id-GostR3411-94-TestParamSet", SBOX_CRYPTOPRO_A: "id-Gost28147-89-CryptoPro-A-ParamSet",
              SBOX_CRYPTOPRO_B: "id-Gost28147-89-CryptoPro-B-ParamSet",
              SBOX_CRYPTOPRO_C: "id-Gost28147-89-CryptoPro-C-ParamSet",
              SBOX_CRYPTOPRO_D: "id-Gost28147-89-CryptoPro-D-ParamSet", SBOX_TC26_Z: "id-tc26-gost-28147-param-Z"}

_ECB = [c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_u64, c_u32, c_u32, c_vp]
_MAC = [c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_sz, c_u64, c_u32, c_vp, c_sz, c_u32, c_vp]
# every symbol include/lcb_gost28147_gpu.h declares
GOST28147_SIGNATURES = [
    ("lcb_gost28147_crypt_batch", ctypes.c_int, [ctypes.c_int, ctypes.c_int] + _ECB),
    ("lcb_gost28147_mac_batch", ctypes.c_int, [ctypes.c_int] + _MAC),
    ("gost28147_blocks_encrypt_batch", ctypes.c_int, _ECB),
    ("gost28147_blocks_encrypt_be_batch", ctypes.c_int, _ECB),
    ("gost28147_blocks_decrypt_batch", ctypes.c_int, _ECB),
    ("gost28147_blocks_decrypt_be_batch", ctypes.c_int, _ECB),
    ("gost28147_blocks_mac_batch", ctypes.c_int, _MAC),
    ("gost28147_blocks_mac_be_batch", ctypes.c_int, _MAC),
    ("lcb_gost28147_sbox", c_vp, [ctypes.c_int]),
    ("lcb_gost28147_gpu_table", ctypes.c_int, [c_vp, c_vp]),
    ("lcb_gost28147_gpu_copy_probe", ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, c_u64, c_u32, c_u32, c_vp]),
]

_glib = None


def gost28147_lib():
    """The loaded liblcb_gost28147_gpu.so (after liblcb_hash_gpu.so, which it
    links against); raises LcbHashError if it has not been built."""
    global _glib
    if _glib is None:
        _glib = load_satellite(LIB_PATH, GOST28147_SIGNATURES)
    return _glib


def sbox(sbox_id):
    """The 128 bytes of parameter set `sbox_id` (SBOX_* constants)."""
    p = gost28147_lib().lcb_gost28147_sbox(int(sbox_id))
    if not p:
        raise ValueError("unknown GOST 28147-89 parameter set %r" % (sbox_id,))
    return ctypes.string_at(p, 128)


def packed_table(sb):
    """The 256-word packed table the kernels use for `sb` (id or 128 bytes)."""
    out = np.zeros(256, np.uint32)
    check(gost28147_lib().lcb_gost28147_gpu_table(_sbox_buf(sb), out.ctypes.data))
    return out


def _sbox_buf(sb):
    if isinstance(sb, (int, np.integer)):
        sb = sbox(sb)
    sb = bytes(sb)
    if len(sb) != 128:
        raise ValueError("sbox must be a parameter-set id or 128 bytes")
    return (ctypes.c_uint8 * 128).from_buffer_copy(sb)


def _key_buf(key):
    key = bytes(key)
    if len(key) != 32:
        raise ValueError("GOST 28147-89 takes a 32-byte key")
    return (ctypes.c_uint8 * 32).from_buffer_copy(key)


def _host_u8(a):
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(a), dtype=np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8)


def _describe(ref, offsets, lengths, count, stride, fixed_len):
    """(dev, total, count, stride, fixed_len, offsets, lengths) with the
    description checked against the buffer."""
    dev = ref.device if _is_dev(ref) else None
    total = ref.numel() if dev is not None else ref.size
    if dev is not None:
        for t, dt in ((offsets, (torch.int64, torch.uint64)), (lengths, (torch.int32, torch.uint32))):
            if t is not None:
                assert _is_dev(t) and t.dtype in dt and t.is_contiguous() and t.device == dev
    else:
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if lengths is not None:
            lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    count, stride, fixed_len = _layout(count, offsets, lengths, stride, fixed_len, total)
    _check_extent(total, count, offsets, lengths, stride, fixed_len)
    return dev, total, count, stride, fixed_len, offsets, lengths


def _ptr(t):
    if t is None:
        return None
    return t.data_ptr() if isinstance(t, torch.Tensor) else t.ctypes.data


def _crypt(op, key, src, sb, be, dst, offsets, lengths, count, stride, fixed_len):
    L = gost28147_lib()
    kbuf, sbuf = _key_buf(key), _sbox_buf(sb)
    if not _is_dev(src):
        src = _host_u8(src)
    else:
        assert src.dtype == torch.uint8 and src.is_contiguous()
    dev, total, count, stride, fixed_len, offsets, lengths = _describe(src, offsets, lengths, count, stride,
                                                                        fixed_len)
    if dev is not None:  # device mode
        if dst is None:
            dst = torch.zeros(max(total, 1), dtype=torch.uint8, device=dev)
        assert _is_dev(dst) and dst.dtype == torch.uint8 and dst.is_contiguous() and dst.device == dev
        _check_extent(dst.numel(), count, offsets, lengths, stride, fixed_len)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            check(L.lcb_gost28147_crypt_batch(op, 1 if be else 0, kbuf, 32, sbuf, _ptr(src), _ptr(dst),
                                              _ptr(offsets), _ptr(lengths), count, stride, fixed_len, F_DEVICE,
                                              stream))
        return dst
    if dst is None:
        dst = np.zeros(max(total, 1), dtype=np.uint8)
    assert isinstance(dst, np.ndarray) and dst.dtype == np.uint8 and dst.flags.c_contiguous
    _check_extent(dst.size, count, offsets, lengths, stride, fixed_len)
    check(L.lcb_gost28147_crypt_batch(op, 1 if be else 0, kbuf, 32, sbuf, src.ctypes.data if src.size else None,
                                      dst.ctypes.data, _ptr(offsets), _ptr(lengths), count, stride, fixed_len, 0,
                                      None))
    return dst


def encrypt_batch(key, src, *, sbox, be=False, dst=None, offsets=None, lengths=None, count=None, stride=None,
                  fixed_len=None):
    """Batched gost28147_blocks_encrypt (be: gost28147_init_be +
    gost28147_blocks_encrypt_be).  key: 32 bytes; sbox: an SBOX_* id or 128
    bytes; dst may be src (in place).  Returns dst."""
    return _crypt(0, key, src, sbox, be, dst, offsets, lengths, count, stride, fixed_len)


def decrypt_batch(key, src, *, sbox, be=False, dst=None, offsets=None, lengths=None, count=None, stride=None,
                  fixed_len=None):
    """Batched gost28147_blocks_decrypt[_be]: the inverse of encrypt_batch at
    every byte offset (the reference's aligned path)."""
    return _crypt(1, key, src, sbox, be, dst, offsets, lengths, count, stride, fixed_len)


def mac_batch(key, data, *, sbox, be=False, mac_size=8, out=None, offsets=None, lengths=None, count=None,
              stride=None, fixed_len=None):
    """Batched gost28147_blocks_mac[_be] + gost28147_final[_be]: returns
    (count, mac_size) bytes, mac_size 1..8."""
    L = gost28147_lib()
    kbuf, sbuf = _key_buf(key), _sbox_buf(sbox)
    if not _is_dev(data):
        data = _host_u8(data)
    else:
        assert data.dtype == torch.uint8 and data.is_contiguous()
    dev, total, count, stride, fixed_len, offsets, lengths = _describe(data, offsets, lengths, count, stride,
                                                                        fixed_len)
    mac_size = int(mac_size)
    rows = max(count, 1) * max(mac_size, 1)
    if dev is not None:
        if out is None:
            out = torch.zeros(rows, dtype=torch.uint8, device=dev)
        assert _is_dev(out) and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= rows
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            check(L.lcb_gost28147_mac_batch(1 if be else 0, kbuf, 32, sbuf, _ptr(data), _ptr(offsets),
                                            _ptr(lengths), count, stride, fixed_len, _ptr(out), mac_size,
                                            F_DEVICE, stream))
        return out[:count * mac_size].view(count, mac_size)
    if out is None:
        out = np.zeros(rows, dtype=np.uint8)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.size >= rows
    check(L.lcb_gost28147_mac_batch(1 if be else 0, kbuf, 32, sbuf, data.ctypes.data if data.size else None,
                                    _ptr(offsets), _ptr(lengths), count, stride, fixed_len, out.ctypes.data,
                                    mac_size, 0, None))
    return out.reshape(-1)[:count * mac_size].reshape(count, mac_size)
