"""Host-side mirror of liblcb's include/crypto/dsa/ecdsa.h, batched:
ECDSA / GOST R 34.10 signature verification over the ten 256-bit prime-field
curves of the reference's table.

verify_batch(curve, hashes, sigs, pub_keys) returns one int32 per item:
exactly what the reference's ecdsa_verify_be (le=False) or ecdsa_verify_le
(le=True) returns for (hash_i, hash_size, r_i, s_i, 32, Qx, Qy, 32): 0 valid,
-2 bad signature, -1 refused public key or R at infinity, EINVAL for r or s
out of range (include/lcb_ecdsa_gpu.h has the whole contract).
verify_messages() digests the messages with hash_batch on the device and
hands the digest tensor straight to verify_batch.  torch CUDA tensors run in
device mode on torch's current stream without waiting; numpy / bytes run in
host mode through page-locked staging.  Every status is produced by the HIP
kernel of liblcb_ecdsa_gpu.so; there is no CPU path.
"""
import ctypes
import os

import numpy as np
import torch

from ._lib import F_DEVICE, HERE, LcbHashError, c_sz, c_u32, c_vp, check, load_satellite
from .hash import _is_dev, hash_batch

__all__ = ["verify_batch", "verify_messages", "curve_id", "curve_params", "ecdsa_lib", "CURVES", "ALGO_ECDSA",
           "ALGO_GOST", "ECDSA_SIGNATURES"]

LIB_PATH = os.path.join(HERE, "liblcb_ecdsa_gpu.so")

ALGO_ECDSA, ALGO_GOST = 0, 1
# Curve ids of lcb_ecdsa_verify_batch, under the reference's names (ecdsa.h:96-739).
CURVES = ["secp256k1", "secp256r1", "brainpoolP256r1", "id-GostR3410-2001-ParamSet-cc",
          "id-gostR3410-2001-Test_ParamSet", "id-gostR3410-2001-CryptoPro-A-ParamSet",
          "id-gostR3410-2001-CryptoPro-B-ParamSet", "id-gostR3410-2001-CryptoPro-C-ParamSet",
          "id-gostR3410-2001-CryptoPro-XchA-ParamSet", "id-gostR3410-2001-CryptoPro-XchB-ParamSet"]

_VERIFY = [c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_u32, c_vp]
# every symbol include/lcb_ecdsa_gpu.h declares
ECDSA_SIGNATURES = [
    ("lcb_ecdsa_curve_count", ctypes.c_int, []),
    ("lcb_ecdsa_curve_name", ctypes.c_char_p, [ctypes.c_int]),
    ("lcb_ecdsa_curve_id", ctypes.c_int, [ctypes.c_char_p]),
    ("lcb_ecdsa_curve_params", ctypes.c_int, [ctypes.c_int, c_vp, c_vp, c_vp]),
    ("lcb_ecdsa_verify_batch", ctypes.c_int, [ctypes.c_int, ctypes.c_int] + _VERIFY),
    ("ecdsa_verify_be_batch", ctypes.c_int, [ctypes.c_int] + _VERIFY),
    ("ecdsa_verify_le_batch", ctypes.c_int, [ctypes.c_int] + _VERIFY),
]

_elib = None


def ecdsa_lib():
    """The loaded liblcb_ecdsa_gpu.so (after liblcb_hash_gpu.so, which it
    links against); raises LcbHashError if it has not been built."""
    global _elib
    if _elib is None:
        _elib = load_satellite(LIB_PATH, ECDSA_SIGNATURES)
    return _elib


def curve_id(name):
    """The id of the curve `name` (the reference's name), or `name` itself if
    it already is an id."""
    if isinstance(name, (int, np.integer)):
        if not 0 <= int(name) < len(CURVES):
            raise ValueError("unknown curve id %r" % (name,))
        return int(name)
    cid = ecdsa_lib().lcb_ecdsa_curve_id(str(name).encode())
    if cid < 0:
        raise ValueError("unknown curve %r" % (name,))
    return cid


def curve_params(curve):
    """{name, algo, h, p, a, b, Gx, Gy, n} of a curve, the numbers as ints."""
    cid = curve_id(curve)
    out = (ctypes.c_uint8 * 192)()
    algo, h = c_u32(), c_u32()
    check(ecdsa_lib().lcb_ecdsa_curve_params(cid, out, ctypes.byref(algo), ctypes.byref(h)))
    raw = bytes(out)
    res = {"name": CURVES[cid], "algo": algo.value, "h": h.value}
    for i, k in enumerate(("p", "a", "b", "Gx", "Gy", "n")):
        res[k] = int.from_bytes(raw[32 * i:32 * i + 32], "big")
    return res


def _host_u8(a):
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(a), dtype=np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)


def verify_batch(curve, hashes, sigs, pub_keys, key_idx=None, le=False, hash_size=None, count=None, out=None):
    """One status per signature.

    hashes    count x hash_size bytes (hash_size defaults to the row length of
              a 2-D array, else 32); the first min(hash_size, 32) bytes count
    sigs      count x 64 bytes, r || s
    pub_keys  nkeys x 64 bytes, x || y; without key_idx key i belongs to item i
    key_idx   int32/uint32 per item, or None; an index >= nkeys gives EINVAL
              for that item
    le        every number little-endian (ecdsa_verify_le), else big-endian
    returns   int32 (count,), same kind of memory as `hashes`
    """
    L = ecdsa_lib()
    cid = curve_id(curve)
    if hash_size is None:
        hash_size = int(hashes.shape[1]) if getattr(hashes, "ndim", 1) == 2 else 32
    hash_size = int(hash_size)
    dev = hashes.device if _is_dev(hashes) else None
    if dev is not None:
        for name, t in (("hashes", hashes), ("sigs", sigs), ("pub_keys", pub_keys)):
            if not _is_dev(t) or t.device != dev or t.dtype != torch.uint8 or not t.is_contiguous():
                raise TypeError("%s must be a contiguous uint8 tensor on %s" % (name, dev))
        size = lambda t: int(t.numel())  # noqa: E731
    else:
        hashes, sigs, pub_keys = _host_u8(hashes), _host_u8(sigs), _host_u8(pub_keys)
        size = lambda t: int(t.size)  # noqa: E731
    if hash_size < 1 or hash_size > 64:
        raise LcbHashError(22, "liblcb_ecdsa_gpu: invalid argument (hash_size %d)" % hash_size)
    if count is None:
        count = size(sigs) // 64
    count = int(count)
    nkeys = size(pub_keys) // 64
    if size(sigs) < 64 * count or size(hashes) < hash_size * count:
        raise ValueError("hashes / sigs hold fewer than %d items" % count)
    if key_idx is None:
        if nkeys < count:
            raise ValueError("pub_keys holds %d keys, count is %d" % (nkeys, count))
        nkeys = count
    elif dev is not None:
        if not _is_dev(key_idx) or key_idx.device != dev or key_idx.dtype not in (torch.int32, torch.uint32) or \
                not key_idx.is_contiguous() or int(key_idx.numel()) < count:
            raise TypeError("key_idx must be a contiguous int32 / uint32 tensor of >= count entries on %s" % dev)
    else:
        key_idx = np.ascontiguousarray(key_idx, dtype=np.uint32)
        if key_idx.size < count:
            raise ValueError("key_idx has %d entries, count is %d" % (key_idx.size, count))
    if dev is not None:
        if out is None:
            out = torch.empty(count, dtype=torch.int32, device=dev)
        elif not _is_dev(out) or out.device != dev or out.dtype != torch.int32 or not out.is_contiguous() or \
                int(out.numel()) < count:
            raise TypeError("out must be a contiguous int32 tensor of >= count entries on %s" % dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            check(L.lcb_ecdsa_verify_batch(cid, 1 if le else 0, hashes.data_ptr(), hash_size, sigs.data_ptr(),
                                           pub_keys.data_ptr(), nkeys,
                                           key_idx.data_ptr() if key_idx is not None else None, count,
                                           out.data_ptr(), F_DEVICE, stream))
        return out[:count]
    if out is None:
        out = np.empty(count, dtype=np.int32)
    elif not isinstance(out, np.ndarray) or out.dtype != np.int32 or not out.flags.c_contiguous or out.size < count:
        raise TypeError("out must be a C-contiguous int32 numpy array of >= count entries")
    ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    check(L.lcb_ecdsa_verify_batch(cid, 1 if le else 0, ptr(hashes), hash_size, ptr(sigs), ptr(pub_keys), nkeys,
                                   key_idx.ctypes.data if key_idx is not None else None, count, out.ctypes.data, 0,
                                   None))
    return out[:count]


def verify_messages(curve, alg, data, sigs, pub_keys, key_idx=None, *, offsets=None, lengths=None, count=None,
                    stride=None, fixed_len=None, le=False, out=None):
    """Digest every message with hash_batch(alg, ...) and verify its signature
    over the digest; the digests stay where `data` is (on the device for a
    CUDA tensor: the two calls are enqueued back to back on the current
    stream).  The natural pairs: SHA-256 with secp256r1 / secp256k1 in the be
    form, GOST R 34.11-2012 256 with the GOST sets in the le form."""
    digests = hash_batch(alg, data, offsets=offsets, lengths=lengths, count=count, stride=stride,
                         fixed_len=fixed_len)
    n, D = int(digests.shape[0]), int(digests.shape[1])
    return verify_batch(curve, digests.reshape(-1), sigs, pub_keys, key_idx=key_idx, le=le, hash_size=D, count=n,
                        out=out)
