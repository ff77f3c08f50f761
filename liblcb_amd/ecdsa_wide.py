"""Host-side mirror of liblcb's include/crypto/dsa/ecdsa.h, batched, on the
six 384- and 512-bit prime-field curves of the reference's table (the
256-bit curves are liblcb_amd.ecdsa's).

verify_batch(curve, hashes, sigs, pub_keys) returns one int32 per item:
exactly what the reference's ecdsa_verify_be (le=False) or ecdsa_verify_le
(le=True) returns for (hash_i, hash_size, r_i, s_i, B, Qx, Qy, B), B =
curve_bytes(curve) = 48 or 64: 0 valid, -2 bad signature, -1 refused public
key or R at infinity, EINVAL for r or s out of range
(include/lcb_ecdsa_wide_gpu.h has the whole contract).  verify_messages()
digests the messages with hash_batch on the device and hands the digest
tensor straight to verify_batch.  torch CUDA tensors run in device mode on
torch's current stream without waiting; numpy / bytes run in host mode
through page-locked staging.  Every status is produced by the HIP kernels of
liblcb_ecdsa_wide_gpu.so; there is no CPU path.
"""
import ctypes
import os

import numpy as np
import torch

from ._lib import F_DEVICE, HERE, LcbHashError, c_sz, c_u32, c_vp, check, load_satellite
from .hash import _is_dev, hash_batch

__all__ = ["verify_batch", "verify_messages", "curve_id", "curve_params", "curve_bytes", "ecdsa_wide_lib", "CURVES",
           "ALGO_ECDSA", "ALGO_GOST", "ECDSA_WIDE_SIGNATURES"]

LIB_PATH = os.path.join(HERE, "liblcb_ecdsa_wide_gpu.so")

ALGO_ECDSA, ALGO_GOST = 0, 1
# Curve ids of lcb_ecdsa_wide_verify_batch, under the reference's names (ecdsa.h:96-739).
CURVES = ["secp384r1", "brainpoolP384r1", "brainpoolP512r1", "id-tc26-gost-3410-12-512-paramSetA",
          "id-tc26-gost-3410-12-512-paramSetB", "id-tc26-gost-3410-2012-512-paramSetTest"]
_BYTES = [48, 48, 64, 64, 64, 64]
MAX_HASH_SIZE = 128

_VERIFY = [c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_u32, c_vp]
# every symbol include/lcb_ecdsa_wide_gpu.h declares
ECDSA_WIDE_SIGNATURES = [
    ("lcb_ecdsa_wide_curve_count", ctypes.c_int, []),
    ("lcb_ecdsa_wide_curve_name", ctypes.c_char_p, [ctypes.c_int]),
    ("lcb_ecdsa_wide_curve_id", ctypes.c_int, [ctypes.c_char_p]),
    ("lcb_ecdsa_wide_curve_bytes", ctypes.c_int, [ctypes.c_int]),
    ("lcb_ecdsa_wide_curve_params", ctypes.c_int, [ctypes.c_int, c_vp, c_vp, c_vp]),
    ("lcb_ecdsa_wide_verify_batch", ctypes.c_int, [ctypes.c_int, ctypes.c_int] + _VERIFY),
    ("ecdsa_verify_be_wide_batch", ctypes.c_int, [ctypes.c_int] + _VERIFY),
    ("ecdsa_verify_le_wide_batch", ctypes.c_int, [ctypes.c_int] + _VERIFY),
]

_wlib = None


def ecdsa_wide_lib():
    """The loaded liblcb_ecdsa_wide_gpu.so (after liblcb_hash_gpu.so, which it
    links against); raises LcbHashError if it has not been built."""
    global _wlib
    if _wlib is None:
        _wlib = load_satellite(LIB_PATH, ECDSA_WIDE_SIGNATURES)
    return _wlib


def curve_id(name):
    """The id of the curve `name` (the reference's name), or `name` itself if
    it already is an id."""
    if isinstance(name, (int, np.integer)):
        if not 0 <= int(name) < len(CURVES):
            raise ValueError("unknown curve id %r" % (name,))
        return int(name)
    cid = ecdsa_wide_lib().lcb_ecdsa_wide_curve_id(str(name).encode())
    if cid < 0:
        raise ValueError("unknown curve %r" % (name,))
    return cid


def curve_bytes(curve):
    """B, the size of every number of the curve in bytes: 48 or 64."""
    return ecdsa_wide_lib().lcb_ecdsa_wide_curve_bytes(curve_id(curve))


def curve_params(curve):
    """{name, algo, h, bytes, p, a, b, Gx, Gy, n} of a curve, the numbers as ints."""
    cid = curve_id(curve)
    B = curve_bytes(cid)
    out = (ctypes.c_uint8 * (6 * B))()
    algo, h = c_u32(), c_u32()
    check(ecdsa_wide_lib().lcb_ecdsa_wide_curve_params(cid, out, ctypes.byref(algo), ctypes.byref(h)))
    raw = bytes(out)
    res = {"name": CURVES[cid], "algo": algo.value, "h": h.value, "bytes": B}
    for i, k in enumerate(("p", "a", "b", "Gx", "Gy", "n")):
        res[k] = int.from_bytes(raw[B * i:B * i + B], "big")
    return res


def _host_u8(a):
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(a), dtype=np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)


def verify_batch(curve, hashes, sigs, pub_keys, key_idx=None, le=False, hash_size=None, count=None, out=None):
    """One status per signature.  B = curve_bytes(curve).

    hashes    count x hash_size bytes (hash_size defaults to the row length of
              a 2-D array, else B); the first min(hash_size, B) bytes count
    sigs      count x 2 B bytes, r || s
    pub_keys  nkeys x 2 B bytes, x || y; without key_idx key i belongs to item i
    key_idx   int32/uint32 per item, or None; an index >= nkeys gives EINVAL
              for that item
    le        every number little-endian (ecdsa_verify_le), else big-endian
    returns   int32 (count,), same kind of memory as `hashes`
    """
    L = ecdsa_wide_lib()
    cid = curve_id(curve)
    B2 = 2 * _BYTES[cid]
    if hash_size is None:
        hash_size = int(hashes.shape[1]) if getattr(hashes, "ndim", 1) == 2 else B2 // 2
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
    if hash_size < 1 or hash_size > MAX_HASH_SIZE:
        raise LcbHashError(22, "liblcb_ecdsa_wide_gpu: invalid argument (hash_size %d)" % hash_size)
    if count is None:
        count = size(sigs) // B2
    count = int(count)
    nkeys = size(pub_keys) // B2
    if size(sigs) < B2 * count or size(hashes) < hash_size * count:
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
            check(L.lcb_ecdsa_wide_verify_batch(cid, 1 if le else 0, hashes.data_ptr(), hash_size, sigs.data_ptr(),
                                                pub_keys.data_ptr(), nkeys,
                                                key_idx.data_ptr() if key_idx is not None else None, count,
                                                out.data_ptr(), F_DEVICE, stream))
        return out[:count]
    if out is None:
        out = np.empty(count, dtype=np.int32)
    elif not isinstance(out, np.ndarray) or out.dtype != np.int32 or not out.flags.c_contiguous or out.size < count:
        raise TypeError("out must be a C-contiguous int32 numpy array of >= count entries")
    ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    check(L.lcb_ecdsa_wide_verify_batch(cid, 1 if le else 0, ptr(hashes), hash_size, ptr(sigs), ptr(pub_keys), nkeys,
                                        key_idx.ctypes.data if key_idx is not None else None, count,
                                        out.ctypes.data, 0, None))
    return out[:count]


def verify_messages(curve, alg, data, sigs, pub_keys, key_idx=None, *, offsets=None, lengths=None, count=None,
                    stride=None, fixed_len=None, le=False, out=None):
    """Digest every message with hash_batch(alg, ...) and verify its signature
    over the digest; the digests stay where `data` is (on the device for a
    CUDA tensor: the two calls are enqueued back to back on the current
    stream).  The natural pairs: SHA-384 with secp384r1 and SHA-512 with
    brainpoolP512r1 in the be form, GOST R 34.11-2012 512 with the tc26
    512-bit sets in the le form."""
    digests = hash_batch(alg, data, offsets=offsets, lengths=lengths, count=count, stride=stride,
                         fixed_len=fixed_len)
    n, D = int(digests.shape[0]), int(digests.shape[1])
    return verify_batch(curve, digests.reshape(-1), sigs, pub_keys, key_idx=key_idx, le=le, hash_size=D, count=n,
                        out=out)
