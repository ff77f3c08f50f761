"""Host-side mirror of the signing half of liblcb's include/crypto/dsa/ecdsa.h,
batched, on the six 384- and 512-bit prime-field curves of liblcb_amd.ecdsa_wide
(the 256-bit curves are liblcb_amd.ecdsa_sign's).

B = ecdsa_wide.curve_bytes(curve) = 48 or 64 is the size of every number.
sign_batch(curve, hashes, priv_keys, rnd) returns (sigs, status): per item
exactly what the reference's ecdsa_sign_be (le=False) or ecdsa_sign_le
(le=True) returns and writes for (hash_i, hash_size, d, B, rnd_i, B); r || s
is zeros where the status is not 0 (include/lcb_ecdsa_wide_sign_gpu.h has the
whole contract).  key_gen_batch and pub_key_batch mirror ecdsa_key_gen_* and
ecdsa_recover_pub_key_from_priv_key_*; their public keys are what
ecdsa_wide.verify_batch takes.  sign_messages() digests the messages with
hash_batch on the device and hands the digest tensor straight to sign_batch.

`rnd` is the caller's: it must come from a cryptographic random generator and
must never repeat for a key.

torch CUDA tensors run in device mode on torch's current stream without
waiting (the first use of a curve on a device uploads its window table with a
blocking copy); numpy / bytes run in host mode through page-locked staging
that is zeroed afterwards.  Every output is produced by the HIP kernels of
liblcb_ecdsa_wide_sign_gpu.so; there is no CPU path.
"""
import ctypes
import os

import numpy as np
import torch

from ._lib import F_DEVICE, HERE, LcbHashError, c_sz, c_u32, c_vp, check, load_satellite
from .ecdsa_wide import _BYTES, MAX_HASH_SIZE, _host_u8, curve_id
from .hash import _is_dev, hash_batch

__all__ = ["sign_batch", "key_gen_batch", "pub_key_batch", "sign_messages", "ecdsa_wide_sign_lib",
           "ECDSA_WIDE_SIGN_SIGNATURES"]

LIB_PATH = os.path.join(HERE, "liblcb_ecdsa_wide_sign_gpu.so")

_SIGN = [c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_vp, c_u32, c_vp]
_KEYGEN = [c_vp, c_sz, c_vp, c_vp, c_vp, c_u32, c_vp]
_PUBKEY = [c_vp, c_sz, c_vp, c_vp, c_u32, c_vp]
_I = ctypes.c_int
# every symbol include/lcb_ecdsa_wide_sign_gpu.h declares
ECDSA_WIDE_SIGN_SIGNATURES = [
    ("lcb_ecdsa_wide_sign_batch", _I, [_I, _I] + _SIGN),
    ("lcb_ecdsa_wide_key_gen_batch", _I, [_I, _I] + _KEYGEN),
    ("lcb_ecdsa_wide_pub_key_batch", _I, [_I, _I] + _PUBKEY),
    ("ecdsa_sign_be_wide_batch", _I, [_I] + _SIGN),
    ("ecdsa_sign_le_wide_batch", _I, [_I] + _SIGN),
    ("ecdsa_key_gen_be_wide_batch", _I, [_I] + _KEYGEN),
    ("ecdsa_key_gen_le_wide_batch", _I, [_I] + _KEYGEN),
    ("ecdsa_recover_pub_key_from_priv_key_be_wide_batch", _I, [_I] + _PUBKEY),
    ("ecdsa_recover_pub_key_from_priv_key_le_wide_batch", _I, [_I] + _PUBKEY),
]

_wslib = None


def ecdsa_wide_sign_lib():
    """The loaded liblcb_ecdsa_wide_sign_gpu.so (after liblcb_hash_gpu.so, which
    it links against); raises LcbHashError if it has not been built."""
    global _wslib
    if _wslib is None:
        _wslib = load_satellite(LIB_PATH, ECDSA_WIDE_SIGN_SIGNATURES)
    return _wslib


def _same_device(dev, **tensors):
    for name, t in tensors.items():
        if not _is_dev(t) or t.device != dev or t.dtype != torch.uint8 or not t.is_contiguous():
            raise TypeError("%s must be a contiguous uint8 tensor on %s" % (name, dev))


def _ptr(a):
    return a.ctypes.data if a.size else None


def sign_batch(curve, hashes, priv_keys, rnd, key_idx=None, le=False, hash_size=None, count=None, out=None):
    """One signature and one status per item.  B = curve_bytes(curve).

    hashes     count x hash_size bytes (hash_size defaults to the row length
               of a 2-D array, else B); the first min(hash_size, B) count
    priv_keys  nkeys x B bytes; without key_idx key i belongs to item i
    rnd        count x B bytes, the nonces: from a CSPRNG, never repeated
    key_idx    int32/uint32 per item, or None; an index >= nkeys gives EINVAL
               for that item
    le         every number little-endian (ecdsa_sign_le), else big-endian
    out        (sigs, status) to write into: uint8 of >= 2 B count bytes and
               int32 of >= count entries, same kind of memory as `hashes`
    returns    (sigs uint8 (count, 2 B) r || s, status int32 (count,))
    """
    L = ecdsa_wide_sign_lib()
    cid = curve_id(curve)
    B = _BYTES[cid]
    if hash_size is None:
        hash_size = int(hashes.shape[1]) if getattr(hashes, "ndim", 1) == 2 else B
    hash_size = int(hash_size)
    dev = hashes.device if _is_dev(hashes) else None
    if dev is not None:
        _same_device(dev, hashes=hashes, priv_keys=priv_keys, rnd=rnd)
        size = lambda t: int(t.numel())  # noqa: E731
    else:
        hashes, priv_keys, rnd = _host_u8(hashes), _host_u8(priv_keys), _host_u8(rnd)
        size = lambda t: int(t.size)  # noqa: E731
    if hash_size < 1 or hash_size > MAX_HASH_SIZE:
        raise LcbHashError(22, "liblcb_ecdsa_wide_sign_gpu: invalid argument (hash_size %d)" % hash_size)
    if count is None:
        count = size(rnd) // B
    count = int(count)
    nkeys = size(priv_keys) // B
    if size(rnd) < B * count or size(hashes) < hash_size * count:
        raise ValueError("hashes / rnd hold fewer than %d items" % count)
    if key_idx is None:
        if nkeys < count:
            raise ValueError("priv_keys holds %d keys, count is %d" % (nkeys, count))
        nkeys = count
    elif dev is not None:
        if not _is_dev(key_idx) or key_idx.device != dev or key_idx.dtype not in (torch.int32, torch.uint32) or \
                not key_idx.is_contiguous() or int(key_idx.numel()) < count:
            raise TypeError("key_idx must be a contiguous int32 / uint32 tensor of >= count entries on %s" % dev)
    else:
        key_idx = np.ascontiguousarray(key_idx, dtype=np.uint32)
        if key_idx.size < count:
            raise ValueError("key_idx has %d entries, count is %d" % (key_idx.size, count))
    sigs, status = out if out is not None else (None, None)
    if dev is not None:
        if out is None:
            sigs = torch.empty(2 * B * count, dtype=torch.uint8, device=dev)
            status = torch.empty(count, dtype=torch.int32, device=dev)
        elif not _is_dev(sigs) or sigs.device != dev or sigs.dtype != torch.uint8 or not sigs.is_contiguous() or \
                int(sigs.numel()) < 2 * B * count or not _is_dev(status) or status.device != dev or \
                status.dtype != torch.int32 or not status.is_contiguous() or int(status.numel()) < count:
            raise TypeError("out must be (contiguous uint8 of >= 2 B count, contiguous int32 of >= count) on %s" % dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            check(L.lcb_ecdsa_wide_sign_batch(cid, 1 if le else 0, hashes.data_ptr(), hash_size,
                                              priv_keys.data_ptr(), nkeys,
                                              key_idx.data_ptr() if key_idx is not None else None, rnd.data_ptr(),
                                              count, sigs.data_ptr(), status.data_ptr(), F_DEVICE, stream))
        return sigs.reshape(-1)[:2 * B * count].reshape(count, 2 * B), status[:count]
    if out is None:
        sigs, status = np.empty(2 * B * count, np.uint8), np.empty(count, np.int32)
    elif not isinstance(sigs, np.ndarray) or sigs.dtype != np.uint8 or not sigs.flags.c_contiguous or \
            sigs.size < 2 * B * count or not isinstance(status, np.ndarray) or status.dtype != np.int32 or \
            not status.flags.c_contiguous or status.size < count:
        raise TypeError("out must be (C-contiguous uint8 of >= 2 B count, C-contiguous int32 of >= count) numpy "
                        "arrays")
    check(L.lcb_ecdsa_wide_sign_batch(cid, 1 if le else 0, _ptr(hashes), hash_size, _ptr(priv_keys), nkeys,
                                      key_idx.ctypes.data if key_idx is not None else None, _ptr(rnd), count,
                                      _ptr(sigs), _ptr(status), 0, None))
    return sigs.reshape(-1)[:2 * B * count].reshape(count, 2 * B), status[:count]


def _keys(gen, curve, src, le, count):
    L = ecdsa_wide_sign_lib()
    cid = curve_id(curve)
    B = _BYTES[cid]
    dev = src.device if _is_dev(src) else None
    if dev is not None:
        _same_device(dev, **{"rnd" if gen else "priv_keys": src})
        have = int(src.numel()) // B
    else:
        src = _host_u8(src)
        have = int(src.size) // B
    count = have if count is None else int(count)
    if have < count:
        raise ValueError("the input holds %d numbers, count is %d" % (have, count))
    if dev is not None:
        priv = torch.empty(B * count, dtype=torch.uint8, device=dev) if gen else None
        pub = torch.empty(2 * B * count, dtype=torch.uint8, device=dev)
        status = torch.empty(count, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            if gen:
                check(L.lcb_ecdsa_wide_key_gen_batch(cid, 1 if le else 0, src.data_ptr(), count, priv.data_ptr(),
                                                     pub.data_ptr(), status.data_ptr(), F_DEVICE, stream))
            else:
                check(L.lcb_ecdsa_wide_pub_key_batch(cid, 1 if le else 0, src.data_ptr(), count, pub.data_ptr(),
                                                     status.data_ptr(), F_DEVICE, stream))
    else:
        priv = np.empty(B * count, np.uint8) if gen else None
        pub, status = np.empty(2 * B * count, np.uint8), np.empty(count, np.int32)
        if gen:
            check(L.lcb_ecdsa_wide_key_gen_batch(cid, 1 if le else 0, _ptr(src), count, _ptr(priv), _ptr(pub),
                                                 _ptr(status), 0, None))
        else:
            check(L.lcb_ecdsa_wide_pub_key_batch(cid, 1 if le else 0, _ptr(src), count, _ptr(pub), _ptr(status), 0,
                                                 None))
    pub = pub.reshape(count, 2 * B)
    return (priv.reshape(count, B), pub, status) if gen else (pub, status)


def key_gen_batch(curve, rnd, le=False, count=None):
    """(priv_keys (count, B), pub_keys (count, 2 B) x || y, status (count,))
    from count x B random bytes: d = rnd below n, else (rnd mod (n - 1)) + 1;
    rnd = 0 gives -1 and zeros.  Same kind of memory as `rnd`."""
    return _keys(True, curve, rnd, le, count)


def pub_key_batch(curve, priv_keys, le=False, count=None):
    """(pub_keys (count, 2 B) x || y, status (count,)) of count x B bytes of
    private keys: EINVAL for d >= n, -1 for d = 0, zeros for both."""
    return _keys(False, curve, priv_keys, le, count)


def sign_messages(curve, alg, data, priv_keys, rnd, key_idx=None, *, offsets=None, lengths=None, count=None,
                  le=False):
    """Digest every message with hash_batch(alg, ...) and sign the digest; the
    digests stay where `data` is (on the device for a CUDA tensor: the two
    calls are enqueued back to back on the current stream).  The natural
    pairs are those of ecdsa_wide.verify_messages.  Returns (sigs, status)."""
    digests = hash_batch(alg, data, offsets=offsets, lengths=lengths, count=count)
    n, D = int(digests.shape[0]), int(digests.shape[1])
    return sign_batch(curve, digests.reshape(-1), priv_keys, rnd, key_idx=key_idx, le=le, hash_size=D, count=n)
