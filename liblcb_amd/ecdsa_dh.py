"""Host-side mirror of the key agreement of liblcb's
include/crypto/dsa/ecdsa.h, batched: ECDH over the ten 256-bit prime-field
curves of liblcb_amd.ecdsa.

dh_batch(curve, pub_keys, priv_keys) returns (shared, status): per item
exactly what the reference's ecdsa_dh_be (le=False) or ecdsa_dh_le (le=True)
returns and writes for (use_cofactor, Qx, Qy, 32, d, 32), the 32 bytes of the
x coordinate of d Q; zeros where the status is not 0
(include/lcb_ecdsa_dh_gpu.h has the whole contract).  dh_digest() hashes each
secret with hash_batch on the same stream, the usual "digest the shared x into
a session key" step without a host round trip.

torch CUDA tensors run in device mode on torch's current stream without
waiting; numpy / bytes run in host mode through page-locked staging that is
zeroed afterwards.  Every output is produced by the HIP kernel of
liblcb_ecdsa_dh_gpu.so; there is no CPU path.

Not offered: compressed / packed key forms, key import / export, key recovery
from a signature, private key verification, curves of other sizes, and any
key derivation beyond one digest.
"""
import numpy as np
import torch

from . import _lib
from ._lib import ECDSA_DH_SIGNATURES, F_DEVICE, check, ecdsa_dh_lib
from .ecdsa import _host_u8, curve_id
from .hash import _is_dev, hash_batch

__all__ = ["dh_batch", "dh_digest", "ecdsa_dh_lib", "ECDSA_DH_SIGNATURES", "LIB_PATH"]

LIB_PATH = _lib.ECDSA_DH_LIB_PATH


def _index(name, idx, dev):
    """(index array or None, its length): int32 / uint32, where the keys are."""
    if idx is None:
        return None, None
    if dev is not None:
        if not _is_dev(idx) or idx.device != dev or idx.dtype not in (torch.int32, torch.uint32) or \
                not idx.is_contiguous():
            raise TypeError("%s must be a contiguous int32 / uint32 tensor on %s" % (name, dev))
        return idx, int(idx.numel())
    idx = np.ascontiguousarray(idx).reshape(-1)
    if idx.dtype != np.uint32:
        idx = idx.view(np.uint32) if idx.dtype == np.int32 else idx.astype(np.uint32)
    return idx, int(idx.size)


def dh_batch(curve, pub_keys, priv_keys, le=False, use_cofactor=False, pub_idx=None, priv_idx=None, count=None,
             out=None):
    """One shared secret and one status per item.

    pub_keys   npub x 64 bytes, x || y; without pub_idx key i belongs to item i
    priv_keys  npriv x 32 bytes; without priv_idx key i belongs to item i.  One
               private key against many peers: one row and a priv_idx of zeros
    le         every number little-endian (ecdsa_dh_le), else big-endian
    use_cofactor  accepted as the reference accepts it; every curve here has
               cofactor 1, so both values give the same bytes
    pub_idx, priv_idx  int32/uint32 per item, or None; an index past its table
               gives EINVAL and zeros for that item
    count      defaults to the length of an index array, else to the number of
               keys; without an index the table may hold more than count keys
    out        (shared, status) to write into: uint8 of >= 32 count bytes and
               int32 of >= count entries, same kind of memory as `pub_keys`
    returns    (shared uint8 (count, 32), status int32 (count,)): 0 secret
               written; -1 public key refused (not below p, not on the curve)
               or d = 0; EINVAL d >= n or an index past its table
    """
    L = ecdsa_dh_lib()
    cid = curve_id(curve)
    dev = pub_keys.device if _is_dev(pub_keys) else None
    if dev is not None:
        for name, t in (("pub_keys", pub_keys), ("priv_keys", priv_keys)):
            if not _is_dev(t) or t.device != dev or t.dtype != torch.uint8 or not t.is_contiguous():
                raise TypeError("%s must be a contiguous uint8 tensor on %s" % (name, dev))
        npub, npriv = int(pub_keys.numel()) // 64, int(priv_keys.numel()) // 32
    else:
        pub_keys, priv_keys = _host_u8(pub_keys), _host_u8(priv_keys)
        npub, npriv = int(pub_keys.size) // 64, int(priv_keys.size) // 32
    pub_idx, n_pi = _index("pub_idx", pub_idx, dev)
    priv_idx, n_di = _index("priv_idx", priv_idx, dev)
    if count is None:
        count = n_pi if n_pi is not None else n_di if n_di is not None else min(npub, npriv)
    count = int(count)
    for what, have in (("pub_idx", n_pi), ("priv_idx", n_di), ("pub_keys", None if pub_idx is not None else npub),
                       ("priv_keys", None if priv_idx is not None else npriv)):
        if have is not None and have < count:
            raise ValueError("%s holds %d entries, count is %d" % (what, have, count))
    if pub_idx is None:
        npub = count
    if priv_idx is None:
        npriv = count
    shared, status = out if out is not None else (None, None)
    head = (cid, 1 if le else 0, 1 if use_cofactor else 0)
    if dev is not None:
        if out is None:
            shared = torch.empty(32 * count, dtype=torch.uint8, device=dev)
            status = torch.empty(count, dtype=torch.int32, device=dev)
        elif not _is_dev(shared) or shared.device != dev or shared.dtype != torch.uint8 or \
                not shared.is_contiguous() or int(shared.numel()) < 32 * count or not _is_dev(status) or \
                status.device != dev or status.dtype != torch.int32 or not status.is_contiguous() or \
                int(status.numel()) < count:
            raise TypeError("out must be (contiguous uint8 of >= 32 count, contiguous int32 of >= count) on %s" % dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            check(L.lcb_ecdsa_dh_batch(*head, pub_keys.data_ptr(), npub,
                                       pub_idx.data_ptr() if pub_idx is not None else None, priv_keys.data_ptr(),
                                       npriv, priv_idx.data_ptr() if priv_idx is not None else None, count,
                                       shared.data_ptr(), status.data_ptr(), F_DEVICE, stream))
        return shared.reshape(-1)[:32 * count].reshape(count, 32), status[:count]
    if out is None:
        shared, status = np.empty(32 * count, np.uint8), np.empty(count, np.int32)
    elif not isinstance(shared, np.ndarray) or shared.dtype != np.uint8 or not shared.flags.c_contiguous or \
            shared.size < 32 * count or not isinstance(status, np.ndarray) or status.dtype != np.int32 or \
            not status.flags.c_contiguous or status.size < count:
        raise TypeError("out must be (C-contiguous uint8 of >= 32 count, C-contiguous int32 of >= count) numpy arrays")
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    check(L.lcb_ecdsa_dh_batch(*head, ptr(pub_keys), npub, ptr(pub_idx), ptr(priv_keys), npriv, ptr(priv_idx), count,
                               ptr(shared), ptr(status), 0, None))
    return shared.reshape(-1)[:32 * count].reshape(count, 32), status[:count]


def dh_digest(alg, curve, pub_keys, priv_keys, le=False, use_cofactor=False, pub_idx=None, priv_idx=None,
              count=None, key=None):
    """dh_batch, then hash_batch(alg) of each 32-byte secret (HMAC where `key`
    is given); the secrets stay where the keys are (on the device for CUDA
    tensors: the two calls are enqueued back to back on the current stream).

    Returns (digests (count, digest size), status (count,)).  An item whose
    status is not 0 has a secret of 32 zero bytes and its digest is the digest
    of those zeros, not a session key: check the status beside every digest.
    """
    shared, status = dh_batch(curve, pub_keys, priv_keys, le=le, use_cofactor=use_cofactor, pub_idx=pub_idx,
                              priv_idx=priv_idx, count=count)
    n = int(shared.shape[0])
    return hash_batch(alg, shared.reshape(-1), count=n, stride=32, fixed_len=32, key=key), status
