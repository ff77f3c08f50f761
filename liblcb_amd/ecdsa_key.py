"""Host-side mirror of the public-key import and export of liblcb's
include/crypto/dsa/ecdsa.h, batched, over the ten 256-bit prime-field curves
of liblcb_amd.ecdsa.

import_batch(curve, keys, ...) returns (pub_keys, status, infinity): per item
exactly what the reference's ecdsa_pub_key_import_be (le=False) or _le
(le=True) returns for the compressed (33 bytes, 02/03 || x), packed (65 bytes,
04/06/07 || x || y), raw (64), x with a separate y (32) and one-byte-infinity
forms, and on 0 the x || y its export of the imported point writes: the form
verify_batch, sign / pub_key_batch and dh_batch take.  export_batch(curve,
pub_keys, form) writes the compressed or the packed form of every key
(include/lcb_ecdsa_key_gpu.h has the whole contract).  verify_wire() imports a
table of wire-form keys and verifies signatures against it through key_idx,
all on the device.

torch CUDA tensors run in device mode on torch's current stream without
waiting; numpy / bytes run in host mode through page-locked staging.  Every
output is produced by the HIP kernels of liblcb_ecdsa_key_gpu.so; there is no
CPU path.
"""
import numpy as np
import torch

from . import _lib
from ._lib import ECDSA_KEY_SIGNATURES, F_DEVICE, check, ecdsa_key_lib
from .ecdsa import _host_u8, curve_id, verify_batch
from .hash import _is_dev

__all__ = ["import_batch", "export_batch", "verify_wire", "ecdsa_key_lib", "ECDSA_KEY_SIGNATURES", "LIB_PATH",
           "PACKED", "COMPRESSED", "FORM_SIZE"]

LIB_PATH = _lib.ECDSA_KEY_LIB_PATH
PACKED, COMPRESSED = 0, 1  # LCB_ECDSA_KEY_PACKED, LCB_ECDSA_KEY_COMPRESSED
FORM_SIZE = {PACKED: 65, COMPRESSED: 33}


def _dev_arr(name, t, dev, dtypes):
    if not _is_dev(t) or t.device != dev or t.dtype not in dtypes or not t.is_contiguous():
        raise TypeError("%s must be a contiguous %s tensor on %s" % (name, " / ".join(str(d) for d in dtypes), dev))
    return t


def import_batch(curve, keys, key_size=None, key_stride=None, sizes=None, keys_y=None, le=False, count=None,
                 want_infinity=True):
    """One x || y, one status and one infinity flag per key.

    keys        the keys, item i at byte i * key_stride
    key_size    the size of every key where `sizes` is None; defaults to
                key_stride
    key_stride  defaults to the row length of a 2-D array, else to key_size
    sizes       int32/uint32 per item, or None; an item whose size is above
                key_stride reads nothing and gets EINVAL.  With sizes, keys
                holds count * key_stride bytes
    keys_y      count x 32 bytes or None: the y of the items of size 32
    le          every number little-endian (ecdsa_pub_key_import_le), else
                big-endian; the prefix byte is the first byte in both
    count       defaults to the length of `sizes`, else to what `keys` holds
    want_infinity  False: the flags are not written and None is returned
    returns     (pub_keys uint8 (count, 64), status int32 (count,), infinity
                uint8 (count,) or None), same kind of memory as `keys`:
                status 0 with x || y, or with zeros and infinity 1 for the
                point at infinity; -1 (refused key, unknown prefix or size,
                no square root) or EINVAL (size 0, size 1 with a non-zero
                byte, size 32 without keys_y, size above key_stride) with zeros
    """
    L = ecdsa_key_lib()
    cid = curve_id(curve)
    dev = keys.device if _is_dev(keys) else None
    if key_stride is None:
        key_stride = int(keys.shape[1]) if getattr(keys, "ndim", 1) == 2 else key_size
    if key_stride is None:
        raise ValueError("key_stride or key_size is needed for a flat array of keys")
    key_stride = int(key_stride)
    key_size = key_stride if key_size is None else int(key_size)
    if key_stride < 0 or key_size < 0:
        raise ValueError("key_stride and key_size must not be negative")
    if dev is not None:
        _dev_arr("keys", keys, dev, (torch.uint8,))
        have = int(keys.numel())
        if sizes is not None:
            _dev_arr("sizes", sizes, dev, (torch.int32, torch.uint32))
        if keys_y is not None:
            _dev_arr("keys_y", keys_y, dev, (torch.uint8,))
        n_sizes = int(sizes.numel()) if sizes is not None else None
        n_y = int(keys_y.numel()) // 32 if keys_y is not None else None
    else:
        keys = _host_u8(keys)
        have = int(keys.size)
        if sizes is not None:
            sizes = np.ascontiguousarray(sizes).reshape(-1)
            if sizes.dtype != np.uint32:
                sizes = sizes.view(np.uint32) if sizes.dtype == np.int32 else sizes.astype(np.uint32)
        if keys_y is not None:
            keys_y = _host_u8(keys_y)
        n_sizes = int(sizes.size) if sizes is not None else None
        n_y = int(keys_y.size) // 32 if keys_y is not None else None
    if count is None:
        if n_sizes is not None:
            count = n_sizes
        elif key_stride:
            count = (have + key_stride - min(key_size, key_stride)) // key_stride
        else:
            raise ValueError("count is needed where key_stride is 0")
    count = int(count)
    if n_sizes is not None and n_sizes < count:
        raise ValueError("sizes holds %d entries, count is %d" % (n_sizes, count))
    if n_y is not None and n_y < count:
        raise ValueError("keys_y holds %d numbers, count is %d" % (n_y, count))
    # every item but the last spans key_stride bytes; the last is read up to its size, key_stride at most
    if count and sizes is None and have < (count - 1) * key_stride + min(key_size, key_stride):
        raise ValueError("keys holds %d bytes, fewer than %d items of stride %d" % (have, count, key_stride))
    if count and sizes is not None and have < count * key_stride:
        raise ValueError("keys holds %d bytes, fewer than %d items of stride %d" % (have, count, key_stride))
    head = (cid, 1 if le else 0)
    if dev is not None:
        pub = torch.empty(64 * count, dtype=torch.uint8, device=dev)
        status = torch.empty(count, dtype=torch.int32, device=dev)
        inf = torch.empty(count, dtype=torch.uint8, device=dev) if want_infinity else None
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            check(L.lcb_ecdsa_key_import_batch(*head, keys.data_ptr(), key_stride,
                                               sizes.data_ptr() if sizes is not None else None, key_size,
                                               keys_y.data_ptr() if keys_y is not None else None, count,
                                               pub.data_ptr(), inf.data_ptr() if inf is not None else None,
                                               status.data_ptr(), F_DEVICE, stream))
        return pub.reshape(count, 64), status, inf
    pub, status = np.empty(64 * count, np.uint8), np.empty(count, np.int32)
    inf = np.empty(count, np.uint8) if want_infinity else None
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    check(L.lcb_ecdsa_key_import_batch(*head, ptr(keys), key_stride, ptr(sizes), key_size, ptr(keys_y), count, ptr(pub),
                                       ptr(inf), ptr(status), 0, None))
    return pub.reshape(count, 64), status, inf


def export_batch(curve, pub_keys, form=COMPRESSED, infinity=None, le=False, count=None, out_stride=None, out=None):
    """The compressed or the packed form of every key; nothing is validated,
    as the reference validates nothing.

    pub_keys    count x 64 bytes, x || y
    form        COMPRESSED (33 bytes, 02/03 || x) or PACKED (65 bytes, 04 || x || y)
    infinity    uint8 per item or None: a non-zero entry exports the point at
                infinity, one zero byte
    out_stride  defaults to the size of the form
    out         a uint8 buffer of >= count * out_stride bytes to write into;
                no byte past an item's size is written
    returns     (out uint8 (count, out_stride), sizes uint32 / int32 (count,),
                status int32 (count,), all 0)
    """
    L = ecdsa_key_lib()
    cid = curve_id(curve)
    if form not in FORM_SIZE:
        raise ValueError("form must be PACKED or COMPRESSED")
    out_stride = FORM_SIZE[form] if out_stride is None else int(out_stride)
    if out_stride < 0:
        raise ValueError("out_stride must not be negative")
    dev = pub_keys.device if _is_dev(pub_keys) else None
    if dev is not None:
        _dev_arr("pub_keys", pub_keys, dev, (torch.uint8,))
        nkeys = int(pub_keys.numel()) // 64
        if infinity is not None:
            _dev_arr("infinity", infinity, dev, (torch.uint8,))
        n_inf = int(infinity.numel()) if infinity is not None else None
    else:
        pub_keys = _host_u8(pub_keys)
        nkeys = int(pub_keys.size) // 64
        if infinity is not None:
            infinity = _host_u8(infinity)
        n_inf = int(infinity.size) if infinity is not None else None
    count = nkeys if count is None else int(count)
    if nkeys < count or (n_inf is not None and n_inf < count):
        raise ValueError("pub_keys / infinity hold fewer than %d items" % count)
    head = (cid, 1 if le else 0, form)
    if dev is not None:
        if out is None:
            out = torch.zeros(count * out_stride, dtype=torch.uint8, device=dev)
        else:
            _dev_arr("out", out, dev, (torch.uint8,))
            if int(out.numel()) < count * out_stride:
                raise ValueError("out holds fewer than %d items of stride %d" % (count, out_stride))
        sizes = torch.empty(count, dtype=torch.int32, device=dev)
        status = torch.empty(count, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            check(L.lcb_ecdsa_key_export_batch(*head, pub_keys.data_ptr(),
                                               infinity.data_ptr() if infinity is not None else None, count,
                                               out.data_ptr(), out_stride, sizes.data_ptr(), status.data_ptr(),
                                               F_DEVICE, stream))
        return out.reshape(-1)[:count * out_stride].reshape(count, out_stride), sizes, status
    if out is None:
        out = np.zeros(count * out_stride, np.uint8)
    elif not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags.c_contiguous or \
            out.size < count * out_stride:
        raise TypeError("out must be a C-contiguous uint8 numpy array of >= count * out_stride bytes")
    sizes, status = np.empty(count, np.uint32), np.empty(count, np.int32)
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    check(L.lcb_ecdsa_key_export_batch(*head, ptr(pub_keys), ptr(infinity), count, ptr(out), out_stride, ptr(sizes),
                                       ptr(status), 0, None))
    return out.reshape(-1)[:count * out_stride].reshape(count, out_stride), sizes, status


def verify_wire(curve, hashes, sigs, keys, key_idx=None, key_size=None, key_stride=None, sizes=None, le=False,
                hash_size=None, count=None):
    """import_batch of a table of wire-form keys, then ecdsa.verify_batch
    against the table (through key_idx where given); for CUDA tensors the two
    calls are enqueued back to back on the current stream and the keys never
    leave the device.

    Returns (verify_status (count,), key_status (nkeys,)).  A key whose import
    status is not 0, and the point at infinity, is (0, 0) in the table and
    every signature under it gets -1 from the verification: verify_status
    alone already refuses them, key_status says why.
    """
    pub, key_status, _ = import_batch(curve, keys, key_size=key_size, key_stride=key_stride, sizes=sizes, le=le,
                                      want_infinity=False)
    status = verify_batch(curve, hashes, sigs, pub.reshape(-1), key_idx=key_idx, le=le, hash_size=hash_size,
                          count=count)
    return status, key_status
