"""Batched radius_pkt_sign / radius_pkt_verify of packed packets on the GPU:
the Python mirror of include/lcb_radius_gpu.h (liblcb_radius_gpu.so).

sign_packed / verify_packed take the packets as ONE uint8 buffer plus a
description (offsets/buf_sizes or stride/fixed_size) and work IN PLACE:
a torch CUDA tensor runs in device mode on torch's current stream, a numpy
array in host mode through page-locked staging.  Both return errors, one
int32 per packet (0 or the code the reference function returns), in the same
kind of memory.  pack / unpack / req_headers convert lists of `bytes`.

Every parse, XOR, compare and hash runs in the HIP kernels of
liblcb_radius_gpu.so and liblcb_hash_gpu.so; there is no CPU path
(liblcb_amd.radius is the per-packet host model these are checked against).
"""
import ctypes
import os

import numpy as np
import torch

from ._lib import F_DEVICE, HERE, c_sz, c_u32, c_u64, c_vp, check, load_satellite
from .hash import _dev_batch, _host_batch, _is_dev, _key_table

__all__ = ["radius_lib", "sign_packed", "verify_packed", "pack", "unpack", "req_headers", "RADIUS_SIGNATURES"]

LIB_PATH = os.path.join(HERE, "liblcb_radius_gpu.so")

_SIGN = [c_vp, c_vp, c_vp, c_sz, c_u64, c_u32, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_u32, c_vp]
_VERIFY = _SIGN[:11] + [c_vp] + _SIGN[11:]
# every symbol include/lcb_radius_gpu.h declares
RADIUS_SIGNATURES = [
    ("radius_pkt_sign_batch", ctypes.c_int, _SIGN),
    ("radius_pkt_verify_batch", ctypes.c_int, _VERIFY),
]

_rlib = None


def radius_lib():
    """The loaded liblcb_radius_gpu.so (after liblcb_hash_gpu.so, which it
    links against); raises LcbHashError if it has not been built."""
    global _rlib
    if _rlib is None:
        _rlib = load_satellite(LIB_PATH, RADIUS_SIGNATURES)
    return _rlib


def pack(packets, gaps=None, fill=0):
    """(blob, offsets, buf_sizes) numpy arrays for a list of `bytes`; gaps[i]
    bytes of `fill` ahead of packet i (default: none)."""
    n = len(packets)
    sizes = np.array([len(p) for p in packets], np.uint32)
    gaps = np.zeros(n, np.uint64) if gaps is None else np.asarray(gaps, np.uint64)
    offs = np.cumsum(gaps + np.concatenate(([0], sizes[:-1])).astype(np.uint64), dtype=np.uint64) if n else \
        np.zeros(0, np.uint64)
    blob = np.full(int(offs[-1] + sizes[-1]) if n else 1, fill, np.uint8)
    for p, o in zip(packets, offs):
        blob[int(o):int(o) + len(p)] = np.frombuffer(bytes(p), np.uint8)
    return blob, offs, sizes


def unpack(blob, offsets, buf_sizes):
    """The list of `bytes` buffers of a packed blob (numpy or torch)."""
    to_np = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)  # noqa: E731
    b, o, s = to_np(blob), to_np(offsets), to_np(buf_sizes)
    return [bytes(b[int(x):int(x) + int(n)]) for x, n in zip(o, s)]


def req_headers(requests):
    """count x 20 uint8: the first 20 bytes of each reply's request, zeros
    (code 0 = no request) where requests[i] is None."""
    out = np.zeros((len(requests), 20), np.uint8)
    for i, r in enumerate(requests):
        if r is not None:
            if len(r) < 20:
                raise ValueError("request %d is shorter than a RADIUS header" % i)
            out[i] = np.frombuffer(bytes(r[:20]), np.uint8)
    return out.reshape(-1)


def _ptr(t):
    if t is None:
        return None
    return t.data_ptr() if isinstance(t, torch.Tensor) else t.ctypes.data


def _run(verify, pkts, keys, key_index, offsets, buf_sizes, count, stride, fixed_size, req_hdrs, key_table=None):
    blob, koff, klen, _ = _key_table(keys, key_table)
    L = radius_lib()
    fn = L.radius_pkt_verify_batch if verify else L.radius_pkt_sign_batch
    if _is_dev(pkts):
        count, stride, fixed_size, err = _dev_batch(pkts, count, offsets, buf_sizes, stride, fixed_size, None, 4,
                                                    per_msg=(("key_index", key_index),))
        if req_hdrs is not None:
            if not _is_dev(req_hdrs) or req_hdrs.device != pkts.device:
                raise ValueError("req_hdrs must be a tensor on %s" % pkts.device)
            if req_hdrs.dtype != torch.uint8 or not req_hdrs.is_contiguous():
                raise TypeError("req_hdrs must be a contiguous uint8 tensor")
            if int(req_hdrs.numel()) < 20 * count:
                raise ValueError("req_hdrs holds %d bytes, %d x 20 needed" % (int(req_hdrs.numel()), count))
        err = err.view(torch.int32).reshape(count)
        args = [_ptr(pkts), _ptr(offsets), _ptr(buf_sizes), count, stride, fixed_size, blob.ctypes.data,
                _ptr(koff), klen.ctypes.data, len(klen), _ptr(key_index)]
        with torch.cuda.device(pkts.device):
            stream = torch.cuda.current_stream(pkts.device).cuda_stream
            check(fn(*(args + ([_ptr(req_hdrs)] if verify else []) + [_ptr(err), F_DEVICE, stream])))
        return err
    if not isinstance(pkts, np.ndarray) or pkts.dtype != np.uint8 or not pkts.flags.c_contiguous or \
            not pkts.flags.writeable:
        raise TypeError("pkts must be a writable C-contiguous uint8 numpy array (or a CUDA tensor): "
                        "the packets are signed / verified in place")
    for name, t in (("offsets", offsets), ("buf_sizes", buf_sizes), ("key_index", key_index), ("req_hdrs", req_hdrs)):
        if isinstance(t, torch.Tensor):
            raise ValueError("%s is a tensor but pkts is host memory" % name)
    _, offsets, buf_sizes, (key_index,), count, stride, fixed_size, err, _ = _host_batch(
        pkts, count, offsets, buf_sizes, stride, fixed_size, None, 4, per_msg=(("key_index", key_index),))
    if req_hdrs is not None:
        req_hdrs = np.ascontiguousarray(req_hdrs, dtype=np.uint8).reshape(-1)
        if req_hdrs.size < 20 * count:
            raise ValueError("req_hdrs holds %d bytes, %d x 20 needed" % (req_hdrs.size, count))
    err = err.view(np.int32).reshape(count)
    args = [pkts.ctypes.data, _ptr(offsets), _ptr(buf_sizes), count, stride, fixed_size, blob.ctypes.data,
            _ptr(koff), klen.ctypes.data, len(klen), _ptr(key_index)]
    check(fn(*(args + ([_ptr(req_hdrs)] if verify else []) + [err.ctypes.data, 0, None])))
    return err


def sign_packed(pkts, keys, key_index=None, offsets=None, buf_sizes=None, count=None, stride=0, fixed_size=0,
                key_table=None):
    """radius_pkt_sign(pkt, buf, NULL, key, key_len, 0) of every packed packet,
    in place (radius.h:1487-1532).  pkts: uint8 CUDA tensor or numpy array;
    keys: the shared secrets (sequence of bytes, host memory), or None with
    key_table=(blob, key_offsets or None, key_lengths), the caller's own key
    geometry (liblcb_amd.hash._key_table); key_index[i]:
    packet i's secret (default 0), offsets / buf_sizes or stride / fixed_size:
    where packet i's buffer lies.  Returns errors (int32 per packet); a packet
    with a nonzero error is unchanged."""
    return _run(False, pkts, keys, key_index, offsets, buf_sizes, count, stride, fixed_size, None, key_table)


def verify_packed(pkts, keys, key_index=None, offsets=None, buf_sizes=None, count=None, stride=0, fixed_size=0,
                  req_hdrs=None, key_table=None):
    """radius_pkt_verify(pkt, key, key_len, pkt_req) of every packed packet
    (radius.h:1535-1568); req_hdrs: req_headers(requests) in the batch's kind
    of memory, or None; keys / key_table as sign_packed.  Returns errors; the
    User-Password of a packet with errors[i] == 0 is decoded in place, nothing
    else changes."""
    return _run(True, pkts, keys, key_index, offsets, buf_sizes, count, stride, fixed_size, req_hdrs, key_table)
