"""Batched streaming digests: device-resident init / update / final contexts
(include/lcb_hash_stream_gpu.h, liblcb_hash_stream_gpu.so).

A StreamSet is `nstreams` contexts of one algorithm on the current device,
optionally keyed (HMAC, one key per set).  update() absorbs one chunk per
listed stream, final() returns the digests (and re-initialises the streams
unless keep=True), export_states() / import_states() move the reference
context's fields (chaining value, byte count, leftover bytes; N and Sigma for
GOST) to and from host records.  After update() a stream holds exactly what
the reference's *_update leaves in its context (md5.h:233-262, sha1.h:761-800,
sha2.h:647-681, gost3411-2012.h:1767-1799).

torch CUDA tensors run in device mode on torch's current stream; numpy arrays
/ bytes run in host mode through page-locked staging.  Every digest is
computed by the HIP kernels of liblcb_hash_stream_gpu.so; there is no CPU
path.
"""
import ctypes
import os

import numpy as np
import torch

from ._lib import DIGEST_SIZE, F_DEVICE, HERE, c_sz, c_u32, c_u64, c_vp, check, load_satellite
from .hash import _check_extent, _is_dev, _layout

__all__ = ["StreamSet", "stream_lib", "STATE_DTYPE", "F_KEEP", "STREAM_ABI_VERSION", "STREAM_SIGNATURES"]

LIB_PATH = os.path.join(HERE, "liblcb_hash_stream_gpu.so")
STREAM_ABI_VERSION = 1
F_KEEP = 0x2

# lcb_hash_stream_state_t, 344 bytes
STATE_DTYPE = np.dtype([("alg", "<u4"), ("used", "<u4"), ("count", "<u8"), ("count_hi", "<u8"),
                        ("h", "u1", (64,)), ("n", "u1", (64,)), ("sigma", "u1", (64,)), ("buf", "u1", (128,))])

c_int = ctypes.c_int
# every symbol include/lcb_hash_stream_gpu.h declares
STREAM_SIGNATURES = [
    ("lcb_hash_stream_abi_version", c_int, []),
    ("lcb_hash_stream_create", c_int, [c_int, c_vp, c_sz, c_sz, c_vp, ctypes.POINTER(c_vp)]),
    ("lcb_hash_stream_destroy", c_int, [c_vp]),
    ("lcb_hash_stream_count", c_sz, [c_vp]),
    ("lcb_hash_stream_alg", c_int, [c_vp]),
    ("lcb_hash_stream_reset", c_int, [c_vp, c_vp, c_sz, c_u32, c_vp]),
    ("lcb_hash_stream_update", c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_u64, c_u32, c_u32, c_vp]),
    ("lcb_hash_stream_final", c_int, [c_vp, c_vp, c_sz, c_vp, c_u32, c_vp]),
    ("lcb_hash_stream_export", c_int, [c_vp, c_vp, c_sz, c_vp]),
    ("lcb_hash_stream_import", c_int, [c_vp, c_vp, c_sz, c_vp]),
]

_slib = None


def stream_lib():
    """The loaded liblcb_hash_stream_gpu.so (after liblcb_hash_gpu.so, which it
    links against); raises LcbHashError if it has not been built."""
    global _slib
    if _slib is None:
        _slib = load_satellite(LIB_PATH, STREAM_SIGNATURES)
    return _slib


def _ptr(t):
    if t is None:
        return None
    return t.data_ptr() if isinstance(t, torch.Tensor) else t.ctypes.data


def _host_u8(a):
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(a), dtype=np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8)


class StreamSet:
    """`nstreams` streaming contexts of `alg` (an id of liblcb_amd, 1..8) on
    the current device; key: bytes for HMAC (b"" is a valid key), None for
    plain digests."""

    def __init__(self, alg, nstreams, key=None):
        self._L = stream_lib()
        self._h = c_vp()
        self.alg, self.nstreams, self.keyed = int(alg), int(nstreams), key is not None
        kbuf, klen = None, 0
        if key is not None:
            key = bytes(key)
            klen = len(key)
            kbuf = (ctypes.c_uint8 * max(klen, 1)).from_buffer_copy(key or b"\0")
        stream = torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else None
        check(self._L.lcb_hash_stream_create(self.alg, kbuf, klen, self.nstreams, stream, ctypes.byref(self._h)))
        self.digest_size = DIGEST_SIZE[self.alg]
        self.device = torch.device("cuda", torch.cuda.current_device())

    # -- helpers
    def _handle(self):
        if not self._h:
            raise ValueError("the stream set is closed")
        return self._h

    def _index(self, index, dev, count=None):
        """The index list as the call's memory mode wants it, or None."""
        if index is None:
            return None
        if dev is not None:
            if not (_is_dev(index) and index.dtype in (torch.int32, torch.uint32) and index.is_contiguous()
                    and index.device == dev):
                raise TypeError("index must be a contiguous int32/uint32 tensor on the data's device")
        else:
            if _is_dev(index):
                raise TypeError("index is a device tensor in a host-mode call")
            index = np.ascontiguousarray(index, dtype=np.uint32)
        if count is not None and int(index.shape[0]) < count:
            raise ValueError("index has %d entries, count is %d" % (int(index.shape[0]), count))
        return index

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    # -- the operations
    def update(self, data, lengths=None, offsets=None, index=None, count=None, stride=0, fixed_len=0):
        """Absorb chunk i (data + offsets[i] or i * stride, lengths[i] or
        fixed_len bytes) into stream index[i] (default i)."""
        h = self._handle()
        if _is_dev(data):
            if data.dtype != torch.uint8 or not data.is_contiguous():
                raise TypeError("data must be a contiguous uint8 tensor")
            dev, total = data.device, data.numel()
            for t, dt in ((offsets, (torch.int64, torch.uint64)), (lengths, (torch.int32, torch.uint32))):
                if t is not None and not (_is_dev(t) and t.dtype in dt and t.is_contiguous() and t.device == dev):
                    raise TypeError("offsets / lengths must be contiguous int64 / int32 tensors on data's device")
        else:
            data = _host_u8(data)
            dev, total = None, data.size
            if offsets is not None:
                offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            if lengths is not None:
                lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        if count is None and lengths is None and offsets is None and index is not None:
            count = int(index.shape[0])
        count, stride, fixed_len = _layout(count, offsets, lengths, stride or None, fixed_len or None, total)
        _check_extent(total, count, offsets, lengths, stride, fixed_len)
        index = self._index(index, dev, count)
        if count == 0:
            return
        if dev is not None:
            with torch.cuda.device(dev):
                check(self._L.lcb_hash_stream_update(h, _ptr(index), _ptr(data), _ptr(offsets), _ptr(lengths), count,
                                                     stride, fixed_len, F_DEVICE, self._stream()))
        else:
            check(self._L.lcb_hash_stream_update(h, _ptr(index), data.ctypes.data if data.size else None,
                                                 _ptr(offsets), _ptr(lengths), count, stride, fixed_len, 0, None))

    def final(self, index=None, keep=False, count=None):
        """Digests of the listed streams (default: all), count x D uint8: a
        CUDA tensor when index is one or absent, a numpy array when index is a
        numpy array.  keep=True leaves the streams as they are; otherwise they
        are freshly initialised."""
        h = self._handle()
        host = index is not None and not _is_dev(index)
        index = self._index(index, None if host else self.device)
        if count is None:
            count = int(index.shape[0]) if index is not None else self.nstreams
        flags = F_KEEP if keep else 0
        D = self.digest_size
        if host:
            out = np.zeros((count, D), np.uint8)
            check(self._L.lcb_hash_stream_final(h, _ptr(index), count, out.ctypes.data, flags, None))
            return out
        out = torch.zeros((count, D), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            check(self._L.lcb_hash_stream_final(h, _ptr(index), count, out.data_ptr(), flags | F_DEVICE,
                                                self._stream()))
        return out

    def final_host(self, index=None, keep=False, count=None):
        """final() in host mode (numpy out) whatever the index."""
        if index is None:
            index = np.arange(self.nstreams if count is None else count, dtype=np.uint32)
        return self.final(np.ascontiguousarray(index, dtype=np.uint32), keep=keep, count=count)

    def reset(self, index=None, count=None):
        """The listed streams (default: all) as after *_init / hmac_*_init(key)."""
        h = self._handle()
        host = index is not None and not _is_dev(index)
        index = self._index(index, None if host else self.device)
        if count is None:
            count = int(index.shape[0]) if index is not None else self.nstreams
        if host:
            check(self._L.lcb_hash_stream_reset(h, _ptr(index), count, 0, None))
        else:
            with torch.cuda.device(self.device):
                check(self._L.lcb_hash_stream_reset(h, _ptr(index), count, F_DEVICE, self._stream()))

    def export_states(self, index=None):
        """The listed streams' records (default: all) as a numpy structured
        array of STATE_DTYPE; synchronous."""
        h = self._handle()
        if index is not None:
            index = np.ascontiguousarray(index.cpu().numpy() if _is_dev(index) else index, dtype=np.uint32)
        count = int(index.shape[0]) if index is not None else self.nstreams
        out = np.zeros(count, STATE_DTYPE)
        check(self._L.lcb_hash_stream_export(h, _ptr(index), count, out.ctypes.data))
        return out

    def import_states(self, states, index=None):
        """Load records (STATE_DTYPE) into the listed streams (default: the
        first len(states)); synchronous.  EINVAL with nothing changed for a
        record of another algorithm or with an impossible `used`."""
        h = self._handle()
        states = np.ascontiguousarray(states, dtype=STATE_DTYPE)
        if index is not None:
            index = np.ascontiguousarray(index.cpu().numpy() if _is_dev(index) else index, dtype=np.uint32)
            if int(index.shape[0]) != states.shape[0]:
                raise ValueError("index has %d entries for %d records" % (int(index.shape[0]), states.shape[0]))
        check(self._L.lcb_hash_stream_import(h, _ptr(index), states.shape[0], states.ctypes.data))

    def close(self):
        if self._h:
            h, self._h = self._h, c_vp()
            check(self._L.lcb_hash_stream_destroy(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
