"""liblcb_hash_stream_gpu.so (include/lcb_hash_stream_gpu.h): builds, loads
after liblcb_hash_gpu.so, exports every declared symbol, takes its runtime
pieces from the hash library, keeps its kernels out of it, lays the record out
as the header says, refuses bad arguments before touching HIP, fails loudly
(never on the CPU) where no MI355X is visible, and none of its kernels uses
scratch.  (The argument errors that need a live set -- unknown flags, count
past the set, NULL digests / states -- are in tests/test_stream_gpu.py.)"""
import ctypes
import errno
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lcb_hash_stream_gpu.h")
LIBDIR = os.path.join(ROOT, "liblcb_amd")
SO = os.path.join(LIBDIR, "liblcb_hash_stream_gpu.so")
E = errno.EINVAL
NAMES = ["lcb_hash_stream_abi_version", "lcb_hash_stream_alg", "lcb_hash_stream_count", "lcb_hash_stream_create",
         "lcb_hash_stream_destroy", "lcb_hash_stream_export", "lcb_hash_stream_final", "lcb_hash_stream_import",
         "lcb_hash_stream_reset", "lcb_hash_stream_update"]


@pytest.fixture(scope="module")
def S():
    from liblcb_amd import stream
    return stream


@pytest.fixture(scope="module")
def L(S):
    return S.stream_lib()


@pytest.fixture(scope="module")
def caller(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stream_caller") / "stream_caller")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "stream_caller.c"), "-o", exe,
                           "-L" + LIBDIR, "-llcb_hash_stream_gpu", "-llcb_hash_gpu", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath-link," + LIBDIR + ":/opt/rocm/lib"])
    return exe


def test_exports_every_declared_symbol(S, L):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(lcb_[a-z_0-9]+)\(", src)))
    assert names == NAMES
    out = subprocess.check_output(["nm", "-D", "--defined-only", SO]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert not [n for n in names if n not in exported]
    assert sorted(n for n, _, _ in S.STREAM_SIGNATURES) == names
    assert "LCB_HASH_STREAM_ABI_VERSION\t1" in open(HDR).read() and L.lcb_hash_stream_abi_version() == 1
    assert S.STREAM_ABI_VERSION == 1 and S.F_KEEP == 2
    # the shared runtime pieces come from the hash library, not from copies
    needed = subprocess.check_output(["readelf", "-d", SO]).decode()
    assert "liblcb_hash_gpu.so" in needed and "$ORIGIN" in needed
    undefined = subprocess.check_output(["nm", "-D", "--undefined-only", SO]).decode()
    for sym in ("ensure_init", "map_err", "scratch_alloc", "scratch_free", "parallel_copy"):
        assert re.search(r" U _ZN6lcbgpu\d+%s" % sym, undefined), sym
    # the hash library is as it was: ABI 6, no stream kernel, no stream entry point
    from liblcb_amd import lib
    assert lib().lcb_hash_gpu_abi_version() == 6
    hash_syms = subprocess.check_output(["nm", "-D", os.path.join(LIBDIR, "liblcb_hash_gpu.so")]).decode()
    assert "lcb_hash_stream" not in hash_syms and "stream_update_kernel" not in hash_syms


def test_package_exports(S):
    import liblcb_amd
    assert liblcb_amd.stream is S and liblcb_amd.stream_lib is S.stream_lib and liblcb_amd.StreamSet is S.StreamSet
    assert "StreamSet" in liblcb_amd.__all__ and "stream_lib" in liblcb_amd.__all__


def test_record_layout_c99_and_numpy(S, caller):
    """sizeof / offsetof from a C99 translation unit against the header, the
    numpy dtype of export_states and the header's own field order."""
    lines = subprocess.check_output([caller]).decode().split("\n")
    nums = [int(x) for x in lines[0].split()]
    assert nums == [344, 0, 4, 8, 16, 24, 88, 152, 216]
    dt = S.STATE_DTYPE
    assert dt.itemsize == 344
    assert [dt.fields[n][1] for n in ("alg", "used", "count", "count_hi", "h", "n", "sigma", "buf")] == nums[1:]
    assert list(dt.names) == ["alg", "used", "count", "count_hi", "h", "n", "sigma", "buf"]
    assert lines[1].strip() == "ok"          # the C caller's own EINVAL checks


def test_argument_errors_before_hip(L):
    out = ctypes.c_void_p(0x1234)
    buf = np.zeros(344, np.uint8)
    p = buf.ctypes.data
    assert L.lcb_hash_stream_create(1, None, 0, 4, None, None) == E                    # NULL out pointer
    for alg in (0, 9, -1, 101):                                                        # unknown algorithm
        assert L.lcb_hash_stream_create(alg, None, 0, 4, None, ctypes.byref(out)) == E
        assert out.value is None                                                       # *out is cleared
    assert L.lcb_hash_stream_create(1, None, 0, 0, None, ctypes.byref(out)) == E       # nstreams == 0
    assert L.lcb_hash_stream_create(1, None, 0, 1 << 32, None, ctypes.byref(out)) == E
    assert L.lcb_hash_stream_create(1, None, 5, 4, None, ctypes.byref(out)) == E       # key_len without a key
    # a NULL set
    assert L.lcb_hash_stream_update(None, None, p, None, None, 1, 64, 64, 0, None) == E
    assert L.lcb_hash_stream_final(None, None, 1, p, 0, None) == E
    assert L.lcb_hash_stream_reset(None, None, 1, 0, None) == E
    assert L.lcb_hash_stream_export(None, None, 1, p) == E and L.lcb_hash_stream_import(None, None, 1, p) == E
    assert L.lcb_hash_stream_destroy(None) == E
    assert L.lcb_hash_stream_count(None) == 0 and L.lcb_hash_stream_alg(None) == 0


def test_fails_loudly_without_gpu(S, L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import liblcb_amd
    out = ctypes.c_void_p()
    for alg in range(1, 9):
        assert L.lcb_hash_stream_create(alg, None, 0, 4, None, ctypes.byref(out)) == errno.ENODEV
        assert L.lcb_hash_stream_create(alg, b"key", 3, 4, None, ctypes.byref(out)) == errno.ENODEV
        assert out.value is None
    with pytest.raises(liblcb_amd.LcbHashError) as e:
        S.StreamSet(liblcb_amd.MD5, 8)
    assert e.value.errno == errno.ENODEV


def test_missing_library_raises_not_falls_back(S, monkeypatch):
    import liblcb_amd
    monkeypatch.setattr(S, "_slib", None)
    monkeypatch.setattr(S, "LIB_PATH", os.path.join(LIBDIR, "no_such_liblcb_hash_stream_gpu.so"))
    with pytest.raises(liblcb_amd.LcbHashError):
        S.StreamSet(liblcb_amd.MD5, 8)


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.kernels(SO)
    names = [r["name"] for r in rows]
    want = {"stream_check_kernel": 1, "stream_fill_kernel": 1, "stream_gather_kernel": 1, "stream_scatter_kernel": 1,
            "stream_update_kernel": 5,      # MD5, SHA-1, SHA-256, SHA-512 and the GOST one
            "stream_final_kernel": 8, "stream_prep_kernel": 8}
    for k, n in want.items():
        assert sum(k in x for x in names) == n, (k, names)
    assert len(rows) == 25
    assert all(r["scratch"] == 0 for r in rows), [(r["name"], r["scratch"]) for r in rows]
    # only the GOST kernels hold a table in LDS: the 64 KiB rotated image (the one-lane prep: the flat 16 KiB)
    for r in rows:
        gost = "gost_stream" in r["name"]
        assert r["lds"] == (0 if not gost else 16384 if "prep" in r["name"] else 65536), (r["name"], r["lds"])
    # the stream kernels are in this library only
    hash_names = [r["name"] for r in kernel_resources.kernels()]
    assert hash_names and not [n for n in hash_names if "stream_" in n.lower() and "lcbstream" in n]
    assert not [n for n in hash_names if "stream_update_kernel" in n or "stream_final_kernel" in n]
