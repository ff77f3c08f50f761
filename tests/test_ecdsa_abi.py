"""liblcb_ecdsa_gpu.so (include/lcb_ecdsa_gpu.h): builds, loads after
liblcb_hash_gpu.so, exports every declared symbol, refuses bad arguments
before touching HIP, fails loudly (never on the CPU) where no MI355X is
visible, and its kernel uses no scratch."""
import errno
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lcb_ecdsa_gpu.h")
LIBDIR = os.path.join(ROOT, "liblcb_amd")
SO = os.path.join(LIBDIR, "liblcb_ecdsa_gpu.so")


@pytest.fixture(scope="module")
def E():
    from liblcb_amd import ecdsa
    return ecdsa


@pytest.fixture(scope="module")
def L(E):
    return E.ecdsa_lib()


def test_exports_every_declared_symbol(E, L):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b([a-z_0-9]+)\(", src)) - {"defined", "sizeof"})
    assert len(names) == 7, names
    out = subprocess.check_output(["nm", "-D", "--defined-only", SO]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert not [n for n in names if n not in exported]
    assert sorted(n for n, _, _ in E.ECDSA_SIGNATURES) == names
    # the shared runtime pieces come from the hash library, not from copies
    needed = subprocess.check_output(["readelf", "-d", SO]).decode()
    assert "liblcb_hash_gpu.so" in needed and "$ORIGIN" in needed
    undefined = subprocess.check_output(["nm", "-D", "--undefined-only", SO]).decode()
    for sym in ("ensure_init", "map_err"):
        assert re.search(r" U _ZN6lcbgpu\d+%s" % sym, undefined), sym


def test_package_exports(E):
    import liblcb_amd
    assert liblcb_amd.ecdsa is E and liblcb_amd.ecdsa_lib is E.ecdsa_lib and "ecdsa_lib" in liblcb_amd.__all__
    assert len(E.CURVES) == 10 and E.curve_id("secp256r1") == 1 and E.curve_id(7) == 7
    assert E.curve_id("id-gostR3410-2001-CryptoPro-A-ParamSet") == 5
    for bad in ("secp384r1", 10, -1):
        with pytest.raises(ValueError):
            E.curve_id(bad)


def test_argument_errors(E, L):
    EINVAL = errno.EINVAL
    buf = np.zeros(256, np.uint8)
    st = np.full(4, 777, np.int32)
    idx = np.zeros(4, np.uint32)
    b, s, i = buf.ctypes.data, st.ctypes.data, idx.ctypes.data

    def v(curve=1, le=0, hashes=b, hash_size=32, sigs=b, keys=b, nkeys=2, key_idx=None, count=2, status=s, flags=0):
        return L.lcb_ecdsa_verify_batch(curve, le, hashes, hash_size, sigs, keys, nkeys, key_idx, count, status,
                                        flags, None)

    # all EINVAL before touching HIP
    assert v(curve=10) == EINVAL and v(curve=-1) == EINVAL
    assert v(hash_size=0) == EINVAL and v(hash_size=65) == EINVAL
    assert v(hashes=None) == EINVAL and v(sigs=None) == EINVAL and v(keys=None) == EINVAL
    assert v(status=None) == EINVAL
    assert v(nkeys=1) == EINVAL and v(nkeys=3) == EINVAL          # key_idx == NULL needs nkeys == count
    assert v(flags=0x10) == EINVAL and v(flags=0x3) == EINVAL
    assert v(count=1 << 32, nkeys=1 << 32) == EINVAL
    assert v(count=0, nkeys=0) == 0 and v(count=0, nkeys=3, key_idx=i) == 0   # empty batch
    assert v(count=0, nkeys=0, hashes=None, sigs=None, keys=None, status=None) == 0
    for name, le in (("ecdsa_verify_be_batch", 0), ("ecdsa_verify_le_batch", 1)):
        fn = getattr(L, name)
        assert fn(10, b, 32, b, b, 2, None, 2, s, 0, None) == EINVAL, name
        assert fn(1, b, 32, b, b, 3, None, 2, s, 0, None) == EINVAL, name
        assert fn(1, b, 32, b, b, 0, None, 0, s, 0, None) == 0, name
    assert (st == 777).all()                                       # nothing was written
    out = (np.zeros(192, np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.uint32))
    p, a, h = (x.ctypes.data for x in out)
    assert L.lcb_ecdsa_curve_params(10, p, a, h) == EINVAL and L.lcb_ecdsa_curve_params(0, None, a, h) == EINVAL
    assert L.lcb_ecdsa_curve_params(0, p, None, h) == EINVAL and L.lcb_ecdsa_curve_params(0, p, a, None) == EINVAL
    from liblcb_amd import LcbHashError
    with pytest.raises(LcbHashError):
        E.verify_batch(1, buf[:64], buf[:128], buf[:128], hash_size=65)
    with pytest.raises(ValueError):
        E.verify_batch(1, buf[:64], buf[:128], buf[:64])          # fewer keys than items
    with pytest.raises(ValueError):
        E.verify_batch(1, buf[:32], buf[:128], buf[:128])         # fewer hashes than items


def test_fails_loudly_without_gpu(E, L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import liblcb_amd
    buf = np.zeros(128, np.uint8)
    st = np.full(2, 777, np.int32)
    for name in ("ecdsa_verify_be_batch", "ecdsa_verify_le_batch"):
        assert getattr(L, name)(1, buf.ctypes.data, 32, buf.ctypes.data, buf.ctypes.data, 2, None, 2,
                                st.ctypes.data, 0, None) == errno.ENODEV
    assert (st == 777).all()                                       # no CPU answer
    with pytest.raises(liblcb_amd.LcbHashError):
        E.verify_batch("secp256r1", buf[:64], buf, buf)


def test_missing_library_raises_not_falls_back(E, monkeypatch):
    import liblcb_amd
    monkeypatch.setattr(E, "_elib", None)
    monkeypatch.setattr(E, "LIB_PATH", os.path.join(LIBDIR, "no_such_liblcb_ecdsa_gpu.so"))
    with pytest.raises(liblcb_amd.LcbHashError):
        E.verify_batch(1, np.zeros(32, np.uint8), np.zeros(64, np.uint8), np.zeros(64, np.uint8))


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.kernels(SO)
    names = [r["name"] for r in rows]
    assert any("ecdsa_verify_kernel" in n for n in names), names
    assert all(r["scratch"] == 0 for r in rows), [(r["name"], r["scratch"]) for r in rows if r["scratch"]]
    k = next(r for r in rows if "ecdsa_verify_kernel" in r["name"])
    # no LDS; two waves per SIMD need at most 256 registers per lane
    assert k["lds"] == 0 and k["vgpr"] <= 256
    # the verification kernel is in this library only
    hash_names = [r["name"] for r in kernel_resources.kernels()]
    assert not [n for n in hash_names if "ecdsa" in n]


def test_c_caller_links(tmp_path):
    exe = str(tmp_path / "ecdsa_caller")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "ecdsa_caller.c"), "-o", exe,
                           "-L" + LIBDIR, "-llcb_ecdsa_gpu", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath-link," + LIBDIR + ":/opt/rocm/lib"])
    assert subprocess.check_output([exe]).decode().strip() == "ok"
