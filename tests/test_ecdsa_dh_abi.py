"""liblcb_ecdsa_dh_gpu.so (include/lcb_ecdsa_dh_gpu.h): builds, loads after
liblcb_hash_gpu.so, exports every declared symbol, refuses bad arguments
before touching HIP, fails loudly (never on the CPU) where no MI355X is
visible, and its kernel uses neither scratch nor LDS."""
import errno
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lcb_ecdsa_dh_gpu.h")
LIBDIR = os.path.join(ROOT, "liblcb_amd")
SO = os.path.join(LIBDIR, "liblcb_ecdsa_dh_gpu.so")
EINVAL = errno.EINVAL


@pytest.fixture(scope="module")
def D():
    from liblcb_amd import ecdsa_dh
    return ecdsa_dh


@pytest.fixture(scope="module")
def L(D):
    return D.ecdsa_dh_lib()


def test_exports_every_declared_symbol(D, L):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b([a-z_0-9]+)\(", src)) - {"defined", "sizeof"})
    assert names == ["ecdsa_dh_be_batch", "ecdsa_dh_le_batch", "lcb_ecdsa_dh_batch"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", SO]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert not [n for n in names if n not in exported]
    assert sorted(n for n, _, _ in D.ECDSA_DH_SIGNATURES) == names
    # the shared runtime pieces come from the hash library, not from copies; the
    # other two ECDSA libraries are not needed
    needed = subprocess.check_output(["readelf", "-d", SO]).decode()
    assert "liblcb_hash_gpu.so" in needed and "$ORIGIN" in needed
    assert "liblcb_ecdsa_gpu.so" not in needed and "liblcb_ecdsa_sign_gpu.so" not in needed
    undefined = subprocess.check_output(["nm", "-D", "--undefined-only", SO]).decode()
    for sym in ("ensure_init", "map_err"):
        assert re.search(r" U _ZN6lcbgpu\d+%s" % sym, undefined), sym


def test_package_exports(D):
    import liblcb_amd
    from liblcb_amd import _lib, ecdsa, ecdsa_sign
    assert liblcb_amd.ecdsa_dh is D and liblcb_amd.ecdsa_dh_lib is D.ecdsa_dh_lib is _lib.ecdsa_dh_lib
    assert "ecdsa_dh" in liblcb_amd.__all__ and "ecdsa_dh_lib" in liblcb_amd.__all__
    assert len({D.LIB_PATH, ecdsa.LIB_PATH, ecdsa_sign.LIB_PATH}) == 3
    # the other two modules' lists are their own headers', unchanged
    assert len(ecdsa.ECDSA_SIGNATURES) == 7 and len(ecdsa_sign.ECDSA_SIGN_SIGNATURES) == 9
    mine = {n for n, _, _ in D.ECDSA_DH_SIGNATURES}
    assert not mine & {n for n, _, _ in ecdsa.ECDSA_SIGNATURES + ecdsa_sign.ECDSA_SIGN_SIGNATURES}
    for fn in ("dh_batch", "dh_digest"):
        assert callable(getattr(D, fn)) and fn in D.__all__
    with pytest.raises(ValueError):
        D.dh_batch("secp384r1", np.zeros(64, np.uint8), np.zeros(32, np.uint8))


def test_argument_errors(D, L):
    buf = np.zeros(256, np.uint8)
    outb = np.full(256, 0x5A, np.uint8)
    st = np.full(4, 777, np.int32)
    idx = np.zeros(4, np.uint32)
    b, o, s, i = buf.ctypes.data, outb.ctypes.data, st.ctypes.data, idx.ctypes.data

    def dh(curve=1, le=0, cof=0, pub=b, npub=2, pub_idx=None, priv=b, npriv=2, priv_idx=None, count=2, shared=o,
           status=s, flags=0):
        return L.lcb_ecdsa_dh_batch(curve, le, cof, pub, npub, pub_idx, priv, npriv, priv_idx, count, shared, status,
                                    flags, None)

    # all EINVAL before touching HIP
    assert dh(curve=10) == EINVAL and dh(curve=-1) == EINVAL
    assert dh(flags=0x10) == EINVAL and dh(flags=0x3) == EINVAL
    assert dh(pub=None) == EINVAL and dh(priv=None) == EINVAL
    assert dh(shared=None) == EINVAL and dh(status=None) == EINVAL
    assert dh(npub=1) == EINVAL and dh(npub=3) == EINVAL          # pub_idx == NULL needs npub == count
    assert dh(npriv=1) == EINVAL and dh(npriv=3) == EINVAL        # priv_idx == NULL needs npriv == count
    assert dh(npub=1, pub_idx=i, npriv=3) == EINVAL and dh(npriv=1, priv_idx=i, npub=3) == EINVAL
    assert dh(count=1 << 32, npub=1 << 32, npriv=1 << 32) == EINVAL
    assert dh(count=1 << 32, npub=1, pub_idx=i, npriv=1, priv_idx=i) == EINVAL
    assert dh(npub=1 << 32, pub_idx=i) == EINVAL and dh(npriv=1 << 32, priv_idx=i) == EINVAL
    assert dh(count=0, npub=0, npriv=0) == 0                      # empty batch
    assert dh(count=0, npub=3, pub_idx=i, npriv=1, priv_idx=i) == 0
    assert dh(count=0, npub=0, npriv=0, pub=None, priv=None, shared=None, status=None) == 0
    for name in ("ecdsa_dh_be_batch", "ecdsa_dh_le_batch"):
        fn = getattr(L, name)
        for cof in (0, 1):
            assert fn(10, cof, b, 2, None, b, 2, None, 2, o, s, 0, None) == EINVAL, name
            assert fn(1, cof, b, 3, None, b, 2, None, 2, o, s, 0, None) == EINVAL, name
            assert fn(1, cof, b, 2, None, b, 1, None, 2, o, s, 0, None) == EINVAL, name
            assert fn(1, cof, None, 2, None, b, 2, None, 2, o, s, 0, None) == EINVAL, name
            assert fn(1, cof, b, 2, None, b, 2, None, 1 << 32, o, s, 0, None) == EINVAL, name
            assert fn(1, cof, b, 0, None, b, 0, None, 0, o, s, 0, None) == 0, name
    assert (st == 777).all() and (outb == 0x5A).all()             # nothing was written
    with pytest.raises(ValueError):
        D.dh_batch(1, buf[:64], buf[:32], count=2)                # fewer keys than items
    with pytest.raises(ValueError):
        D.dh_batch(1, buf[:128], buf[:32], pub_idx=idx[:2])       # two items, one unindexed private key
    with pytest.raises(ValueError):
        D.dh_batch(1, buf[:128], buf[:32], pub_idx=idx[:2], priv_idx=idx[:1])


def test_fails_loudly_without_gpu(D, L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import liblcb_amd
    buf = np.zeros(128, np.uint8)
    idx = np.zeros(2, np.uint32)
    outb = np.full(128, 0x5A, np.uint8)
    st = np.full(2, 777, np.int32)
    b, o, s, i = buf.ctypes.data, outb.ctypes.data, st.ctypes.data, idx.ctypes.data
    for name in ("ecdsa_dh_be_batch", "ecdsa_dh_le_batch"):
        assert getattr(L, name)(1, 0, b, 2, None, b, 2, None, 2, o, s, 0, None) == errno.ENODEV
        assert getattr(L, name)(1, 1, b, 2, None, b, 1, i, 2, o, s, 0, None) == errno.ENODEV
    assert (st == 777).all() and (outb == 0x5A).all()             # no CPU answer
    with pytest.raises(liblcb_amd.LcbHashError):
        D.dh_batch("secp256r1", buf[:128], buf[:64])
    with pytest.raises(liblcb_amd.LcbHashError):
        D.dh_digest(liblcb_amd.SHA256, "secp256r1", buf[:128], buf[:32], priv_idx=idx)


def test_missing_library_raises_not_falls_back(D, monkeypatch):
    import liblcb_amd
    from liblcb_amd import _lib
    monkeypatch.setattr(_lib, "_dhlib", None)
    monkeypatch.setattr(_lib, "ECDSA_DH_LIB_PATH", os.path.join(LIBDIR, "no_such_liblcb_ecdsa_dh_gpu.so"))
    z = np.zeros(64, np.uint8)
    with pytest.raises(liblcb_amd.LcbHashError):
        liblcb_amd.ecdsa_dh_lib()
    with pytest.raises(liblcb_amd.LcbHashError):
        D.dh_batch(1, z, z[:32])
    with pytest.raises(liblcb_amd.LcbHashError):
        D.dh_digest(liblcb_amd.SHA256, 1, z, z[:32])


def test_kernel_uses_no_scratch_and_no_lds():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.kernels(SO)
    assert [r["name"].split("(")[0] for r in rows] == ["lcbec::ecdsa_dh_kernel"], rows
    assert all(r["scratch"] == 0 and r["lds"] == 0 for r in rows), [(r["name"], r["scratch"], r["lds"]) for r in rows]
    # two waves per SIMD need at most 256 registers per lane
    assert all(r["vgpr"] <= 256 for r in rows), [(r["name"], r["vgpr"]) for r in rows]
    # the kernel is in this library only
    for other in (None, os.path.join(LIBDIR, "liblcb_ecdsa_gpu.so"), os.path.join(LIBDIR, "liblcb_ecdsa_sign_gpu.so")):
        there = [r["name"] for r in (kernel_resources.kernels(other) if other else kernel_resources.kernels())]
        assert there and not [n for n in there if "ecdsa_dh" in n], other


def test_c_caller_links(tmp_path):
    exe = str(tmp_path / "ecdsa_dh_caller")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "ecdsa_dh_caller.c"), "-o", exe,
                           "-L" + LIBDIR, "-llcb_ecdsa_dh_gpu", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath-link," + LIBDIR + ":/opt/rocm/lib"])
    assert subprocess.check_output([exe]).decode().strip() == "ok"
