"""liblcb_ecdsa_key_gpu.so (include/lcb_ecdsa_key_gpu.h): builds, loads after
liblcb_hash_gpu.so, exports every declared symbol, refuses bad arguments
before touching HIP, fails loudly (never on the CPU) where no MI355X is
visible, and its kernels use neither scratch nor LDS."""
import errno
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lcb_ecdsa_key_gpu.h")
LIBDIR = os.path.join(ROOT, "liblcb_amd")
SO = os.path.join(LIBDIR, "liblcb_ecdsa_key_gpu.so")
EINVAL = errno.EINVAL
NAMES = ["ecdsa_pub_key_export_be_batch", "ecdsa_pub_key_export_le_batch", "ecdsa_pub_key_import_be_batch",
         "ecdsa_pub_key_import_le_batch", "lcb_ecdsa_key_export_batch", "lcb_ecdsa_key_import_batch"]


@pytest.fixture(scope="module")
def K():
    from liblcb_amd import ecdsa_key
    return ecdsa_key


@pytest.fixture(scope="module")
def L(K):
    return K.ecdsa_key_lib()


def test_exports_every_declared_symbol(K, L):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b([a-z_0-9]+)\(", src)) - {"defined", "sizeof"})
    assert names == NAMES
    out = subprocess.check_output(["nm", "-D", "--defined-only", SO]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert not [n for n in names if n not in exported]
    assert sorted(n for n, _, _ in K.ECDSA_KEY_SIGNATURES) == names
    assert (K.PACKED, K.COMPRESSED) == tuple(int(re.search(r"#define\s+LCB_ECDSA_KEY_%s\s+(\d+)" % n, src).group(1))
                                             for n in ("PACKED", "COMPRESSED"))
    # the shared runtime pieces come from the hash library, not from copies; no
    # other ECDSA library is needed
    needed = subprocess.check_output(["readelf", "-d", SO]).decode()
    assert "liblcb_hash_gpu.so" in needed and "$ORIGIN" in needed
    assert len(re.findall(r"NEEDED.*liblcb_", needed)) == 1
    undefined = subprocess.check_output(["nm", "-D", "--undefined-only", SO]).decode()
    for sym in ("ensure_init", "map_err"):
        assert re.search(r" U _ZN6lcbgpu\d+%s" % sym, undefined), sym


def test_package_exports(K):
    import liblcb_amd
    from liblcb_amd import _lib, ecdsa, ecdsa_dh, ecdsa_sign
    assert liblcb_amd.ecdsa_key is K and liblcb_amd.ecdsa_key_lib is K.ecdsa_key_lib is _lib.ecdsa_key_lib
    assert "ecdsa_key" in liblcb_amd.__all__ and "ecdsa_key_lib" in liblcb_amd.__all__
    assert len({K.LIB_PATH, ecdsa.LIB_PATH, ecdsa_sign.LIB_PATH, ecdsa_dh.LIB_PATH}) == 4
    # the other three modules' lists are their own headers', unchanged
    assert len(ecdsa.ECDSA_SIGNATURES) == 7 and len(ecdsa_sign.ECDSA_SIGN_SIGNATURES) == 9
    assert len(ecdsa_dh.ECDSA_DH_SIGNATURES) == 3 and len(K.ECDSA_KEY_SIGNATURES) == 6
    mine = {n for n, _, _ in K.ECDSA_KEY_SIGNATURES}
    assert not mine & {n for n, _, _ in ecdsa.ECDSA_SIGNATURES + ecdsa_sign.ECDSA_SIGN_SIGNATURES +
                       ecdsa_dh.ECDSA_DH_SIGNATURES}
    for fn in ("import_batch", "export_batch", "verify_wire"):
        assert callable(getattr(K, fn)) and fn in K.__all__
    with pytest.raises(ValueError):
        K.import_batch("secp384r1", np.zeros(33, np.uint8), key_size=33)
    with pytest.raises(ValueError):
        K.export_batch(1, np.zeros(64, np.uint8), form=2)


def test_argument_errors(K, L):
    buf = np.zeros(256, np.uint8)
    outb = np.full(256, 0x5A, np.uint8)
    st = np.full(4, 777, np.int32)
    inf = np.full(4, 0x5A, np.uint8)
    szs = np.full(4, 33, np.uint32)
    b, o, s, f, z = buf.ctypes.data, outb.ctypes.data, st.ctypes.data, inf.ctypes.data, szs.ctypes.data

    def imp(curve=1, le=0, keys=b, stride=33, sizes=None, size=33, keys_y=None, count=2, pub=o, infinity=f, status=s,
            flags=0):
        return L.lcb_ecdsa_key_import_batch(curve, le, keys, stride, sizes, size, keys_y, count, pub, infinity, status,
                                            flags, None)

    def exp(curve=1, le=0, form=1, pub=b, infinity=None, count=2, out=o, stride=80, sizes=z, status=s, flags=0):
        return L.lcb_ecdsa_key_export_batch(curve, le, form, pub, infinity, count, out, stride, sizes, status, flags,
                                            None)

    # all EINVAL before touching HIP
    assert imp(curve=10) == EINVAL and imp(curve=-1) == EINVAL
    assert imp(flags=0x10) == EINVAL and imp(flags=0x3) == EINVAL
    assert imp(keys=None) == EINVAL and imp(pub=None) == EINVAL and imp(status=None) == EINVAL
    assert imp(count=1 << 32) == EINVAL and imp(stride=1 << 32) == EINVAL
    assert imp(count=0) == 0 and imp(count=0, keys=None, pub=None, infinity=None, status=None) == 0
    assert exp(curve=10) == EINVAL and exp(curve=-1) == EINVAL
    assert exp(flags=0x10) == EINVAL and exp(flags=0x3) == EINVAL
    assert exp(form=2) == EINVAL and exp(form=-1) == EINVAL
    assert exp(form=1, stride=32) == EINVAL and exp(form=0, stride=64) == EINVAL and exp(form=0, stride=33) == EINVAL
    assert exp(stride=0) == EINVAL
    assert exp(pub=None) == EINVAL and exp(out=None) == EINVAL and exp(sizes=None) == EINVAL
    assert exp(status=None) == EINVAL
    assert exp(count=1 << 32) == EINVAL and exp(stride=1 << 32) == EINVAL
    assert exp(count=0) == 0 and exp(count=0, pub=None, out=None, sizes=None, status=None) == 0
    assert exp(count=0, stride=0) == EINVAL                       # the stride is checked first
    for le in ("be", "le"):
        fi, fe = getattr(L, "ecdsa_pub_key_import_%s_batch" % le), getattr(L, "ecdsa_pub_key_export_%s_batch" % le)
        assert fi(10, b, 33, None, 33, None, 2, o, f, s, 0, None) == EINVAL
        assert fi(1, None, 33, None, 33, None, 2, o, f, s, 0, None) == EINVAL
        assert fi(1, b, 33, None, 33, None, 2, o, f, s, 0x10, None) == EINVAL
        assert fi(1, b, 33, None, 33, None, 0, o, f, s, 0, None) == 0
        assert fe(10, 1, b, None, 2, o, 33, z, s, 0, None) == EINVAL
        assert fe(1, 1, b, None, 2, o, 32, z, s, 0, None) == EINVAL
        assert fe(1, 0, b, None, 2, o, 64, z, s, 0, None) == EINVAL
        assert fe(1, 5, b, None, 2, o, 32, z, s, 0, None) == EINVAL   # compress != 0: the compressed form
        assert fe(1, 0, b, None, 0, o, 65, z, s, 0, None) == 0
    assert (st == 777).all() and (outb == 0x5A).all() and (inf == 0x5A).all() and (szs == 33).all()
    with pytest.raises(ValueError):
        K.import_batch(1, buf[:65], key_size=33, count=3)         # fewer keys than items
    with pytest.raises(ValueError):
        K.import_batch(1, buf[:66], key_stride=33, sizes=szs[:3])
    with pytest.raises(ValueError):
        K.import_batch(1, buf[:66])                               # neither a stride nor a size
    with pytest.raises(ValueError):
        K.export_batch(1, buf[:128], count=3)


def test_fails_loudly_without_gpu(K, L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import liblcb_amd
    buf = np.zeros(160, np.uint8)
    outb = np.full(160, 0x5A, np.uint8)
    st = np.full(2, 777, np.int32)
    szs = np.full(2, 99, np.uint32)
    b, o, s, z = buf.ctypes.data, outb.ctypes.data, st.ctypes.data, szs.ctypes.data
    for le in ("be", "le"):
        assert getattr(L, "ecdsa_pub_key_import_%s_batch" % le)(1, b, 33, None, 33, None, 2, o, None, s, 0,
                                                                None) == errno.ENODEV
        assert getattr(L, "ecdsa_pub_key_export_%s_batch" % le)(1, 1, b, None, 2, o, 33, z, s, 0,
                                                                None) == errno.ENODEV
    assert (st == 777).all() and (outb == 0x5A).all() and (szs == 99).all()   # no CPU answer
    with pytest.raises(liblcb_amd.LcbHashError):
        K.import_batch("secp256r1", buf[:66], key_size=33)
    with pytest.raises(liblcb_amd.LcbHashError):
        K.export_batch("secp256r1", buf[:128])
    with pytest.raises(liblcb_amd.LcbHashError):
        K.verify_wire("secp256r1", buf[:64], buf[:128], buf[:66], key_size=33)


def test_missing_library_raises_not_falls_back(K, monkeypatch):
    import liblcb_amd
    from liblcb_amd import _lib
    monkeypatch.setattr(_lib, "_keylib", None)
    monkeypatch.setattr(_lib, "ECDSA_KEY_LIB_PATH", os.path.join(LIBDIR, "no_such_liblcb_ecdsa_key_gpu.so"))
    z = np.zeros(66, np.uint8)
    with pytest.raises(liblcb_amd.LcbHashError):
        liblcb_amd.ecdsa_key_lib()
    with pytest.raises(liblcb_amd.LcbHashError):
        K.import_batch(1, z, key_size=33)
    with pytest.raises(liblcb_amd.LcbHashError):
        K.export_batch(1, z[:64])


def test_kernels_use_no_scratch_and_no_lds():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.kernels(SO)
    assert sorted(r["name"].split("(")[0] for r in rows) == ["lcbec::ecdsa_key_export_kernel",
                                                             "lcbec::ecdsa_key_import_kernel"], rows
    assert all(r["scratch"] == 0 and r["lds"] == 0 for r in rows), [(r["name"], r["scratch"], r["lds"]) for r in rows]
    # two waves per SIMD need at most 256 registers per lane
    assert all(r["vgpr"] <= 256 for r in rows), [(r["name"], r["vgpr"]) for r in rows]
    # the kernels are in this library only
    for other in (None, "liblcb_ecdsa_gpu.so", "liblcb_ecdsa_sign_gpu.so", "liblcb_ecdsa_dh_gpu.so"):
        there = [r["name"] for r in (kernel_resources.kernels(os.path.join(LIBDIR, other)) if other
                                     else kernel_resources.kernels())]
        assert there and not [n for n in there if "ecdsa_key_import" in n or "ecdsa_key_export" in n], other


def test_c_caller_links(tmp_path):
    exe = str(tmp_path / "ecdsa_key_caller")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "ecdsa_key_caller.c"), "-o", exe,
                           "-L" + LIBDIR, "-llcb_ecdsa_key_gpu", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath-link," + LIBDIR + ":/opt/rocm/lib"])
    assert subprocess.check_output([exe]).decode().strip() == "ok"
