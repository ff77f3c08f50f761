"""liblcb_ecdsa_sign_gpu.so (include/lcb_ecdsa_sign_gpu.h): builds, loads
after liblcb_hash_gpu.so, exports every declared symbol, refuses bad
arguments before touching HIP, fails loudly (never on the CPU) where no MI355X
is visible, and its kernels use neither scratch nor LDS."""
import errno
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lcb_ecdsa_sign_gpu.h")
LIBDIR = os.path.join(ROOT, "liblcb_amd")
SO = os.path.join(LIBDIR, "liblcb_ecdsa_sign_gpu.so")
EINVAL = errno.EINVAL


@pytest.fixture(scope="module")
def S():
    from liblcb_amd import ecdsa_sign
    return ecdsa_sign


@pytest.fixture(scope="module")
def L(S):
    return S.ecdsa_sign_lib()


def test_exports_every_declared_symbol(S, L):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b([a-z_0-9]+)\(", src)) - {"defined", "sizeof"})
    assert len(names) == 9, names
    out = subprocess.check_output(["nm", "-D", "--defined-only", SO]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert not [n for n in names if n not in exported]
    assert sorted(n for n, _, _ in S.ECDSA_SIGN_SIGNATURES) == names
    # the shared runtime pieces come from the hash library, not from copies; the
    # verification library is not needed
    needed = subprocess.check_output(["readelf", "-d", SO]).decode()
    assert "liblcb_hash_gpu.so" in needed and "$ORIGIN" in needed and "liblcb_ecdsa_gpu.so" not in needed
    undefined = subprocess.check_output(["nm", "-D", "--undefined-only", SO]).decode()
    for sym in ("ensure_init", "map_err"):
        assert re.search(r" U _ZN6lcbgpu\d+%s" % sym, undefined), sym


def test_package_exports(S):
    import liblcb_amd
    from liblcb_amd import ecdsa
    assert liblcb_amd.ecdsa_sign is S and liblcb_amd.ecdsa_sign_lib is S.ecdsa_sign_lib
    assert "ecdsa_sign" in liblcb_amd.__all__ and "ecdsa_sign_lib" in liblcb_amd.__all__
    assert S.LIB_PATH != ecdsa.LIB_PATH
    # the verification module's list is its own header's, unchanged
    assert len(ecdsa.ECDSA_SIGNATURES) == 7
    assert not {n for n, _, _ in ecdsa.ECDSA_SIGNATURES} & {n for n, _, _ in S.ECDSA_SIGN_SIGNATURES}
    for fn in ("sign_batch", "key_gen_batch", "pub_key_batch", "sign_messages"):
        assert callable(getattr(S, fn)) and fn in S.__all__
    with pytest.raises(ValueError):
        S.sign_batch("secp384r1", np.zeros(32, np.uint8), np.zeros(32, np.uint8), np.zeros(32, np.uint8))


def test_argument_errors(S, L):
    buf = np.zeros(256, np.uint8)
    outb = np.full(256, 0x5A, np.uint8)
    st = np.full(4, 777, np.int32)
    idx = np.zeros(4, np.uint32)
    b, o, s, i = buf.ctypes.data, outb.ctypes.data, st.ctypes.data, idx.ctypes.data

    def sg(curve=1, le=0, hashes=b, hash_size=32, priv=b, nkeys=2, key_idx=None, rnd=b, count=2, sigs=o, status=s,
           flags=0):
        return L.lcb_ecdsa_sign_batch(curve, le, hashes, hash_size, priv, nkeys, key_idx, rnd, count, sigs, status,
                                      flags, None)

    # all EINVAL before touching HIP
    assert sg(curve=10) == EINVAL and sg(curve=-1) == EINVAL
    assert sg(hash_size=0) == EINVAL and sg(hash_size=65) == EINVAL
    assert sg(flags=0x10) == EINVAL and sg(flags=0x3) == EINVAL
    assert sg(hashes=None) == EINVAL and sg(priv=None) == EINVAL and sg(rnd=None) == EINVAL
    assert sg(sigs=None) == EINVAL and sg(status=None) == EINVAL
    assert sg(nkeys=1) == EINVAL and sg(nkeys=3) == EINVAL        # key_idx == NULL needs nkeys == count
    assert sg(count=1 << 32, nkeys=1 << 32) == EINVAL
    assert sg(count=2, nkeys=1 << 32, key_idx=i) == EINVAL
    assert sg(count=0, nkeys=0) == 0 and sg(count=0, nkeys=3, key_idx=i) == 0   # empty batch
    assert sg(count=0, nkeys=0, hashes=None, priv=None, rnd=None, sigs=None, status=None) == 0
    for name in ("ecdsa_sign_be_batch", "ecdsa_sign_le_batch"):
        fn = getattr(L, name)
        assert fn(10, b, 32, b, 2, None, b, 2, o, s, 0, None) == EINVAL, name
        assert fn(1, b, 32, b, 3, None, b, 2, o, s, 0, None) == EINVAL, name
        assert fn(1, b, 32, b, 0, None, b, 0, o, s, 0, None) == 0, name

    def kg(fn=L.lcb_ecdsa_key_gen_batch, head=(1, 0), rnd=b, count=2, priv=o, pub=o + 64, status=s, flags=0):
        return fn(*head, rnd, count, priv, pub, status, flags, None)

    def pk(fn=L.lcb_ecdsa_pub_key_batch, head=(1, 0), priv=b, count=2, pub=o, status=s, flags=0):
        return fn(*head, priv, count, pub, status, flags, None)

    for call, variants in ((kg, (("lcb_ecdsa_key_gen_batch", 2), ("ecdsa_key_gen_be_batch", 1),
                                 ("ecdsa_key_gen_le_batch", 1))),
                           (pk, (("lcb_ecdsa_pub_key_batch", 2), ("ecdsa_recover_pub_key_from_priv_key_be_batch", 1),
                                 ("ecdsa_recover_pub_key_from_priv_key_le_batch", 1)))):
        for name, nhead in variants:
            fn = getattr(L, name)
            ok, bad, neg = ((1, 0), (10, 0), (-1, 0)) if nhead == 2 else ((1,), (10,), (-1,))
            assert call(fn, bad) == EINVAL and call(fn, neg) == EINVAL, name
            assert call(fn, ok, flags=0x10) == EINVAL and call(fn, ok, flags=0x3) == EINVAL, name
            assert call(fn, ok, count=1 << 32) == EINVAL, name
            assert call(fn, ok, pub=None) == EINVAL and call(fn, ok, status=None) == EINVAL, name
            assert call(fn, ok, count=0) == 0, name
    assert kg(rnd=None) == EINVAL and kg(priv=None) == EINVAL
    assert pk(priv=None) == EINVAL
    assert kg(count=0, rnd=None, priv=None, pub=None, status=None) == 0
    assert pk(count=0, priv=None, pub=None, status=None) == 0
    assert (st == 777).all() and (outb == 0x5A).all()             # nothing was written
    from liblcb_amd import LcbHashError
    with pytest.raises(LcbHashError):
        S.sign_batch(1, buf[:128], buf[:64], buf[:64], hash_size=65)
    with pytest.raises(ValueError):
        S.sign_batch(1, buf[:64], buf[:32], buf[:64])             # fewer keys than items
    with pytest.raises(ValueError):
        S.sign_batch(1, buf[:32], buf[:64], buf[:64])             # fewer hashes than items
    with pytest.raises(ValueError):
        S.pub_key_batch(1, buf[:32], count=2)


def test_fails_loudly_without_gpu(S, L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import liblcb_amd
    buf = np.zeros(128, np.uint8)
    outb = np.full(256, 0x5A, np.uint8)
    st = np.full(2, 777, np.int32)
    b, o, s = buf.ctypes.data, outb.ctypes.data, st.ctypes.data
    for name in ("ecdsa_sign_be_batch", "ecdsa_sign_le_batch"):
        assert getattr(L, name)(1, b, 32, b, 2, None, b, 2, o, s, 0, None) == errno.ENODEV
    for name in ("ecdsa_key_gen_be_batch", "ecdsa_key_gen_le_batch"):
        assert getattr(L, name)(1, b, 2, o, o + 64, s, 0, None) == errno.ENODEV
    for name in ("ecdsa_recover_pub_key_from_priv_key_be_batch", "ecdsa_recover_pub_key_from_priv_key_le_batch"):
        assert getattr(L, name)(1, b, 2, o, s, 0, None) == errno.ENODEV
    assert (st == 777).all() and (outb == 0x5A).all()             # no CPU answer
    with pytest.raises(liblcb_amd.LcbHashError):
        S.sign_batch("secp256r1", buf[:64], buf[:64], buf[:64])
    with pytest.raises(liblcb_amd.LcbHashError):
        S.key_gen_batch("secp256r1", buf[:64])
    with pytest.raises(liblcb_amd.LcbHashError):
        S.pub_key_batch("secp256r1", buf[:64])


def test_missing_library_raises_not_falls_back(S, monkeypatch):
    import liblcb_amd
    monkeypatch.setattr(S, "_slib", None)
    monkeypatch.setattr(S, "LIB_PATH", os.path.join(LIBDIR, "no_such_liblcb_ecdsa_sign_gpu.so"))
    z = np.zeros(32, np.uint8)
    with pytest.raises(liblcb_amd.LcbHashError):
        S.sign_batch(1, z, z, z)
    with pytest.raises(liblcb_amd.LcbHashError):
        S.key_gen_batch(1, z)
    with pytest.raises(liblcb_amd.LcbHashError):
        S.pub_key_batch(1, z)


def test_kernels_use_no_scratch_and_no_lds():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.kernels(SO)
    names = [r["name"] for r in rows]
    assert any("ecdsa_sign_kernel" in n for n in names) and any("ecdsa_keys_kernel" in n for n in names), names
    assert all(r["scratch"] == 0 and r["lds"] == 0 for r in rows), [(r["name"], r["scratch"], r["lds"]) for r in rows]
    # two waves per SIMD need at most 256 registers per lane
    assert all(r["vgpr"] <= 256 for r in rows), [(r["name"], r["vgpr"]) for r in rows]
    # the signing kernels are in this library only
    for other in (None, os.path.join(LIBDIR, "liblcb_ecdsa_gpu.so")):
        there = [r["name"] for r in (kernel_resources.kernels(other) if other else kernel_resources.kernels())]
        assert there and not [n for n in there if "ecdsa_sign" in n or "ecdsa_keys" in n], other


def test_c_caller_links(tmp_path):
    exe = str(tmp_path / "ecdsa_sign_caller")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "ecdsa_sign_caller.c"), "-o", exe,
                           "-L" + LIBDIR, "-llcb_ecdsa_sign_gpu", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath-link," + LIBDIR + ":/opt/rocm/lib"])
    assert subprocess.check_output([exe]).decode().strip() == "ok"
