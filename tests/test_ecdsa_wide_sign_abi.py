"""liblcb_ecdsa_wide_sign_gpu.so (include/lcb_ecdsa_wide_sign_gpu.h): builds,
loads after liblcb_hash_gpu.so, exports every declared symbol, refuses bad
arguments before touching HIP, fails loudly (never on the CPU) where no MI355X
is visible, and its four kernels use neither scratch nor LDS within the
register counts DESIGN.md 5l reports."""
import errno
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lcb_ecdsa_wide_sign_gpu.h")
LIBDIR = os.path.join(ROOT, "liblcb_amd")
SO = os.path.join(LIBDIR, "liblcb_ecdsa_wide_sign_gpu.so")
EINVAL = errno.EINVAL

# registers per lane (architectural VGPRs + AGPRs) and scratch
# bytes per lane of the four kernels, __launch_bounds__(64, 1).
PINS = {"ecdsa_wide_sign_kernel_384": {"vgpr": 256, "agpr": 39, "scratch": 0},
        "ecdsa_wide_sign_kernel_512": {"vgpr": 256, "agpr": 135, "scratch": 0},
        "ecdsa_wide_keys_kernel_384": {"vgpr": 256, "agpr": 17, "scratch": 0},
        "ecdsa_wide_keys_kernel_512": {"vgpr": 256, "agpr": 109, "scratch": 0}}


@pytest.fixture(scope="module")
def S():
    from liblcb_amd import ecdsa_wide_sign
    return ecdsa_wide_sign


@pytest.fixture(scope="module")
def L(S):
    return S.ecdsa_wide_sign_lib()


def exported(so):
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    return set(l.split()[-1] for l in out.splitlines() if " T " in l)


def test_exports_every_declared_symbol(S, L):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b([a-z_0-9]+)\(", src)) - {"defined", "sizeof"})
    assert len(names) == 9, names
    assert not [n for n in names if n not in exported(SO)]
    assert sorted(n for n, _, _ in S.ECDSA_WIDE_SIGN_SIGNATURES) == names
    # the shared runtime pieces come from the hash library, not from copies;
    # the hash library is the only one of the project's that is linked
    needed = subprocess.check_output(["readelf", "-d", SO]).decode()
    assert "$ORIGIN" in needed
    assert re.findall(r"NEEDED.*\[(liblcb_[a-z0-9_]+\.so)\]", needed) == ["liblcb_hash_gpu.so"]
    undefined = subprocess.check_output(["nm", "-D", "--undefined-only", SO]).decode()
    for sym in ("ensure_init", "map_err"):
        assert re.search(r" U _ZN6lcbgpu\d+%s" % sym, undefined), sym


def test_the_other_libraries_keep_their_exports():
    """The wide verification library has 8 functions, the 256-bit signing
    library 9, and none of them is the new library's."""
    from liblcb_amd import ecdsa_sign, ecdsa_wide, ecdsa_wide_sign
    new = {n for n, _, _ in ecdsa_wide_sign.ECDSA_WIDE_SIGN_SIGNATURES}
    for mod_names, so, count in (
            ([n for n, _, _ in ecdsa_wide.ECDSA_WIDE_SIGNATURES], "liblcb_ecdsa_wide_gpu.so", 8),
            ([n for n, _, _ in ecdsa_sign.ECDSA_SIGN_SIGNATURES], "liblcb_ecdsa_sign_gpu.so", 9)):
        funcs = {n for n in exported(os.path.join(LIBDIR, so)) if not n.startswith("_")}
        assert funcs == set(mod_names) and len(funcs) == count, (so, sorted(funcs))
        assert not funcs & new
    assert {n for n in exported(SO) if not n.startswith("_")} == new


def test_package_exports(S):
    import liblcb_amd
    from liblcb_amd import ecdsa_sign, ecdsa_wide
    assert liblcb_amd.ecdsa_wide_sign is S and liblcb_amd.ecdsa_wide_sign_lib is S.ecdsa_wide_sign_lib
    assert "ecdsa_wide_sign" in liblcb_amd.__all__ and "ecdsa_wide_sign_lib" in liblcb_amd.__all__
    assert len({S.LIB_PATH, ecdsa_wide.LIB_PATH, ecdsa_sign.LIB_PATH}) == 3
    for fn in ("sign_batch", "key_gen_batch", "pub_key_batch", "sign_messages"):
        assert callable(getattr(S, fn)) and fn in S.__all__
    z = np.zeros(64, np.uint8)
    for bad in ("secp256r1", "secp521r1", 6, -1):  # curve names and ids are ecdsa_wide's
        with pytest.raises(ValueError):
            S.sign_batch(bad, z, z, z)
        with pytest.raises(ValueError):
            S.key_gen_batch(bad, z)
        with pytest.raises(ValueError):
            S.pub_key_batch(bad, z)


def test_argument_errors(S, L):
    buf = np.zeros(512, np.uint8)
    outb = np.full(512, 0x5A, np.uint8)
    st = np.full(4, 777, np.int32)
    idx = np.zeros(4, np.uint32)
    b, o, s, i = buf.ctypes.data, outb.ctypes.data, st.ctypes.data, idx.ctypes.data

    def sg(curve=0, le=0, hashes=b, hash_size=48, priv=b, nkeys=2, key_idx=None, rnd=b, count=2, sigs=o, status=s,
           flags=0):
        return L.lcb_ecdsa_wide_sign_batch(curve, le, hashes, hash_size, priv, nkeys, key_idx, rnd, count, sigs,
                                           status, flags, None)

    # all EINVAL before touching HIP
    assert sg(curve=6) == EINVAL and sg(curve=-1) == EINVAL
    assert sg(hash_size=0) == EINVAL and sg(hash_size=129) == EINVAL
    assert sg(curve=3, hash_size=0) == EINVAL and sg(curve=3, hash_size=129) == EINVAL
    assert sg(flags=0x10) == EINVAL and sg(flags=0x3) == EINVAL
    assert sg(hashes=None) == EINVAL and sg(priv=None) == EINVAL and sg(rnd=None) == EINVAL
    assert sg(sigs=None) == EINVAL and sg(status=None) == EINVAL
    assert sg(nkeys=1) == EINVAL and sg(nkeys=3) == EINVAL        # key_idx == NULL needs nkeys == count
    assert sg(count=1 << 32, nkeys=1 << 32) == EINVAL
    assert sg(count=2, nkeys=1 << 32, key_idx=i) == EINVAL
    assert sg(count=0, nkeys=0) == 0 and sg(count=0, nkeys=3, key_idx=i) == 0   # empty batch
    assert sg(count=0, nkeys=0, hash_size=128) == 0 and sg(count=0, nkeys=0, hash_size=1) == 0
    assert sg(count=0, nkeys=0, hashes=None, priv=None, rnd=None, sigs=None, status=None) == 0
    for name in ("ecdsa_sign_be_wide_batch", "ecdsa_sign_le_wide_batch"):
        fn = getattr(L, name)
        assert fn(6, b, 48, b, 2, None, b, 2, o, s, 0, None) == EINVAL, name
        assert fn(2, b, 64, b, 3, None, b, 2, o, s, 0, None) == EINVAL, name
        assert fn(2, b, 129, b, 2, None, b, 2, o, s, 0, None) == EINVAL, name
        assert fn(2, b, 64, b, 0, None, b, 0, o, s, 0, None) == 0, name

    def kg(fn=L.lcb_ecdsa_wide_key_gen_batch, head=(0, 0), rnd=b, count=2, priv=o, pub=o + 128, status=s, flags=0):
        return fn(*head, rnd, count, priv, pub, status, flags, None)

    def pk(fn=L.lcb_ecdsa_wide_pub_key_batch, head=(0, 0), priv=b, count=2, pub=o, status=s, flags=0):
        return fn(*head, priv, count, pub, status, flags, None)

    for call, variants in ((kg, (("lcb_ecdsa_wide_key_gen_batch", 2), ("ecdsa_key_gen_be_wide_batch", 1),
                                 ("ecdsa_key_gen_le_wide_batch", 1))),
                           (pk, (("lcb_ecdsa_wide_pub_key_batch", 2),
                                 ("ecdsa_recover_pub_key_from_priv_key_be_wide_batch", 1),
                                 ("ecdsa_recover_pub_key_from_priv_key_le_wide_batch", 1)))):
        for name, nhead in variants:
            fn = getattr(L, name)
            for cid in (0, 3):  # one curve per limb count
                ok, bad, neg = ((cid, 0), (6, 0), (-1, 0)) if nhead == 2 else ((cid,), (6,), (-1,))
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
        S.sign_batch(0, buf[:258], buf[:96], buf[:96], hash_size=129)
    with pytest.raises(LcbHashError):
        S.sign_batch(0, buf[:96], buf[:96], buf[:96], hash_size=0)
    with pytest.raises(ValueError):
        S.sign_batch(0, buf[:96], buf[:48], buf[:96])             # fewer keys than items
    with pytest.raises(ValueError):
        S.sign_batch(2, buf[:64], buf[:128], buf[:128])           # fewer hashes than items
    with pytest.raises(ValueError):
        S.pub_key_batch(2, buf[:64], count=2)


def test_fails_loudly_without_gpu(S, L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import liblcb_amd
    buf = np.zeros(256, np.uint8)
    outb = np.full(512, 0x5A, np.uint8)
    st = np.full(2, 777, np.int32)
    b, o, s = buf.ctypes.data, outb.ctypes.data, st.ctypes.data
    for curve, B in ((0, 48), (3, 64)):
        for name in ("ecdsa_sign_be_wide_batch", "ecdsa_sign_le_wide_batch"):
            assert getattr(L, name)(curve, b, B, b, 2, None, b, 2, o, s, 0, None) == errno.ENODEV
        for name in ("ecdsa_key_gen_be_wide_batch", "ecdsa_key_gen_le_wide_batch"):
            assert getattr(L, name)(curve, b, 2, o, o + 128, s, 0, None) == errno.ENODEV
        for name in ("ecdsa_recover_pub_key_from_priv_key_be_wide_batch",
                     "ecdsa_recover_pub_key_from_priv_key_le_wide_batch"):
            assert getattr(L, name)(curve, b, 2, o, s, 0, None) == errno.ENODEV
    assert (st == 777).all() and (outb == 0x5A).all()             # no CPU answer
    with pytest.raises(liblcb_amd.LcbHashError):
        S.sign_batch("secp384r1", buf[:96], buf[:96], buf[:96])
    with pytest.raises(liblcb_amd.LcbHashError):
        S.key_gen_batch("brainpoolP512r1", buf[:128])
    with pytest.raises(liblcb_amd.LcbHashError):
        S.pub_key_batch("id-tc26-gost-3410-12-512-paramSetA", buf[:128], le=True)


def test_missing_library_raises_not_falls_back(S, monkeypatch):
    import liblcb_amd
    monkeypatch.setattr(S, "_wslib", None)
    monkeypatch.setattr(S, "LIB_PATH", os.path.join(LIBDIR, "no_such_liblcb_ecdsa_wide_sign_gpu.so"))
    z = np.zeros(48, np.uint8)
    with pytest.raises(liblcb_amd.LcbHashError):
        S.sign_batch(0, z, z, z)
    with pytest.raises(liblcb_amd.LcbHashError):
        S.key_gen_batch(0, z)
    with pytest.raises(liblcb_amd.LcbHashError):
        S.pub_key_batch(0, z)


def kernel_tools():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    return kernel_resources


def agpr_counts(so_path):
    """{mangled kernel name: .agpr_count} from the gfx950 code objects' notes."""
    kernel_resources = kernel_tools()
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for k, co in enumerate(kernel_resources.code_objects(so_path)):
            path = os.path.join(td, "%d.co" % k)
            open(path, "wb").write(co)
            txt = subprocess.run([kernel_resources.READELF, "--notes", path], capture_output=True, text=True,
                                 check=True).stdout
            # the keys of a kernel's mapping are sorted: .agpr_count opens it, .name follows
            for agpr, name in re.findall(r"\.agpr_count:\s+(\d+)\n.*?\n\s+\.name:\s+(\S+)", txt, flags=re.S):
                out[name] = int(agpr)
    return out


def test_kernel_resources_are_those_of_the_design_note():
    kernel_resources = kernel_tools()
    rows = kernel_resources.kernels(SO)
    assert len(rows) == 4, [r["name"] for r in rows]
    agpr = agpr_counts(SO)
    for key, pin in PINS.items():
        k = next(r for r in rows if key in r["name"])
        # vgpr_count of the notes is the lane's whole allocation, architectural + accumulation
        assert k["scratch"] == pin["scratch"] == 0, (key, k["scratch"])
        assert k["lds"] == 0
        assert agpr[k["mangled"]] == pin["agpr"], (key, agpr[k["mangled"]])
        assert k["vgpr"] - agpr[k["mangled"]] == pin["vgpr"], (key, k["vgpr"])
        assert k["vgpr"] <= 512                                   # one wave per SIMD
    # the wide signing kernels are in this library only
    for other in ("liblcb_hash_gpu.so", "liblcb_ecdsa_sign_gpu.so", "liblcb_ecdsa_wide_gpu.so"):
        there = [r["name"] for r in kernel_resources.kernels(os.path.join(LIBDIR, other))]
        assert there and not [n for n in there if "wide_sign" in n or "wide_keys" in n], other
    # and no other kernel is in this one
    assert not [r["name"] for r in rows if "wide_sign" not in r["name"] and "wide_keys" not in r["name"]]


def test_c_caller_links(tmp_path):
    exe = str(tmp_path / "ecdsa_wide_sign_caller")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "ecdsa_wide_sign_caller.c"), "-o", exe,
                           "-L" + LIBDIR, "-llcb_ecdsa_wide_sign_gpu", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath-link," + LIBDIR + ":/opt/rocm/lib"])
    assert subprocess.check_output([exe]).decode().strip() == "ok"
