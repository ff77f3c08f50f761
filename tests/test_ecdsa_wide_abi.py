"""liblcb_ecdsa_wide_gpu.so (include/lcb_ecdsa_wide_gpu.h): builds, loads
after liblcb_hash_gpu.so, exports every declared symbol, refuses bad arguments
before touching HIP, fails loudly (never on the CPU) where no MI355X is
visible, and its two kernels use no scratch within the register counts
DESIGN.md 5k reports."""
import errno
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lcb_ecdsa_wide_gpu.h")
LIBDIR = os.path.join(ROOT, "liblcb_amd")
SO = os.path.join(LIBDIR, "liblcb_ecdsa_wide_gpu.so")

# registers per lane (architectural VGPRs + AGPRs) and scratch
# bytes per lane of the two kernels, __launch_bounds__(64, 1).
PINS = {"ecdsa_wide_verify_kernel_384": {"vgpr": 256, "agpr": 51, "scratch": 0},
        "ecdsa_wide_verify_kernel_512": {"vgpr": 256, "agpr": 137, "scratch": 0}}


@pytest.fixture(scope="module")
def W():
    from liblcb_amd import ecdsa_wide
    return ecdsa_wide


@pytest.fixture(scope="module")
def L(W):
    return W.ecdsa_wide_lib()


def test_exports_every_declared_symbol(W, L):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b([a-z_0-9]+)\(", src)) - {"defined", "sizeof"})
    assert len(names) == 8, names
    out = subprocess.check_output(["nm", "-D", "--defined-only", SO]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert not [n for n in names if n not in exported]
    assert sorted(n for n, _, _ in W.ECDSA_WIDE_SIGNATURES) == names
    # the shared runtime pieces come from the hash library, not from copies;
    # none of the 256-bit ECDSA libraries is linked
    needed = subprocess.check_output(["readelf", "-d", SO]).decode()
    assert "liblcb_hash_gpu.so" in needed and "$ORIGIN" in needed and "liblcb_ecdsa" not in needed.replace(
        "liblcb_ecdsa_wide_gpu.so", "")
    undefined = subprocess.check_output(["nm", "-D", "--undefined-only", SO]).decode()
    for sym in ("ensure_init", "map_err"):
        assert re.search(r" U _ZN6lcbgpu\d+%s" % sym, undefined), sym


def test_package_exports(W):
    import liblcb_amd
    assert liblcb_amd.ecdsa_wide is W and liblcb_amd.ecdsa_wide_lib is W.ecdsa_wide_lib
    assert "ecdsa_wide_lib" in liblcb_amd.__all__ and "ecdsa_wide" in liblcb_amd.__all__
    assert len(W.CURVES) == 6 and W.curve_id("secp384r1") == 0 and W.curve_id(4) == 4
    assert W.curve_id("id-tc26-gost-3410-2012-512-paramSetTest") == 5
    assert [W.curve_bytes(i) for i in range(6)] == [48, 48, 64, 64, 64, 64]
    for bad in ("secp256r1", "secp521r1", 6, -1):
        with pytest.raises(ValueError):
            W.curve_id(bad)
    # the 256-bit library keeps its ten curves
    assert len(liblcb_amd.ecdsa.CURVES) == 10 and liblcb_amd.ecdsa_lib().lcb_ecdsa_curve_count() == 10


def test_argument_errors(W, L):
    EINVAL = errno.EINVAL
    buf = np.zeros(512, np.uint8)
    st = np.full(4, 777, np.int32)
    idx = np.zeros(4, np.uint32)
    b, s, i = buf.ctypes.data, st.ctypes.data, idx.ctypes.data

    def v(curve=0, le=0, hashes=b, hash_size=48, sigs=b, keys=b, nkeys=2, key_idx=None, count=2, status=s, flags=0):
        return L.lcb_ecdsa_wide_verify_batch(curve, le, hashes, hash_size, sigs, keys, nkeys, key_idx, count, status,
                                             flags, None)

    # all EINVAL before touching HIP
    assert v(curve=6) == EINVAL and v(curve=-1) == EINVAL
    assert v(hash_size=0) == EINVAL and v(hash_size=129) == EINVAL
    assert v(curve=3, hash_size=0) == EINVAL and v(curve=3, hash_size=129) == EINVAL
    assert v(hashes=None) == EINVAL and v(sigs=None) == EINVAL and v(keys=None) == EINVAL
    assert v(status=None) == EINVAL
    assert v(nkeys=1) == EINVAL and v(nkeys=3) == EINVAL          # key_idx == NULL needs nkeys == count
    assert v(flags=0x10) == EINVAL and v(flags=0x3) == EINVAL
    assert v(count=1 << 32, nkeys=1 << 32) == EINVAL
    assert v(count=0, nkeys=0) == 0 and v(count=0, nkeys=3, key_idx=i) == 0   # empty batch
    assert v(count=0, nkeys=0, hash_size=128) == 0 and v(count=0, nkeys=0, hash_size=1) == 0
    assert v(count=0, nkeys=0, hashes=None, sigs=None, keys=None, status=None) == 0
    for name in ("ecdsa_verify_be_wide_batch", "ecdsa_verify_le_wide_batch"):
        fn = getattr(L, name)
        assert fn(6, b, 48, b, b, 2, None, 2, s, 0, None) == EINVAL, name
        assert fn(2, b, 64, b, b, 3, None, 2, s, 0, None) == EINVAL, name
        assert fn(2, b, 129, b, b, 2, None, 2, s, 0, None) == EINVAL, name
        assert fn(2, b, 64, b, b, 0, None, 0, s, 0, None) == 0, name
    assert (st == 777).all()                                       # nothing was written
    out = (np.zeros(384, np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.uint32))
    p, a, h = (x.ctypes.data for x in out)
    assert L.lcb_ecdsa_wide_curve_params(6, p, a, h) == EINVAL
    assert L.lcb_ecdsa_wide_curve_params(0, None, a, h) == EINVAL
    assert L.lcb_ecdsa_wide_curve_params(0, p, None, h) == EINVAL
    assert L.lcb_ecdsa_wide_curve_params(0, p, a, None) == EINVAL
    from liblcb_amd import LcbHashError
    with pytest.raises(LcbHashError):
        W.verify_batch(0, buf[:258], buf[:192], buf[:192], hash_size=129)
    with pytest.raises(ValueError):
        W.verify_batch(0, buf[:96], buf[:192], buf[:96])          # fewer keys than items
    with pytest.raises(ValueError):
        W.verify_batch(2, buf[:64], buf[:256], buf[:256])         # fewer hashes than items


def test_fails_loudly_without_gpu(W, L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import liblcb_amd
    buf = np.zeros(256, np.uint8)
    st = np.full(2, 777, np.int32)
    for name in ("ecdsa_verify_be_wide_batch", "ecdsa_verify_le_wide_batch"):
        for curve, hs in ((0, 48), (3, 64)):
            assert getattr(L, name)(curve, buf.ctypes.data, hs, buf.ctypes.data, buf.ctypes.data, 2, None, 2,
                                    st.ctypes.data, 0, None) == errno.ENODEV
    assert (st == 777).all()                                       # no CPU answer
    with pytest.raises(liblcb_amd.LcbHashError):
        W.verify_batch("secp384r1", buf[:96], buf[:192], buf[:192])


def test_missing_library_raises_not_falls_back(W, monkeypatch):
    import liblcb_amd
    monkeypatch.setattr(W, "_wlib", None)
    monkeypatch.setattr(W, "LIB_PATH", os.path.join(LIBDIR, "no_such_liblcb_ecdsa_wide_gpu.so"))
    with pytest.raises(liblcb_amd.LcbHashError):
        W.verify_batch(0, np.zeros(48, np.uint8), np.zeros(96, np.uint8), np.zeros(96, np.uint8))


def agpr_counts(so_path):
    """{mangled kernel name: .agpr_count} from the gfx950 code objects' notes."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
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
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.kernels(SO)
    assert len(rows) == 2, [r["name"] for r in rows]
    agpr = agpr_counts(SO)
    for key, pin in PINS.items():
        k = next(r for r in rows if key in r["name"])
        # vgpr_count of the notes is the lane's whole allocation, architectural + accumulation
        assert k["scratch"] == pin["scratch"] == 0, (key, k["scratch"])
        assert k["lds"] == 0
        assert agpr[k["mangled"]] == pin["agpr"], (key, agpr[k["mangled"]])
        assert k["vgpr"] - agpr[k["mangled"]] == pin["vgpr"], (key, k["vgpr"])
        assert k["vgpr"] <= 512                                   # one wave per SIMD
    # never above the naive instantiation of ecdsa_math.hpp: 112 B at 12 limbs, 160 B at 16
    assert all(r["scratch"] <= lim for r, lim in zip(sorted(rows, key=lambda r: r["name"]), (112, 160)))
    # the wide kernels are in this library only
    for other in ("liblcb_hash_gpu.so", "liblcb_ecdsa_gpu.so"):
        assert not [r["name"] for r in kernel_resources.kernels(os.path.join(LIBDIR, other)) if "wide" in r["name"]]
    # and the 256-bit kernel is not in this one
    assert not [r["name"] for r in rows if "wide" not in r["name"]]


def test_c_caller_links(tmp_path):
    exe = str(tmp_path / "ecdsa_wide_caller")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "ecdsa_wide_caller.c"), "-o", exe,
                           "-L" + LIBDIR, "-llcb_ecdsa_wide_gpu", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath-link," + LIBDIR + ":/opt/rocm/lib"])
    assert subprocess.check_output([exe]).decode().strip() == "ok"
