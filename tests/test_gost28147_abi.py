"""liblcb_gost28147_gpu.so (include/lcb_gost28147_gpu.h): builds, loads after
liblcb_hash_gpu.so, exports every declared symbol, refuses bad arguments
before touching HIP, fails loudly (never on the CPU) where no MI355X is
visible, and none of its kernels uses scratch."""
import errno
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lcb_gost28147_gpu.h")
LIBDIR = os.path.join(ROOT, "liblcb_amd")
SO = os.path.join(LIBDIR, "liblcb_gost28147_gpu.so")


@pytest.fixture(scope="module")
def G():
    from liblcb_amd import gost28147
    return gost28147


@pytest.fixture(scope="module")
def L(G):
    return G.gost28147_lib()


def test_exports_every_declared_symbol(G, L):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b([a-z_0-9]+)\(", src)) - {"defined", "sizeof"})
    assert len(names) == 11, names
    out = subprocess.check_output(["nm", "-D", "--defined-only", SO]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert not [n for n in names if n not in exported]
    assert sorted(n for n, _, _ in G.GOST28147_SIGNATURES) == names
    # the shared runtime pieces come from the hash library, not from copies
    needed = subprocess.check_output(["readelf", "-d", SO]).decode()
    assert "liblcb_hash_gpu.so" in needed and "$ORIGIN" in needed
    undefined = subprocess.check_output(["nm", "-D", "--undefined-only", SO]).decode()
    for sym in ("ensure_init", "map_err", "scratch_alloc", "scratch_free", "parallel_copy"):
        assert re.search(r" U _ZN6lcbgpu\d+%s" % sym, undefined), sym


def test_package_exports(G):
    import liblcb_amd
    assert liblcb_amd.gost28147 is G and liblcb_amd.gost28147_lib is G.gost28147_lib
    assert [G.SBOX_TEST, G.SBOX_CRYPTOPRO_A, G.SBOX_CRYPTOPRO_D, G.SBOX_TC26_Z] == [0, 1, 4, 5]
    assert len(G.sbox(G.SBOX_TC26_Z)) == 128 and max(G.sbox(G.SBOX_TC26_Z)) == 15
    assert len(set(G.sbox(i) for i in range(6))) == 6


def test_argument_errors(G, L):
    key = np.zeros(32, np.uint8)
    buf = np.zeros(64, np.uint8)
    mac = np.zeros(8, np.uint8)
    sb = np.frombuffer(G.sbox(0), np.uint8).copy()
    k, b, s, m = key.ctypes.data, buf.ctypes.data, sb.ctypes.data, mac.ctypes.data
    E = errno.EINVAL

    def crypt(op=0, be=0, key=k, key_size=32, sbox=s, src=b, dst=b, count=1, fixed_len=64, flags=0):
        return L.lcb_gost28147_crypt_batch(op, be, key, key_size, sbox, src, dst, None, None, count, 0, fixed_len,
                                           flags, None)

    def macb(key=k, key_size=32, sbox=s, data=b, count=1, fixed_len=64, macs=m, mac_size=8, flags=0):
        return L.lcb_gost28147_mac_batch(0, key, key_size, sbox, data, None, None, count, 0, fixed_len, macs,
                                         mac_size, flags, None)

    # all EINVAL before touching HIP
    assert crypt(key_size=16) == E and crypt(key_size=0) == E and crypt(key_size=33) == E
    assert crypt(sbox=None) == E and crypt(key=None) == E and crypt(dst=None) == E and crypt(src=None) == E
    assert crypt(fixed_len=60) == E and crypt(fixed_len=4) == E
    assert crypt(flags=0x10) == E and crypt(op=2) == E
    assert macb(key_size=31) == E and macb(sbox=None) == E and macb(key=None) == E and macb(macs=None) == E
    assert macb(fixed_len=12) == E and macb(flags=0x2) == E
    assert macb(mac_size=0) == E and macb(mac_size=9) == E
    bad = sb.copy()
    bad[77] = 16
    assert crypt(sbox=bad.ctypes.data) == E and macb(sbox=bad.ctypes.data) == E
    for name in ("gost28147_blocks_encrypt_batch", "gost28147_blocks_encrypt_be_batch",
                 "gost28147_blocks_decrypt_batch", "gost28147_blocks_decrypt_be_batch"):
        assert getattr(L, name)(k, 32, s, b, b, None, None, 1, 0, 63, 0, None) == E, name
        assert getattr(L, name)(k, 256, s, b, b, None, None, 0, 0, 64, 0, None) == 0, name  # empty batch
    for name in ("gost28147_blocks_mac_batch", "gost28147_blocks_mac_be_batch"):
        assert getattr(L, name)(k, 32, s, b, None, None, 1, 0, 64, m, 9, 0, None) == E, name
        assert getattr(L, name)(k, 256, s, b, None, None, 0, 0, 64, m, 8, 0, None) == 0, name
    with pytest.raises(ValueError):
        G.encrypt_batch(bytes(31), buf, sbox=0, count=1, fixed_len=64)
    with pytest.raises(ValueError):
        G.mac_batch(bytes(32), buf, sbox=bytes(127), count=1, fixed_len=64)


def test_fails_loudly_without_gpu(G, L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import liblcb_amd
    key = np.zeros(32, np.uint8)
    buf = np.zeros(64, np.uint8)
    sb = np.frombuffer(G.sbox(5), np.uint8).copy()
    assert L.gost28147_blocks_encrypt_batch(key.ctypes.data, 32, sb.ctypes.data, buf.ctypes.data, buf.ctypes.data,
                                            None, None, 1, 0, 64, 0, None) == errno.ENODEV
    assert L.gost28147_blocks_mac_batch(key.ctypes.data, 32, sb.ctypes.data, buf.ctypes.data, None, None, 1, 0, 64,
                                        buf.ctypes.data, 8, 0, None) == errno.ENODEV
    for fn in (G.encrypt_batch, G.decrypt_batch, G.mac_batch):
        with pytest.raises(liblcb_amd.LcbHashError):
            fn(bytes(32), buf, sbox=5, count=1, fixed_len=64)


def test_missing_library_raises_not_falls_back(G, monkeypatch):
    import liblcb_amd
    monkeypatch.setattr(G, "_glib", None)
    monkeypatch.setattr(G, "LIB_PATH", os.path.join(LIBDIR, "no_such_liblcb_gost28147_gpu.so"))
    with pytest.raises(liblcb_amd.LcbHashError):
        G.encrypt_batch(bytes(32), np.zeros(64, np.uint8), sbox=5, count=1, fixed_len=64)


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.kernels(SO)
    names = [r["name"] for r in rows]
    for want in ("gost28147_ecb_kernel", "gost28147_mac_kernel", "gost28147_table_kernel",
                 "gost28147_scan_final"):
        assert any(want in n for n in names), (want, names)
    assert all(r["scratch"] == 0 for r in rows), [(r["name"], r["scratch"]) for r in rows if r["scratch"]]
    by = {n: r for n, r in zip(names, rows)}
    ecb = next(r for n, r in by.items() if "gost28147_ecb_kernel" in n)
    mac = next(r for n, r in by.items() if "gost28147_mac_kernel" in n)
    # 32 lane-private copies of the 256-word table; 5 workgroups per CU
    assert ecb["lds"] == 32768 and mac["lds"] == 32768
    assert ecb["vgpr"] <= 64 and mac["vgpr"] <= 64
    # the cipher's kernels are in this library only
    hash_names = [r["name"] for r in kernel_resources.kernels()]
    assert not [n for n in hash_names if "gost28147" in n]


def test_c_caller_links(tmp_path):
    exe = str(tmp_path / "gost28147_caller")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "gost28147_caller.c"), "-o", exe,
                           "-L" + LIBDIR, "-llcb_gost28147_gpu", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath-link," + LIBDIR + ":/opt/rocm/lib"])
    assert subprocess.check_output([exe]).decode().strip() == "ok"
