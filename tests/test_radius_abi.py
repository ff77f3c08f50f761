"""liblcb_radius_gpu.so (include/lcb_radius_gpu.h): builds, loads after
liblcb_hash_gpu.so, exports every declared symbol, takes its runtime pieces
and keyed batches from the hash library, refuses bad arguments before
touching HIP, fails loudly (never on the CPU) where no MI355X is visible, and
none of its kernels uses scratch."""
import errno
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lcb_radius_gpu.h")
LIBDIR = os.path.join(ROOT, "liblcb_amd")
SO = os.path.join(LIBDIR, "liblcb_radius_gpu.so")
E = errno.EINVAL


@pytest.fixture(scope="module")
def RB():
    from liblcb_amd import radius_batch
    return radius_batch


@pytest.fixture(scope="module")
def L(RB):
    return RB.radius_lib()


def test_exports_every_declared_symbol(RB, L):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b([a-z_0-9]+)\(", src)) - {"defined", "sizeof"})
    assert names == ["radius_pkt_sign_batch", "radius_pkt_verify_batch"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", SO]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert not [n for n in names if n not in exported]
    assert sorted(n for n, _, _ in RB.RADIUS_SIGNATURES) == names
    # the shared runtime pieces and the keyed batches come from the hash library, not from copies
    needed = subprocess.check_output(["readelf", "-d", SO]).decode()
    assert "liblcb_hash_gpu.so" in needed and "$ORIGIN" in needed
    undefined = subprocess.check_output(["nm", "-D", "--undefined-only", SO]).decode()
    for sym in ("ensure_init", "map_err", "scratch_alloc", "scratch_free", "parallel_copy"):
        assert re.search(r" U _ZN6lcbgpu\d+%s" % sym, undefined), sym
    assert re.search(r" U lcb_hash_batch_keyed\b", undefined)
    assert "md_keyed_kernel" not in out and "lcb_hash_batch_keyed" not in exported


def test_package_exports(RB):
    import liblcb_amd
    assert liblcb_amd.radius_batch is RB and liblcb_amd.radius_lib is RB.radius_lib
    blob, offs, sizes = RB.pack([b"abc", b"", b"defgh"], gaps=[2, 1, 0], fill=0x5A)
    assert offs.tolist() == [2, 6, 6] and sizes.tolist() == [3, 0, 5] and blob.size == 11
    assert RB.unpack(blob, offs, sizes) == [b"abc", b"", b"defgh"] and blob[0] == 0x5A
    rh = RB.req_headers([None, bytes(range(30))])
    assert rh.size == 40 and not rh[:20].any() and bytes(rh[20:]) == bytes(range(20))
    with pytest.raises(ValueError):
        RB.req_headers([b"short"])


def _calls(L):
    pk = np.zeros(128, np.uint8)
    key = np.frombuffer(b"testing123", np.uint8).copy()
    klen = np.array([10], np.uint32)
    err = np.full(2, -1, np.int32)
    req = np.zeros(40, np.uint8)
    base = dict(pkts=pk.ctypes.data, offsets=None, buf_sizes=None, count=2, stride=64, fixed_size=64,
                keys=key.ctypes.data, key_offsets=None, key_lengths=klen.ctypes.data, nkeys=1, key_index=None,
                errors=err.ctypes.data, flags=0, stream=None)
    order = ["pkts", "offsets", "buf_sizes", "count", "stride", "fixed_size", "keys", "key_offsets", "key_lengths",
             "nkeys", "key_index"]

    def sign(**kw):
        a = dict(base, **kw)
        return L.radius_pkt_sign_batch(*([a[k] for k in order] + [a["errors"], a["flags"], a["stream"]]))

    def verify(**kw):
        a = dict(base, **kw)
        return L.radius_pkt_verify_batch(*([a[k] for k in order] +
                                           [a.get("req_hdrs", req.ctypes.data), a["errors"], a["flags"], a["stream"]]))
    return sign, verify, (pk, key, klen, err, req)


def test_argument_errors(L):
    sign, verify, keep = _calls(L)
    for fn in (sign, verify):
        # all EINVAL before touching HIP
        assert fn(pkts=None) == E and fn(errors=None) == E and fn(keys=None) == E
        assert fn(nkeys=0) == E and fn(key_lengths=None) == E
        assert fn(flags=0x10) == E and fn(flags=0x3) == E
        assert fn(fixed_size=19) == E and fn(fixed_size=0) == E
        assert fn(stride=63) == E and fn(stride=0) == E
        assert fn(count=0) == 0 and fn(count=0, stride=0) == 0       # empty batch
    assert keep[3].tolist() == [-1, -1]                               # errors untouched


def test_fails_loudly_without_gpu(RB, L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import liblcb_amd
    sign, verify, keep = _calls(L)
    assert sign() == errno.ENODEV and verify() == errno.ENODEV and verify(req_hdrs=None) == errno.ENODEV
    assert sign(stride=63, count=1) == errno.ENODEV                   # one packet: stride is not read
    pk = np.zeros(128, np.uint8)
    for fn in (RB.sign_packed, RB.verify_packed):
        with pytest.raises(liblcb_amd.LcbHashError) as e:
            fn(pk, [b"testing123"], count=2, stride=64, fixed_size=64)
        assert e.value.errno == errno.ENODEV


def test_missing_library_raises_not_falls_back(RB, monkeypatch):
    import liblcb_amd
    monkeypatch.setattr(RB, "_rlib", None)
    monkeypatch.setattr(RB, "LIB_PATH", os.path.join(LIBDIR, "no_such_liblcb_radius_gpu.so"))
    with pytest.raises(liblcb_amd.LcbHashError):
        RB.sign_packed(np.zeros(64, np.uint8), [b"k"], count=1, stride=64, fixed_size=64)


def test_host_wrapper_validation(RB):
    """Descriptions the C-ABI would read out of range are refused before it is called."""
    pk = np.zeros(8 * 64, np.uint8)
    offs = np.arange(8, dtype=np.uint64) * 64
    bsz = np.full(8, 64, np.uint32)
    K = [b"k"]
    with pytest.raises((TypeError, ValueError)):
        RB.sign_packed(bytes(8 * 64), K, count=8, stride=64, fixed_size=64)       # not writable in place
    with pytest.raises((TypeError, ValueError)):
        RB.sign_packed(pk.astype(np.int32), K, count=8, stride=64, fixed_size=64)
    with pytest.raises(ValueError):
        RB.sign_packed(pk, K, offsets=offs[:4], buf_sizes=bsz)
    with pytest.raises(ValueError):
        RB.sign_packed(pk, K, offsets=offs + 1, buf_sizes=bsz)                    # runs past the blob
    with pytest.raises(ValueError):
        RB.sign_packed(pk, K, key_index=np.zeros(3, np.uint32), offsets=offs, buf_sizes=bsz)
    with pytest.raises(ValueError):
        RB.verify_packed(pk, K, offsets=offs, buf_sizes=bsz, req_hdrs=np.zeros(20, np.uint8))


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.kernels(SO)
    names = [r["name"] for r in rows]
    for want in ("radius_parse_kernel", "radius_password_kernel", "radius_mid_kernel", "radius_fin_kernel"):
        assert sum(want in n for n in names) == 2, (want, names)      # sign and verify
    assert len(rows) == 8
    assert all(r["scratch"] == 0 and r["lds"] == 0 for r in rows), [(r["name"], r["scratch"], r["lds"]) for r in rows]
    # the walk and the fix-up kernels are latency-bound: small enough for full occupancy
    assert all(r["vgpr"] <= 32 for r in rows if "password" not in r["name"])
    assert all(r["vgpr"] <= 128 for r in rows)
    # the RADIUS kernels are in this library only
    hash_names = [r["name"] for r in kernel_resources.kernels()]
    assert hash_names and not [n for n in hash_names if "radius" in n.lower()]


def test_c_caller_links(tmp_path):
    exe = str(tmp_path / "radius_caller")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "radius_caller.c"), "-o", exe,
                           "-L" + LIBDIR, "-llcb_radius_gpu", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath-link," + LIBDIR + ":/opt/rocm/lib"])
    assert subprocess.check_output([exe]).decode().strip() == "ok"
