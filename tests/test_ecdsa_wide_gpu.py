"""Batched ECDSA / GOST R 34.10-2012 verification on 384- and 512-bit curves
on the MI355X (include/lcb_ecdsa_wide_gpu.h) against the reference-generated
fixture tests/golden/ecdsa_wide.json (every status there is what the
reference returned) and, for signatures the tests make themselves, the
Python-int model tests/ecdsa_wide_model.py (itself pinned to that fixture on
the CPU).

One lane verifies one signature, so the shapes that matter are counts around
the 64-lane wave (1, 63, 64, 65, 129) with accepted and rejected items
sharing a wave, every hash size the import treats differently (1, 20, B - 1,
B, B + 1, 64, 65, 128), both byte orders, both limb counts, and the key table
with a bad index.  A 512-bit wave takes tens of milliseconds, so no batch
here is larger than a few hundred items."""
import errno
import os
import random
import subprocess

import numpy as np
import pytest

from tests import ecdsa_wide_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "liblcb_amd")
FX = M.load_fixture()
CURVES = M.load_curves(FX)
GROUP_IDS = ["%s-%s" % (g["curve"], "le" if g["le"] else "be") for g in FX["cases"]]
GUARD = 0xA5


@pytest.fixture(scope="module")
def W(gpu):
    from liblcb_amd import ecdsa_wide
    ecdsa_wide.ecdsa_wide_lib()
    return ecdsa_wide


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


def u8(h):
    return np.frombuffer(bytes.fromhex(h), np.uint8).copy()


def pack(recs, hash_size):
    """(hashes, sigs, keys, statuses) of records that share one hash_size."""
    hashes = u8("".join(k["hash"][:2 * hash_size] for k in recs))
    sigs = u8("".join(k["r"] + k["s"] for k in recs))
    keys = u8("".join(k["Qx"] + k["Qy"] for k in recs))
    return hashes, sigs, keys, np.array([k["status"] for k in recs], np.int32)


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def group(name, le):
    return next(g for g in FX["cases"] if g["curve"] == name and g["le"] == le)


@pytest.mark.parametrize("grp", FX["cases"], ids=GROUP_IDS)
def test_every_fixture_status_in_both_memory_modes(W, torch_, grp):
    torch = torch_
    seen = 0
    for hs in sorted({k["hash_size"] for k in grp["records"]}):
        recs = [k for k in grp["records"] if k["hash_size"] == hs]
        hashes, sigs, keys, want = pack(recs, hs)
        got = W.verify_batch(grp["curve"], dev(torch, hashes), dev(torch, sigs), dev(torch, keys), le=grp["le"],
                             hash_size=hs)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        bad = [(k["name"], int(g), int(w)) for k, g, w in zip(recs, got, want) if g != w]
        assert not bad, ("device", hs, bad)
        host = W.verify_batch(grp["curve"], hashes, sigs, keys, le=grp["le"], hash_size=hs)
        assert isinstance(host, np.ndarray) and host.dtype == np.int32
        bad = [(k["name"], int(g), int(w)) for k, g, w in zip(recs, host, want) if g != w]
        assert not bad, ("host", hs, bad)
        seen += len(recs)
    assert seen == len(grp["records"])
    assert {1, 20, 64, 65, 128} <= {k["hash_size"] for k in grp["records"]}


@pytest.mark.parametrize("grp", FX["cases"], ids=GROUP_IDS)
def test_mixed_batches_around_the_wave(W, torch_, grp):
    """Accepted and rejected items interleaved, repeated cyclically: a lane
    that leaves early (-1, EINVAL) shares its wave with lanes that run the
    whole ladder, and the last wave is partial; statuses compared position by
    position."""
    torch = torch_
    B = CURVES[grp["curve"]]["bytes"]
    recs = [k for k in grp["records"] if k["hash_size"] == B]
    assert {0, -1, -2, errno.EINVAL} <= {k["status"] for k in recs}
    h1, s1, k1, w1 = pack(recs, B)
    for count in (1, 63, 64, 65, 129):
        # start each count at another record, so that lane 0 is not always "valid"
        idx = (np.arange(count) + count) % len(recs)
        hashes, sigs, keys = h1.reshape(-1, B)[idx], s1.reshape(-1, 2 * B)[idx], k1.reshape(-1, 2 * B)[idx]
        got = W.verify_batch(grp["curve"], dev(torch, hashes.reshape(-1)), dev(torch, sigs.reshape(-1)),
                             dev(torch, keys.reshape(-1)), le=grp["le"])
        torch.cuda.synchronize()
        assert got.shape == (count,) and got.dtype == torch.int32
        got = got.cpu().numpy()
        assert np.array_equal(got, w1[idx]), (count, np.nonzero(got != w1[idx])[0][:8])


@pytest.mark.parametrize("name,le", [("brainpoolP384r1", False), ("id-tc26-gost-3410-12-512-paramSetB", True)])
def test_key_table_and_bad_index(W, torch_, name, le):
    """Three keys addressed through key_idx: repeated, out of order, and two
    indices past the table (EINVAL, no key read)."""
    torch = torch_
    c = CURVES[name]
    B = c["bytes"]
    rng = random.Random(31)
    ds = [rng.randrange(1, c["n"]) for _ in range(3)]
    Qs = [M.public_key(c, d) for d in ds]
    table = np.frombuffer(b"".join(M.to_bytes(c, q[0], le) + M.to_bytes(c, q[1], le) for q in Qs), np.uint8).copy()
    n = 70
    kidx = np.array([2, 2, 0, 1, 0] + [rng.randrange(3) for _ in range(n - 5)], np.uint32)
    signer = kidx.copy()
    signer[5] = (signer[5] + 1) % 3        # signed by another key of the table: -2
    kidx[17] = 3                           # the first index past the table
    kidx[40] = 0xFFFFFFFF
    hashes, sigs = [], []
    for i in range(n):
        h = bytes(rng.randrange(256) for _ in range(B))
        r, s = M.sign(c, h, B, ds[signer[i]], rng.randrange(1, 1 << (8 * B)), le)
        hashes.append(h)
        sigs.append(M.to_bytes(c, r, le) + M.to_bytes(c, s, le))
    hashes = np.frombuffer(b"".join(hashes), np.uint8).copy()
    sigs = np.frombuffer(b"".join(sigs), np.uint8).copy()
    want = np.zeros(n, np.int32)
    want[5] = -2
    want[[17, 40]] = errno.EINVAL
    for as_int32 in (False, True):
        di = dev(torch, kidx.view(np.int32) if as_int32 else kidx)
        got = W.verify_batch(name, dev(torch, hashes), dev(torch, sigs), dev(torch, table), key_idx=di, le=le)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(W.verify_batch(name, hashes, sigs, table, key_idx=kidx, le=le), want)
    # the same items with one key per item: the bad indices get key 0, which did not sign them
    flat = table.reshape(3, 2 * B)[np.where(kidx < 3, kidx, 0)].reshape(-1)
    want2 = want.copy()
    for i in (17, 40):
        want2[i] = 0 if signer[i] == 0 else -2
    got = W.verify_batch(name, dev(torch, hashes), dev(torch, sigs), dev(torch, flat), le=le)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want2)


@pytest.mark.parametrize("grp", FX["messages"], ids=lambda g: "%s-%s" % (g["alg"], g["curve"]))
def test_verify_messages(W, torch_, oracle, grp):
    """The natural pairs: the stored messages digested on the device and
    verified without leaving it; the statuses are the reference's, which
    signed the digest of the message before every second one was altered."""
    torch = torch_
    recs = grp["records"]
    msgs = [bytes.fromhex(k["msg"]) for k in recs]
    lens = np.array([len(m) for m in msgs], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    data = np.frombuffer(b"".join(msgs), np.uint8).copy()
    # the oracle digests the stored message to the stored hash
    digests = oracle.batch(grp["alg_id"], data, offs, lens)
    assert [d.tobytes().hex() for d in digests] == [k["hash"] for k in recs]
    sigs = u8("".join(k["r"] + k["s"] for k in recs))
    keys = u8("".join(k["Qx"] + k["Qy"] for k in recs))
    want = np.array([k["status"] for k in recs], np.int32)
    assert set(want) == {0, -2}
    d = lambda a: dev(torch, a)  # noqa: E731
    got = W.verify_messages(grp["curve"], grp["alg_id"], d(data), d(sigs), d(keys), offsets=d(offs.astype(np.int64)),
                            lengths=d(lens.astype(np.int32)), le=grp["le"])
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    # host memory goes the same way
    assert np.array_equal(W.verify_messages(grp["curve"], grp["alg_id"], data, sigs, keys, offsets=offs,
                                            lengths=lens, le=grp["le"]), want)


@pytest.mark.parametrize("name,le,which", [("secp384r1", False, "1"), ("secp384r1", False, "B"),
                                           ("secp384r1", False, "128"),
                                           ("id-tc26-gost-3410-12-512-paramSetA", True, "1"),
                                           ("id-tc26-gost-3410-12-512-paramSetA", True, "B"),
                                           ("id-tc26-gost-3410-12-512-paramSetA", True, "128")])
def test_canaries_after_status_and_inputs(W, torch_, name, le, which):
    """Nothing past status[count - 1] is written and no input byte changes;
    the hashes are packed at hash_size, so for 1 they are unaligned."""
    torch = torch_
    c = CURVES[name]
    B = c["bytes"]
    hs = B if which == "B" else int(which)
    base = [k for k in group(name, le)["records"] if k["hash_size"] == B]
    count = 67
    # the records' B hash bytes, zero-extended to 128, imported at another size:
    # those statuses come from the model (pinned to the fixture on the CPU)
    ext = [dict(k, hash=k["hash"] + "00" * (128 - B)) for k in base]
    wants = np.array([k["status"] if hs == B else
                      M.verify(c, bytes.fromhex(k["hash"]), hs, bytes.fromhex(k["r"]), bytes.fromhex(k["s"]),
                               bytes.fromhex(k["Qx"]), bytes.fromhex(k["Qy"]), le) for k in ext], np.int32)
    pick = np.arange(count) % len(ext)
    hashes, sigs, keys, _ = pack([ext[i] for i in pick], hs)
    want = wants[pick]
    tail = np.full(48, GUARD, np.uint8)
    bufs = [dev(torch, np.concatenate([a, tail])) for a in (hashes, sigs, keys)]
    before = [b.clone() for b in bufs]
    out = torch.full((count + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    got = W.verify_batch(name, bufs[0], bufs[1], bufs[2], le=le, hash_size=hs, count=count, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and np.array_equal(got.cpu().numpy(), want)
    assert (out[count:] == 0x5A5A5A5A).all().item()
    for b, a in zip(before, bufs):
        assert torch.equal(b, a)
    # host mode: the same through numpy, status guarded, inputs unchanged
    hout = np.full(count + 16, 0x5A5A5A5A, np.int32)
    copies = [a.copy() for a in (hashes, sigs, keys)]
    W.verify_batch(name, hashes, sigs, keys, le=le, hash_size=hs, count=count, out=hout)
    assert np.array_equal(hout[:count], want) and (hout[count:] == 0x5A5A5A5A).all()
    for b, a in zip(copies, (hashes, sigs, keys)):
        assert np.array_equal(b, a)


def test_async_on_the_current_stream(W, torch_):
    """Device mode enqueues on torch's current stream: inputs written by an
    earlier kernel of that stream are seen, and a side stream is honoured."""
    torch = torch_
    grp = group("brainpoolP512r1", False)
    recs = [k for k in grp["records"] if k["hash_size"] == 64]
    hashes, sigs, keys, want = pack(recs, 64)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dh = torch.zeros(hashes.size, dtype=torch.uint8, device="cuda:0")
        dh.copy_(dev(torch, hashes))                 # enqueued on s, ahead of the verify
        got = W.verify_batch("brainpoolP512r1", dh, dev(torch, sigs), dev(torch, keys))
    s.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)


def test_c_caller_verifies_one_case_per_curve(W, tmp_path):
    exe = str(tmp_path / "ecdsa_wide_caller")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "ecdsa_wide_caller.c"), "-o", exe,
                           "-L" + LIBDIR, "-llcb_ecdsa_wide_gpu", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath-link," + LIBDIR + ":/opt/rocm/lib"])
    lines, want = [], []
    for i, grp in enumerate(FX["cases"]):
        # a valid one per group, and a rejected one of a kind that changes with the group
        for k in (grp["records"][0], grp["records"][3 + i % 12]):
            lines.append("%s %d %d %s %s %s %s %s" % (grp["curve"], k["le"], k["hash_size"], k["hash"], k["r"],
                                                      k["s"], k["Qx"], k["Qy"]))
            want.append(str(k["status"]))
    assert {g["curve"] for g in FX["cases"]} == set(CURVES)
    out = subprocess.run([exe, "verify"], input="\n".join(lines).encode(), stdout=subprocess.PIPE, check=True)
    assert out.stdout.decode().split() == want
