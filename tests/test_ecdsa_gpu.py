"""Batched ECDSA / GOST R 34.10 verification on the MI355X
(include/lcb_ecdsa_gpu.h) against the reference-generated fixture
tests/golden/ecdsa.json (every status there is what the reference returned)
and, for signatures the tests make themselves, the Python-int model
tests/ecdsa_model.py (itself pinned to that fixture on the CPU).

One lane verifies one signature, so the shapes that matter are counts around
the 64-lane wave (1, 63, 64, 65, 257) with accepted and rejected items
sharing a wave, every hash size the import treats differently (1, 20, 32,
33, 64), both byte orders, and the key table with a bad index."""
import errno
import os
import random
import subprocess

import numpy as np
import pytest

from tests import ecdsa_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "liblcb_amd")
FX = M.load_fixture()
CURVES = M.load_curves(FX)
GROUP_IDS = ["%s-%s" % (g["curve"], "le" if g["le"] else "be") for g in FX["cases"]]
GUARD = 0xA5


@pytest.fixture(scope="module")
def E(gpu):
    from liblcb_amd import ecdsa
    ecdsa.ecdsa_lib()
    return ecdsa


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


@pytest.mark.parametrize("grp", FX["cases"], ids=GROUP_IDS)
def test_every_fixture_status_in_both_memory_modes(E, torch_, grp):
    torch = torch_
    seen = 0
    for hs in sorted({k["hash_size"] for k in grp["records"]}):
        recs = [k for k in grp["records"] if k["hash_size"] == hs]
        hashes, sigs, keys, want = pack(recs, hs)
        got = E.verify_batch(grp["curve"], dev(torch, hashes), dev(torch, sigs), dev(torch, keys), le=grp["le"],
                             hash_size=hs)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        bad = [(k["name"], int(g), int(w)) for k, g, w in zip(recs, got, want) if g != w]
        assert not bad, ("device", hs, bad)
        host = E.verify_batch(grp["curve"], hashes, sigs, keys, le=grp["le"], hash_size=hs)
        assert isinstance(host, np.ndarray) and host.dtype == np.int32
        bad = [(k["name"], int(g), int(w)) for k, g, w in zip(recs, host, want) if g != w]
        assert not bad, ("host", hs, bad)
        seen += len(recs)
    assert seen == len(grp["records"])


@pytest.mark.parametrize("grp", FX["cases"], ids=GROUP_IDS)
def test_mixed_batches_around_the_wave(E, torch_, grp):
    """Accepted and rejected items interleaved, repeated cyclically: a lane
    that leaves early (-1, EINVAL) shares its wave with lanes that run the
    whole ladder; statuses compared position by position."""
    torch = torch_
    recs = [k for k in grp["records"] if k["hash_size"] == 32]
    assert {0, -1, -2, errno.EINVAL} <= {k["status"] for k in recs}
    h1, s1, k1, w1 = pack(recs, 32)
    for count in (1, 63, 64, 65, 257):
        # start each count at another record, so that lane 0 is not always "valid"
        idx = (np.arange(count) + count) % len(recs)
        hashes, sigs, keys = h1.reshape(-1, 32)[idx], s1.reshape(-1, 64)[idx], k1.reshape(-1, 64)[idx]
        got = E.verify_batch(grp["curve"], dev(torch, hashes.reshape(-1)), dev(torch, sigs.reshape(-1)),
                             dev(torch, keys.reshape(-1)), le=grp["le"])
        torch.cuda.synchronize()
        assert got.shape == (count,) and got.dtype == torch.int32
        got = got.cpu().numpy()
        assert np.array_equal(got, w1[idx]), (count, np.nonzero(got != w1[idx])[0][:8])


@pytest.mark.parametrize("name,le", [("secp256k1", False), ("id-gostR3410-2001-CryptoPro-B-ParamSet", True)])
def test_key_table_and_bad_index(E, torch_, name, le):
    torch = torch_
    c = CURVES[name]
    rng = random.Random(31)
    ds = [rng.randrange(1, c["n"]) for _ in range(3)]
    Qs = [M.public_key(c, d) for d in ds]
    table = np.frombuffer(b"".join(M.to_bytes(q[0], le) + M.to_bytes(q[1], le) for q in Qs), np.uint8).copy()
    n = 70
    kidx = np.array([rng.randrange(3) for _ in range(n)], np.uint32)
    signer = kidx.copy()
    signer[5] = (signer[5] + 1) % 3        # signed by another key of the table: -2
    kidx[17] = 3                           # the first index past the table
    kidx[40] = 0xFFFFFFFF
    hashes, sigs = [], []
    for i in range(n):
        h = bytes(rng.randrange(256) for _ in range(32))
        r, s = M.sign(c, h, 32, ds[signer[i]], rng.randrange(1, 1 << 256), le)
        hashes.append(h)
        sigs.append(M.to_bytes(r, le) + M.to_bytes(s, le))
    hashes = np.frombuffer(b"".join(hashes), np.uint8).copy()
    sigs = np.frombuffer(b"".join(sigs), np.uint8).copy()
    want = np.zeros(n, np.int32)
    want[5] = -2
    want[[17, 40]] = errno.EINVAL
    for as_int32 in (False, True):
        di = dev(torch, kidx.view(np.int32) if as_int32 else kidx)
        got = E.verify_batch(name, dev(torch, hashes), dev(torch, sigs), dev(torch, table), key_idx=di, le=le)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(E.verify_batch(name, hashes, sigs, table, key_idx=kidx, le=le), want)
    # the same items with one key per item: the bad indices get key 0, which did not sign them
    flat = table.reshape(3, 64)[np.where(kidx < 3, kidx, 0)].reshape(-1)
    want2 = want.copy()
    for i in (17, 40):
        want2[i] = 0 if signer[i] == 0 else -2
    got = E.verify_batch(name, dev(torch, hashes), dev(torch, sigs), dev(torch, flat), le=le)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want2)
    assert np.array_equal(E.verify_batch(name, hashes, sigs, flat, le=le), want2)


@pytest.mark.parametrize("name,alg,le", [("secp256r1", "sha256", False),
                                         ("id-gostR3410-2001-CryptoPro-A-ParamSet", "gost256", True)])
def test_verify_messages(E, torch_, oracle, name, alg, le):
    """64 ragged messages of 0..300 bytes signed by the model over the
    oracle's digests; every second message then has one byte altered."""
    import liblcb_amd
    torch = torch_
    c = CURVES[name]
    alg_id = liblcb_amd.ALG_IDS[alg]
    rng = random.Random(64)
    n = 64
    lens = np.array([0, 300, 1, 299] + [rng.randrange(301) for _ in range(n - 4)], np.uint32)
    lens[1::2] = np.maximum(lens[1::2], 1)            # the altered ones need a byte to alter
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    data = np.frombuffer(bytes(rng.randrange(256) for _ in range(int(lens.sum()))), np.uint8).copy()
    digests = oracle.batch(alg_id, data, offs, lens)
    ds = [rng.randrange(1, c["n"]) for _ in range(4)]
    Qs = [M.public_key(c, d) for d in ds]
    table = np.frombuffer(b"".join(M.to_bytes(q[0], le) + M.to_bytes(q[1], le) for q in Qs), np.uint8).copy()
    kidx = np.arange(n, dtype=np.uint32) % 4
    sigs = []
    for i in range(n):
        r, s = M.sign(c, digests[i].tobytes(), 32, ds[kidx[i]], rng.randrange(1, 1 << 256), le)
        sigs.append(M.to_bytes(r, le) + M.to_bytes(s, le))
    sigs = np.frombuffer(b"".join(sigs), np.uint8).copy()
    altered = data.copy()
    for i in range(1, n, 2):
        altered[int(offs[i]) + rng.randrange(int(lens[i]))] ^= 0x40
    want = np.zeros(n, np.int32)
    want[1::2] = -2
    d = lambda a: dev(torch, a)  # noqa: E731
    got = E.verify_messages(name, alg_id, d(altered), d(sigs), d(table), d(kidx.view(np.int32)), offsets=d(offs.astype(np.int64)),
                            lengths=d(lens.astype(np.int32)), le=le)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    good = E.verify_messages(name, alg_id, d(data), d(sigs), d(table), d(kidx.view(np.int32)), offsets=d(offs.astype(np.int64)),
                             lengths=d(lens.astype(np.int32)), le=le)
    torch.cuda.synchronize()
    assert not good.cpu().numpy().any()
    # host memory goes the same way
    assert np.array_equal(E.verify_messages(name, alg_id, altered, sigs, table, kidx, offsets=offs, lengths=lens,
                                            le=le), want)


@pytest.mark.parametrize("hs", [20, 32, 33])
def test_canaries_after_status_and_inputs(E, torch_, hs):
    """Nothing past status[count - 1] is written and no input byte changes;
    the hashes are packed at hash_size, so for 20 and 33 they are unaligned."""
    torch = torch_
    grp = next(g for g in FX["cases"] if g["curve"] == "secp256r1" and not g["le"])
    base = [k for k in grp["records"] if k["hash_size"] == 32]
    count = 67
    recs = [base[i % len(base)] for i in range(count)]
    if hs != 32:   # statuses for another hash size come from the model (pinned to the fixture on the CPU)
        c = CURVES["secp256r1"]
        want = np.array([M.verify(c, bytes.fromhex(k["hash"]), hs, bytes.fromhex(k["r"]), bytes.fromhex(k["s"]),
                                  bytes.fromhex(k["Qx"]), bytes.fromhex(k["Qy"]), False)
                         for k in base], np.int32)[np.arange(count) % len(base)]
        recs = [dict(k, hash=k["hash"] + "00" * 32) for k in recs]
        hashes, sigs, keys, _ = pack(recs, hs)
    else:
        hashes, sigs, keys, want = pack(recs, hs)
    tail = np.full(48, GUARD, np.uint8)
    bufs = [dev(torch, np.concatenate([a, tail])) for a in (hashes, sigs, keys)]
    before = [b.clone() for b in bufs]
    out = torch.full((count + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    got = E.verify_batch("secp256r1", bufs[0], bufs[1], bufs[2], hash_size=hs, count=count, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and np.array_equal(got.cpu().numpy(), want)
    assert (out[count:] == 0x5A5A5A5A).all().item()
    for b, a in zip(before, bufs):
        assert torch.equal(b, a)
    # host mode: the same through numpy, status guarded
    hout = np.full(count + 16, 0x5A5A5A5A, np.int32)
    E.verify_batch("secp256r1", hashes, sigs, keys, hash_size=hs, count=count, out=hout)
    assert np.array_equal(hout[:count], want) and (hout[count:] == 0x5A5A5A5A).all()


def test_async_on_the_current_stream(E, torch_):
    """Device mode enqueues on torch's current stream: inputs written by an
    earlier kernel of that stream are seen, and a side stream is honoured."""
    torch = torch_
    grp = next(g for g in FX["cases"] if g["curve"] == "secp256k1")
    recs = [k for k in grp["records"] if k["hash_size"] == 32]
    hashes, sigs, keys, want = pack(recs, 32)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dh = torch.zeros(hashes.size, dtype=torch.uint8, device="cuda:0")
        dh.copy_(dev(torch, hashes))                 # enqueued on s, ahead of the verify
        got = E.verify_batch("secp256k1", dh, dev(torch, sigs), dev(torch, keys))
    s.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)


def test_c_caller_verifies_one_case_per_curve(E, tmp_path):
    exe = str(tmp_path / "ecdsa_caller")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "ecdsa_caller.c"), "-o", exe,
                           "-L" + LIBDIR, "-llcb_ecdsa_gpu", "-Wl,-rpath," + LIBDIR,
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
