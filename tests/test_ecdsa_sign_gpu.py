"""Batched ECDSA / GOST R 34.10 signing, key generation and public keys on the
MI355X (include/lcb_ecdsa_sign_gpu.h) against the reference-generated fixture
tests/golden/ecdsa_sign.json (every status and byte there is what the
reference returned and wrote) and, for inputs the tests make themselves, the
Python-int model tests/ecdsa_model.py and the existing verification kernel.

One lane serves one item, so the shapes that matter are counts around the
64-lane wave (1, 63, 64, 65, 257) with accepted and rejected items sharing a
wave, every hash size the import treats differently, both byte orders, and
the key table with a bad index."""
import errno
import json
import os
import random
import subprocess

import numpy as np
import pytest

from tests import ecdsa_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "liblcb_amd")
with open(os.path.join(ROOT, "tests", "golden", "ecdsa_sign.json")) as f:
    FX = json.load(f)
CURVES = M.load_curves()
GROUP_IDS = ["%s-%s" % (g["curve"], "le" if g["le"] else "be") for g in FX["groups"]]
GUARD = 0xA5
EINVAL = errno.EINVAL


@pytest.fixture(scope="module")
def S(gpu):
    from liblcb_amd import ecdsa_sign
    ecdsa_sign.ecdsa_sign_lib()
    return ecdsa_sign


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


def cat(recs, *fields):
    return u8("".join("".join(k[f] for f in fields) for k in recs))


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def statuses(recs):
    return np.array([k["status"] for k in recs], np.int32)


def model_sign(c, h, hs, d, k, le):
    """(status, r || s) of one item by the Python-int model (d, k: ints)."""
    if d >= c["n"]:
        return EINVAL, bytes(64)
    rs = M.sign(c, h, hs, d, k, le)
    return (-1, bytes(64)) if rs is None else (0, M.to_bytes(rs[0], le) + M.to_bytes(rs[1], le))


def model_pub(c, d, le):
    if d >= c["n"]:
        return EINVAL, bytes(64)
    if d == 0:
        return -1, bytes(64)
    Q = M.public_key(c, d)
    return 0, M.to_bytes(Q[0], le) + M.to_bytes(Q[1], le)


def check_rows(what, recs, got, want):
    bad = [(k["name"], bytes(g).hex(), bytes(w).hex()) for k, g, w in zip(recs, got, want) if bytes(g) != bytes(w)]
    assert not bad, (what, bad[:4])


@pytest.mark.parametrize("grp", FX["groups"], ids=GROUP_IDS)
def test_every_fixture_record_in_both_memory_modes(S, torch_, grp):
    torch = torch_
    name, le = grp["curve"], grp["le"]
    for mode in ("device", "host"):
        put = (lambda a: dev(torch, a)) if mode == "device" else (lambda a: a)
        seen = 0
        for hs in sorted({k["hash_size"] for k in grp["sign"]}):
            recs = [k for k in grp["sign"] if k["hash_size"] == hs]
            sigs, st = S.sign_batch(name, put(cat(recs, "hash")), put(cat(recs, "d")), put(cat(recs, "rnd")), le=le,
                                    hash_size=hs)
            torch.cuda.synchronize()
            assert sigs.shape == (len(recs), 64) and st.shape == (len(recs),)
            assert (mode == "host") == isinstance(st, np.ndarray)
            assert host(st).tolist() == statuses(recs).tolist(), (mode, hs)
            check_rows((mode, "sign", hs), recs, host(sigs), cat(recs, "r", "s").reshape(-1, 64))
            rejected = host(st) != 0
            assert not host(sigs)[rejected].any()
            seen += len(recs)
        assert seen == len(grp["sign"])
        recs = grp["key_gen"]
        priv, pub, st = S.key_gen_batch(name, put(cat(recs, "rnd")), le=le)
        torch.cuda.synchronize()
        assert host(st).tolist() == statuses(recs).tolist(), mode
        check_rows((mode, "key_gen d"), recs, host(priv), cat(recs, "d").reshape(-1, 32))
        check_rows((mode, "key_gen Q"), recs, host(pub), cat(recs, "Qx", "Qy").reshape(-1, 64))
        assert not host(priv)[host(st) != 0].any() and not host(pub)[host(st) != 0].any()
        recs = grp["pub_key"]
        pub, st = S.pub_key_batch(name, put(cat(recs, "d")), le=le)
        torch.cuda.synchronize()
        assert host(st).tolist() == statuses(recs).tolist(), mode
        check_rows((mode, "pub_key"), recs, host(pub), cat(recs, "Qx", "Qy").reshape(-1, 64))
        assert not host(pub)[host(st) != 0].any()


@pytest.mark.parametrize("grp", FX["groups"], ids=GROUP_IDS)
def test_mixed_batches_around_the_wave(S, torch_, grp):
    """Accepted and rejected items interleaved, repeated cyclically: a lane
    that leaves early (-1, EINVAL) shares its wave with lanes that run all 64
    windows; statuses and bytes compared position by position."""
    torch = torch_
    name, le = grp["curve"], grp["le"]
    recs = [k for k in grp["sign"] if k["hash_size"] == 32]
    assert {0, -1, EINVAL} <= {k["status"] for k in recs}
    h1, d1, k1 = (cat(recs, f).reshape(-1, 32) for f in ("hash", "d", "rnd"))
    s1, w1 = cat(recs, "r", "s").reshape(-1, 64), statuses(recs)
    kg, pk = grp["key_gen"], grp["pub_key"]
    for count in (1, 63, 64, 65, 257):
        # start each count at another record, so that lane 0 is not always "valid"
        idx = (np.arange(count) + count) % len(recs)
        sigs, st = S.sign_batch(name, dev(torch, h1[idx].reshape(-1)), dev(torch, d1[idx].reshape(-1)),
                                dev(torch, k1[idx].reshape(-1)), le=le)
        jdx = (np.arange(count) + count) % len(kg)
        priv, pub, kst = S.key_gen_batch(name, dev(torch, cat(kg, "rnd").reshape(-1, 32)[jdx].reshape(-1)), le=le)
        pub2, pst = S.pub_key_batch(name, dev(torch, cat(pk, "d").reshape(-1, 32)[jdx].reshape(-1)), le=le)
        torch.cuda.synchronize()
        assert st.shape == (count,) and st.dtype == torch.int32 and sigs.shape == (count, 64)
        assert np.array_equal(host(st), w1[idx]), (count, np.nonzero(host(st) != w1[idx])[0][:8])
        assert np.array_equal(host(sigs), s1[idx]), count
        assert np.array_equal(host(kst), statuses(kg)[jdx]) and np.array_equal(host(pst), statuses(pk)[jdx]), count
        assert np.array_equal(host(priv), cat(kg, "d").reshape(-1, 32)[jdx]), count
        assert np.array_equal(host(pub), cat(kg, "Qx", "Qy").reshape(-1, 64)[jdx]), count
        assert np.array_equal(host(pub2), cat(pk, "Qx", "Qy").reshape(-1, 64)[jdx]), count


@pytest.mark.parametrize("name,le", [("secp256k1", False), ("id-gostR3410-2001-CryptoPro-B-ParamSet", True)])
def test_key_table_and_bad_index(S, torch_, name, le):
    torch = torch_
    c = CURVES[name]
    rng = random.Random(37)
    ds = [rng.randrange(1, c["n"]) for _ in range(3)]
    table = np.frombuffer(b"".join(M.to_bytes(d, le) for d in ds), np.uint8).copy()
    n = 70
    kidx = np.array([rng.randrange(3) for _ in range(n)], np.uint32)
    kidx[17] = 3                           # the first index past the table
    kidx[40] = 0xFFFFFFFF
    hashes = [bytes(rng.randrange(256) for _ in range(32)) for _ in range(n)]
    rnds = [rng.randrange(1, 1 << 256) for _ in range(n)]
    want_st, want_sig = np.zeros(n, np.int32), np.zeros((n, 64), np.uint8)
    for i in range(n):
        if kidx[i] >= 3:
            want_st[i] = EINVAL
            continue
        st, rs = model_sign(c, hashes[i], 32, ds[kidx[i]], rnds[i], le)
        want_st[i], want_sig[i] = st, np.frombuffer(rs, np.uint8)
    assert want_st[17] == EINVAL and want_st[40] == EINVAL and (want_st == 0).sum() == n - 2
    hashes = np.frombuffer(b"".join(hashes), np.uint8).copy()
    rnd = np.frombuffer(b"".join(M.to_bytes(k, le) for k in rnds), np.uint8).copy()
    for as_int32 in (False, True):
        ki = kidx.view(np.int32) if as_int32 else kidx
        sigs, st = S.sign_batch(name, dev(torch, hashes), dev(torch, table), dev(torch, rnd), key_idx=dev(torch, ki),
                                le=le)
        torch.cuda.synchronize()
        assert np.array_equal(host(st), want_st) and np.array_equal(host(sigs), want_sig), ("device", as_int32)
        sigs, st = S.sign_batch(name, hashes, table, rnd, key_idx=ki, le=le)
        assert np.array_equal(st, want_st) and np.array_equal(sigs, want_sig), ("host", as_int32)


@pytest.mark.parametrize("name,le", [("secp256k1", False), ("id-gostR3410-2001-CryptoPro-B-ParamSet", True)])
def test_round_trip_with_the_verification_kernel(S, E, torch_, name, le):
    """key_gen_batch -> sign_batch -> verify_batch on the device, 257 items."""
    torch = torch_
    n = 257
    rng = np.random.default_rng(257)
    seed, nonce, hashes = (rng.integers(0, 256, 32 * n, dtype=np.uint8) for _ in range(3))
    priv, pub, kst = S.key_gen_batch(name, dev(torch, seed), le=le)
    dh = dev(torch, hashes)
    sigs, st = S.sign_batch(name, dh, priv.reshape(-1), dev(torch, nonce), le=le)
    ok = E.verify_batch(name, dh, sigs.reshape(-1), pub.reshape(-1), le=le)
    flipped = hashes.reshape(n, 32).copy()
    flipped[1::2, 7] ^= 0x10                       # one hash bit per odd item
    bad = E.verify_batch(name, dev(torch, flipped.reshape(-1)), sigs.reshape(-1), pub.reshape(-1), le=le)
    pub2, pst = S.pub_key_batch(name, priv.reshape(-1), le=le)
    torch.cuda.synchronize()
    assert not host(kst).any() and not host(st).any() and not host(pst).any()
    assert not host(ok).any()
    want = np.zeros(n, np.int32)
    want[1::2] = -2
    assert np.array_equal(host(bad), want)
    assert torch.equal(pub2, pub) and host(pub).any(axis=1).all()


@pytest.mark.parametrize("name,alg,le", [("secp256r1", "sha256", False),
                                         ("id-gostR3410-2001-CryptoPro-A-ParamSet", "gost256", True)])
def test_sign_messages(S, E, torch_, oracle, name, alg, le):
    """64 ragged messages of 0..300 bytes: the signatures equal the model's
    over the oracle's digests and verify_messages accepts them."""
    import liblcb_amd
    torch = torch_
    c = CURVES[name]
    alg_id = liblcb_amd.ALG_IDS[alg]
    rng = random.Random(65)
    n = 64
    lens = np.array([0, 300, 1, 299] + [rng.randrange(301) for _ in range(n - 4)], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    data = np.frombuffer(bytes(rng.randrange(256) for _ in range(int(lens.sum()))), np.uint8).copy()
    digests = oracle.batch(alg_id, data, offs, lens)
    ds = [rng.randrange(1, c["n"]) for _ in range(4)]
    kidx = np.arange(n, dtype=np.uint32) % 4
    rnds = [rng.randrange(1, 1 << 256) for _ in range(n)]
    want = np.frombuffer(b"".join(model_sign(c, digests[i].tobytes(), 32, ds[kidx[i]], rnds[i], le)[1]
                                  for i in range(n)), np.uint8).reshape(n, 64)
    assert want.any(axis=1).all()
    table = np.frombuffer(b"".join(M.to_bytes(d, le) for d in ds), np.uint8).copy()
    rnd = np.frombuffer(b"".join(M.to_bytes(k, le) for k in rnds), np.uint8).copy()
    pubs = np.frombuffer(b"".join(model_pub(c, d, le)[1] for d in ds), np.uint8).copy()
    d = lambda a: dev(torch, a)  # noqa: E731
    layout = dict(offsets=d(offs.astype(np.int64)), lengths=d(lens.astype(np.int32)))
    sigs, st = S.sign_messages(name, alg_id, d(data), d(table), d(rnd), d(kidx.view(np.int32)), le=le, **layout)
    good = E.verify_messages(name, alg_id, d(data), sigs.reshape(-1), d(pubs), d(kidx.view(np.int32)), le=le,
                             **layout)
    torch.cuda.synchronize()
    assert not host(st).any() and np.array_equal(host(sigs), want)
    assert not host(good).any()
    # host memory goes the same way
    sigs, st = S.sign_messages(name, alg_id, data, table, rnd, kidx, offsets=offs, lengths=lens, le=le)
    assert not st.any() and np.array_equal(sigs, want)


@pytest.mark.parametrize("hs", [20, 32, 33])
def test_canaries_after_outputs_and_inputs(S, torch_, hs):
    """Nothing past sigs[count - 1] and status[count - 1] is written and no
    input byte changes; the hashes are packed at hash_size, so for 20 and 33
    they are unaligned."""
    torch = torch_
    name, le = "secp256r1", False
    c = CURVES[name]
    grp = next(g for g in FX["groups"] if g["curve"] == name and not g["le"])
    base = [k for k in grp["sign"] if k["hash_size"] == 32]
    count = 67
    model = [model_sign(c, (bytes.fromhex(k["hash"]) + bytes(32))[:hs], hs, int(k["d"], 16), int(k["rnd"], 16), le)
             for k in base]
    if hs == 32:   # the model and the reference agree on the records both know
        assert [m[0] for m in model] == [k["status"] for k in base]
    recs = [base[i % len(base)] for i in range(count)]
    want_st = np.array([model[i % len(base)][0] for i in range(count)], np.int32)
    want_sig = np.frombuffer(b"".join(model[i % len(base)][1] for i in range(count)), np.uint8).reshape(count, 64)
    assert {0, -1, EINVAL} <= set(want_st.tolist())
    hashes = u8("".join((k["hash"] + "00" * 32)[:2 * hs] for k in recs))
    priv, rnd = cat(recs, "d"), cat(recs, "rnd")
    tail = np.full(48, GUARD, np.uint8)
    bufs = [dev(torch, np.concatenate([a, tail])) for a in (hashes, priv, rnd)]
    before = [b.clone() for b in bufs]
    osig = torch.full((64 * (count + 16),), 0x5A, dtype=torch.uint8, device="cuda:0")
    ost = torch.full((count + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    sigs, st = S.sign_batch(name, bufs[0], bufs[1], bufs[2], hash_size=hs, count=count, out=(osig, ost))
    torch.cuda.synchronize()
    assert sigs.data_ptr() == osig.data_ptr() and st.data_ptr() == ost.data_ptr()
    assert np.array_equal(host(st), want_st) and np.array_equal(host(sigs), want_sig)
    assert (osig[64 * count:] == 0x5A).all().item() and (ost[count:] == 0x5A5A5A5A).all().item()
    for b, a in zip(before, bufs):
        assert torch.equal(b, a)
    # host mode: the same through numpy, outputs guarded
    hsig, hst = np.full(64 * (count + 16), 0x5A, np.uint8), np.full(count + 16, 0x5A5A5A5A, np.int32)
    hin = [np.concatenate([a, tail]) for a in (hashes, priv, rnd)]
    keep = [a.copy() for a in hin]
    S.sign_batch(name, hin[0], hin[1], hin[2], hash_size=hs, count=count, out=(hsig, hst))
    assert np.array_equal(hst[:count], want_st) and np.array_equal(hsig[:64 * count].reshape(count, 64), want_sig)
    assert (hsig[64 * count:] == 0x5A).all() and (hst[count:] == 0x5A5A5A5A).all()
    assert all(np.array_equal(a, b) for a, b in zip(hin, keep))


def test_async_on_the_current_stream(S, torch_):
    """Device mode enqueues on torch's current stream: inputs written by an
    earlier kernel of that stream are seen, and a side stream is honoured."""
    torch = torch_
    grp = next(g for g in FX["groups"] if g["curve"] == "secp256k1")
    recs = [k for k in grp["sign"] if k["hash_size"] == 32]
    hashes, priv, rnd = cat(recs, "hash"), cat(recs, "d"), cat(recs, "rnd")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dh = torch.zeros(hashes.size, dtype=torch.uint8, device="cuda:0")
        dh.copy_(dev(torch, hashes))                 # enqueued on s, ahead of the signing
        sigs, st = S.sign_batch("secp256k1", dh, dev(torch, priv), dev(torch, rnd))
    s.synchronize()
    assert np.array_equal(host(st), statuses(recs))
    assert np.array_equal(host(sigs), cat(recs, "r", "s").reshape(-1, 64))


def test_c_caller_signs_one_case_per_curve(S, tmp_path):
    from liblcb_amd import ecdsa
    exe = str(tmp_path / "ecdsa_sign_caller")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "ecdsa_sign_caller.c"), "-o", exe,
                           "-L" + LIBDIR, "-llcb_ecdsa_sign_gpu", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath-link," + LIBDIR + ":/opt/rocm/lib"])
    lines, want = [], []
    for i, grp in enumerate(FX["groups"]):
        c, le = CURVES[grp["curve"]], grp["le"]
        rejected = [k for k in grp["sign"] if k["status"] != 0]
        # a valid one per group, and a rejected one of a kind that changes with the group
        for k in (grp["sign"][0], rejected[i % len(rejected)]):
            lines.append("%d %d %d %s %s %s" % (ecdsa.CURVES.index(grp["curve"]), le, k["hash_size"], k["hash"],
                                                k["d"], k["rnd"]))
            kst, q = model_pub(c, M.num(bytes.fromhex(k["d"]), le), le)
            want.append("%d %s %d %s" % (k["status"], k["r"] + k["s"], kst, q.hex()))
    assert {g["curve"] for g in FX["groups"]} == set(CURVES)
    out = subprocess.run([exe, "sign"], input="\n".join(lines).encode(), stdout=subprocess.PIPE, check=True)
    assert out.stdout.decode().splitlines() == want
