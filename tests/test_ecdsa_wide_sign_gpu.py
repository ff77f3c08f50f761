"""Batched ECDSA / GOST R 34.10-2012 signing, key generation and public keys on
the 384- and 512-bit curves on the MI355X (include/lcb_ecdsa_wide_sign_gpu.h)
against the reference-generated fixture tests/golden/ecdsa_wide_sign.json
(every status and byte there is what the reference returned and wrote) and,
for inputs the tests make themselves, the Python-int model
(tests/ecdsa_wide_model.py, tests/ecdsa_wide_sign_cases.py) and the wide
verification kernel.

One lane serves one item and one wave is one workgroup, so the shapes that
matter are counts around the 64-lane wave (1, 63, 64, 65, 129) with accepted
and rejected items sharing a wave, every hash size the import treats
differently on both sides of B, both byte orders, both limb counts, and the
key table with a bad index."""
import errno
import os
import random
import subprocess

import numpy as np
import pytest

from tests import ecdsa_wide_model as M
from tests import ecdsa_wide_sign_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "liblcb_amd")
FX = K.load_fixture()
CURVES = M.load_curves()
GROUP_IDS = ["%s-%s" % (g["curve"], "le" if g["le"] else "be") for g in FX["groups"]]
P384, BP512, GOST_A = "secp384r1", "brainpoolP512r1", "id-tc26-gost-3410-12-512-paramSetA"
# one curve per limb count (12, 16), in its natural form
PER_LIMBS = [(P384, False), (GOST_A, True)]
# one curve per limb count and algorithm kind, with the digest it pairs with
PAIRS = [(P384, "sha384", False), (BP512, "sha512", False), (GOST_A, "gost512", True)]
GUARD = 0xA5
EINVAL = errno.EINVAL


@pytest.fixture(scope="module")
def S(gpu):
    from liblcb_amd import ecdsa_wide_sign
    ecdsa_wide_sign.ecdsa_wide_sign_lib()
    return ecdsa_wide_sign


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


def cat(recs, *fields):
    return u8("".join("".join(k[f] for f in fields) for k in recs))


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def statuses(recs):
    return np.array([k["status"] for k in recs], np.int32)


def group(name, le):
    return next(g for g in FX["groups"] if g["curve"] == name and g["le"] == le)


def model_sign(c, h, hs, d, k, le):
    """(status, r || s) of one item by the Python-int model (d, k: ints)."""
    st, r, s = K.sign(c, h, hs, M.to_bytes(c, d, le), M.to_bytes(c, k, le), le)
    return st, r + s


def model_pub(c, d, le):
    st, x, y = K.pub_key(c, M.to_bytes(c, d, le), le)
    return st, x + y


def check_rows(what, recs, got, want):
    bad = [(k["name"], bytes(g).hex(), bytes(w).hex()) for k, g, w in zip(recs, got, want) if bytes(g) != bytes(w)]
    assert not bad, (what, bad[:4])


@pytest.mark.parametrize("grp", FX["groups"], ids=GROUP_IDS)
def test_every_fixture_record_in_both_memory_modes(S, torch_, grp):
    torch = torch_
    name, le = grp["curve"], grp["le"]
    B = CURVES[name]["bytes"]
    for mode in ("device", "host"):
        put = (lambda a: dev(torch, a)) if mode == "device" else (lambda a: a)
        seen = 0
        for hs in sorted({k["hash_size"] for k in grp["sign"]}):
            recs = [k for k in grp["sign"] if k["hash_size"] == hs]
            sigs, st = S.sign_batch(name, put(cat(recs, "hash")), put(cat(recs, "d")), put(cat(recs, "rnd")), le=le,
                                    hash_size=hs)
            torch.cuda.synchronize()
            assert sigs.shape == (len(recs), 2 * B) and st.shape == (len(recs),)
            assert (mode == "host") == isinstance(st, np.ndarray)
            assert host(st).tolist() == statuses(recs).tolist(), (mode, hs)
            check_rows((mode, "sign", hs), recs, host(sigs), cat(recs, "r", "s").reshape(-1, 2 * B))
            assert not host(sigs)[host(st) != 0].any()
            seen += len(recs)
        assert seen == len(grp["sign"])
        recs = grp["key_gen"]
        priv, pub, st = S.key_gen_batch(name, put(cat(recs, "rnd")), le=le)
        torch.cuda.synchronize()
        assert priv.shape == (len(recs), B) and pub.shape == (len(recs), 2 * B)
        assert host(st).tolist() == statuses(recs).tolist(), mode
        check_rows((mode, "key_gen d"), recs, host(priv), cat(recs, "d").reshape(-1, B))
        check_rows((mode, "key_gen Q"), recs, host(pub), cat(recs, "Qx", "Qy").reshape(-1, 2 * B))
        assert not host(priv)[host(st) != 0].any() and not host(pub)[host(st) != 0].any()
        recs = grp["pub_key"]
        pub, st = S.pub_key_batch(name, put(cat(recs, "d")), le=le)
        torch.cuda.synchronize()
        assert host(st).tolist() == statuses(recs).tolist(), mode
        check_rows((mode, "pub_key"), recs, host(pub), cat(recs, "Qx", "Qy").reshape(-1, 2 * B))
        assert not host(pub)[host(st) != 0].any()


@pytest.mark.parametrize("name,le", PER_LIMBS)
def test_mixed_batches_around_the_wave(S, torch_, name, le):
    """Accepted and rejected items interleaved, repeated cyclically: a lane
    that leaves early (-1, EINVAL) shares its wave with lanes that run all
    8 L windows; statuses and bytes compared position by position."""
    torch = torch_
    grp, B = group(name, le), CURVES[name]["bytes"]
    recs = [k for k in grp["sign"] if k["hash_size"] == B]
    assert {0, -1, EINVAL} <= {k["status"] for k in recs}
    h1, d1, k1 = (cat(recs, f).reshape(-1, B) for f in ("hash", "d", "rnd"))
    s1, w1 = cat(recs, "r", "s").reshape(-1, 2 * B), statuses(recs)
    kg, pk = grp["key_gen"], grp["pub_key"]
    assert {0, -1} <= set(statuses(kg).tolist()) and {0, -1, EINVAL} <= set(statuses(pk).tolist())
    for count in (1, 63, 64, 65, 129):
        # start each count at another record, so that lane 0 is not always "valid"
        idx = (np.arange(count) + count) % len(recs)
        sigs, st = S.sign_batch(name, dev(torch, h1[idx].reshape(-1)), dev(torch, d1[idx].reshape(-1)),
                                dev(torch, k1[idx].reshape(-1)), le=le)
        jdx = (np.arange(count) + count) % len(kg)
        priv, pub, kst = S.key_gen_batch(name, dev(torch, cat(kg, "rnd").reshape(-1, B)[jdx].reshape(-1)), le=le)
        pub2, pst = S.pub_key_batch(name, dev(torch, cat(pk, "d").reshape(-1, B)[jdx].reshape(-1)), le=le)
        torch.cuda.synchronize()
        assert st.shape == (count,) and st.dtype == torch.int32 and sigs.shape == (count, 2 * B)
        assert np.array_equal(host(st), w1[idx]), (count, np.nonzero(host(st) != w1[idx])[0][:8])
        assert np.array_equal(host(sigs), s1[idx]), count
        assert np.array_equal(host(kst), statuses(kg)[jdx]) and np.array_equal(host(pst), statuses(pk)[jdx]), count
        assert np.array_equal(host(priv), cat(kg, "d").reshape(-1, B)[jdx]), count
        assert np.array_equal(host(pub), cat(kg, "Qx", "Qy").reshape(-1, 2 * B)[jdx]), count
        assert np.array_equal(host(pub2), cat(pk, "Qx", "Qy").reshape(-1, 2 * B)[jdx]), count


@pytest.mark.parametrize("name,le", PER_LIMBS)
def test_key_table_and_bad_index(S, torch_, name, le):
    """Repeated and out-of-order indices, the first index past the table and
    the largest one.  The table is the whole buffer handed over, so a read
    of key 3 would be a read past the allocation."""
    torch = torch_
    c = CURVES[name]
    B = c["bytes"]
    rng = random.Random(37 + B)
    ds = [rng.randrange(1, c["n"]) for _ in range(3)]
    table = np.frombuffer(b"".join(M.to_bytes(c, d, le) for d in ds), np.uint8).copy()
    n = 70
    kidx = np.array([2, 2, 0, 1, 0] + [rng.randrange(3) for _ in range(n - 5)], np.uint32)
    kidx[17] = 3                           # the first index past the table
    kidx[40] = 0xFFFFFFFF
    hashes = [bytes(rng.randrange(256) for _ in range(B)) for _ in range(n)]
    rnds = [rng.randrange(1, 1 << (8 * B)) for _ in range(n)]
    want_st, want_sig = np.zeros(n, np.int32), np.zeros((n, 2 * B), np.uint8)
    for i in range(n):
        if kidx[i] >= 3:
            want_st[i] = EINVAL
            continue
        st, rs = model_sign(c, hashes[i], B, ds[kidx[i]], rnds[i], le)
        want_st[i], want_sig[i] = st, np.frombuffer(rs, np.uint8)
    assert want_st[17] == EINVAL and want_st[40] == EINVAL and (want_st == 0).sum() == n - 2
    hashes = np.frombuffer(b"".join(hashes), np.uint8).copy()
    rnd = np.frombuffer(b"".join(M.to_bytes(c, k, le) for k in rnds), np.uint8).copy()
    for as_int32 in (False, True):
        ki = kidx.view(np.int32) if as_int32 else kidx
        sigs, st = S.sign_batch(name, dev(torch, hashes), dev(torch, table), dev(torch, rnd), key_idx=dev(torch, ki),
                                le=le)
        torch.cuda.synchronize()
        assert np.array_equal(host(st), want_st) and np.array_equal(host(sigs), want_sig), ("device", as_int32)
        sigs, st = S.sign_batch(name, hashes, table, rnd, key_idx=ki, le=le)
        assert np.array_equal(st, want_st) and np.array_equal(sigs, want_sig), ("host", as_int32)


@pytest.mark.parametrize("name,alg,le", PAIRS)
def test_round_trip_with_the_verification_kernel(S, W, torch_, name, alg, le):
    """key_gen_batch -> sign_batch -> ecdsa_wide.verify_batch on the device,
    129 items: all 0; with one flipped hash byte per item all -2."""
    torch = torch_
    B = CURVES[name]["bytes"]
    n = 129
    rng = np.random.default_rng(129 + B)
    seed, nonce, hashes = (rng.integers(0, 256, B * n, dtype=np.uint8) for _ in range(3))
    priv, pub, kst = S.key_gen_batch(name, dev(torch, seed), le=le)
    dh = dev(torch, hashes)
    sigs, st = S.sign_batch(name, dh, priv.reshape(-1), dev(torch, nonce), le=le)
    ok = W.verify_batch(name, dh, sigs.reshape(-1), pub.reshape(-1), le=le)
    flipped = hashes.reshape(n, B).copy()
    flipped[np.arange(n), np.arange(n) % B] ^= 0x10          # one hash byte per item, every position
    bad = W.verify_batch(name, dev(torch, flipped.reshape(-1)), sigs.reshape(-1), pub.reshape(-1), le=le)
    pub2, pst = S.pub_key_batch(name, priv.reshape(-1), le=le)
    torch.cuda.synchronize()
    assert not host(kst).any() and not host(st).any() and not host(pst).any()
    assert not host(ok).any()
    assert np.array_equal(host(bad), np.full(n, -2, np.int32))
    assert torch.equal(pub2, pub) and host(pub).any(axis=1).all() and host(sigs).any(axis=1).all()


@pytest.mark.parametrize("name,alg,le", PAIRS)
def test_sign_messages(S, W, torch_, oracle, name, alg, le):
    """A handful of short messages: the signatures equal the model's over the
    oracle's digests and verify_messages accepts them."""
    import liblcb_amd
    torch = torch_
    c = CURVES[name]
    B = c["bytes"]
    alg_id = liblcb_amd.ALG_IDS[alg]
    assert liblcb_amd.DIGEST_SIZE[alg_id] == B
    rng = random.Random(65 + B)
    lens = np.array([0, 1, 47, 64, 129, 200, 127, 128], np.uint32)
    n = len(lens)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    data = np.frombuffer(bytes(rng.randrange(256) for _ in range(int(lens.sum()))), np.uint8).copy()
    digests = oracle.batch(alg_id, data, offs, lens)
    ds = [rng.randrange(1, c["n"]) for _ in range(3)]
    kidx = np.arange(n, dtype=np.uint32) % 3
    rnds = [rng.randrange(1, 1 << (8 * B)) for _ in range(n)]
    want = np.frombuffer(b"".join(model_sign(c, digests[i].tobytes(), B, ds[kidx[i]], rnds[i], le)[1]
                                  for i in range(n)), np.uint8).reshape(n, 2 * B)
    assert want.any(axis=1).all()
    table = np.frombuffer(b"".join(M.to_bytes(c, d, le) for d in ds), np.uint8).copy()
    rnd = np.frombuffer(b"".join(M.to_bytes(c, k, le) for k in rnds), np.uint8).copy()
    pubs = np.frombuffer(b"".join(model_pub(c, d, le)[1] for d in ds), np.uint8).copy()
    d = lambda a: dev(torch, a)  # noqa: E731
    layout = dict(offsets=d(offs.astype(np.int64)), lengths=d(lens.astype(np.int32)))
    sigs, st = S.sign_messages(name, alg_id, d(data), d(table), d(rnd), d(kidx.view(np.int32)), le=le, **layout)
    good = W.verify_messages(name, alg_id, d(data), sigs.reshape(-1), d(pubs), d(kidx.view(np.int32)), le=le,
                             **layout)
    torch.cuda.synchronize()
    assert not host(st).any() and np.array_equal(host(sigs), want)
    assert not host(good).any()
    # host memory goes the same way
    sigs, st = S.sign_messages(name, alg_id, data, table, rnd, kidx, offsets=offs, lengths=lens, le=le)
    assert not st.any() and np.array_equal(sigs, want)


@pytest.mark.parametrize("name,le", PER_LIMBS)
@pytest.mark.parametrize("hs", ["1", "B", "128"])
def test_canaries_after_outputs_and_inputs(S, torch_, name, le, hs):
    """Nothing past the last item of any output (sigs, status; priv, pub) is
    written and no input byte changes; the hashes are packed at hash_size."""
    torch = torch_
    c = CURVES[name]
    B = c["bytes"]
    hs = B if hs == "B" else int(hs)
    base = [k for k in group(name, le)["sign"] if k["hash_size"] == B]
    count = 67
    pad = lambda k: (bytes.fromhex(k["hash"]) + bytes(range(1, 129)))[:hs]  # noqa: E731
    model = [K.sign(c, pad(k), hs, bytes.fromhex(k["d"]), bytes.fromhex(k["rnd"]), le) for k in base]
    if hs == B:   # the model and the reference agree on the records both know
        assert [m[0] for m in model] == [k["status"] for k in base]
    recs = [base[i % len(base)] for i in range(count)]
    want_st = np.array([model[i % len(base)][0] for i in range(count)], np.int32)
    want_sig = np.frombuffer(b"".join(model[i % len(base)][1] + model[i % len(base)][2] for i in range(count)),
                             np.uint8).reshape(count, 2 * B)
    assert {0, -1, EINVAL} <= set(want_st.tolist())
    hashes = np.frombuffer(b"".join(pad(k) for k in recs), np.uint8).copy()
    priv, rnd = cat(recs, "d"), cat(recs, "rnd")
    tail = np.full(48, GUARD, np.uint8)
    bufs = [dev(torch, np.concatenate([a, tail])) for a in (hashes, priv, rnd)]
    before = [b.clone() for b in bufs]
    osig = torch.full((2 * B * (count + 16),), 0x5A, dtype=torch.uint8, device="cuda:0")
    ost = torch.full((count + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    sigs, st = S.sign_batch(name, bufs[0], bufs[1], bufs[2], le=le, hash_size=hs, count=count, out=(osig, ost))
    torch.cuda.synchronize()
    assert sigs.data_ptr() == osig.data_ptr() and st.data_ptr() == ost.data_ptr()
    assert np.array_equal(host(st), want_st) and np.array_equal(host(sigs), want_sig)
    assert (osig[2 * B * count:] == 0x5A).all().item() and (ost[count:] == 0x5A5A5A5A).all().item()
    for b, a in zip(before, bufs):
        assert torch.equal(b, a)
    # host mode: the same through numpy, outputs guarded
    hsig, hst = np.full(2 * B * (count + 16), 0x5A, np.uint8), np.full(count + 16, 0x5A5A5A5A, np.int32)
    hin = [np.concatenate([a, tail]) for a in (hashes, priv, rnd)]
    keep = [a.copy() for a in hin]
    S.sign_batch(name, hin[0], hin[1], hin[2], le=le, hash_size=hs, count=count, out=(hsig, hst))
    assert np.array_equal(hst[:count], want_st)
    assert np.array_equal(hsig[:2 * B * count].reshape(count, 2 * B), want_sig)
    assert (hsig[2 * B * count:] == 0x5A).all() and (hst[count:] == 0x5A5A5A5A).all()
    assert all(np.array_equal(a, b) for a, b in zip(hin, keep))
    if hs != B:
        return
    # the key calls: their outputs are views of exactly count items, each in an
    # allocation of its own; a batch of count + 1 must differ only by its last row
    src = dev(torch, np.concatenate([rnd, rnd[:B]]))
    keep = src.clone()
    p1, q1, s1 = S.key_gen_batch(name, src, le=le, count=count)
    p2, q2, s2 = S.key_gen_batch(name, src, le=le)
    q3, s3 = S.pub_key_batch(name, src, le=le, count=count)
    torch.cuda.synchronize()
    assert p1.shape == (count, B) and q1.shape == (count, 2 * B) and s1.shape == (count,) and s2.shape == (count + 1,)
    assert torch.equal(p1, p2[:count]) and torch.equal(q1, q2[:count]) and torch.equal(s1, s2[:count])
    assert q3.shape == (count, 2 * B) and s3.shape == (count,) and torch.equal(src, keep)


@pytest.mark.parametrize("name,le", PER_LIMBS)
def test_second_use_of_a_cached_table_gives_the_same_bytes(S, torch_, name, le):
    torch = torch_
    B = CURVES[name]["bytes"]
    recs = [k for k in group(name, le)["sign"] if k["hash_size"] == B]
    args = [dev(torch, cat(recs, f)) for f in ("hash", "d", "rnd")]
    outs = []
    for _ in range(2):
        sigs, st = S.sign_batch(name, *args, le=le)
        pub, pst = S.pub_key_batch(name, args[1], le=le)
        torch.cuda.synchronize()
        outs.append([host(t).copy() for t in (sigs, st, pub, pst)])
    assert all(np.array_equal(a, b) for a, b in zip(*outs))
    assert np.array_equal(outs[0][1], statuses(recs))
    assert np.array_equal(outs[0][0], cat(recs, "r", "s").reshape(-1, 2 * B))
    # another thread of the process finds the same table (host mode has its own staging per thread)
    import threading
    res = []
    t = threading.Thread(target=lambda: res.append(S.sign_batch(name, *(cat(recs, f) for f in ("hash", "d", "rnd")),
                                                                le=le)))
    t.start()
    t.join()
    assert np.array_equal(res[0][0], outs[0][0]) and np.array_equal(res[0][1], outs[0][1])


def test_async_on_the_current_stream(S, torch_):
    """Device mode enqueues on torch's current stream: inputs written by an
    earlier kernel of that stream are seen, and a side stream is honoured."""
    torch = torch_
    B = 48
    recs = [k for k in group(P384, False)["sign"] if k["hash_size"] == B]
    hashes, priv, rnd = cat(recs, "hash"), cat(recs, "d"), cat(recs, "rnd")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dh = torch.zeros(hashes.size, dtype=torch.uint8, device="cuda:0")
        dh.copy_(dev(torch, hashes))                 # enqueued on s, ahead of the signing
        sigs, st = S.sign_batch(P384, dh, dev(torch, priv), dev(torch, rnd))
    s.synchronize()
    assert np.array_equal(host(st), statuses(recs))
    assert np.array_equal(host(sigs), cat(recs, "r", "s").reshape(-1, 2 * B))


def test_c_caller_signs_one_case_per_group(S, tmp_path):
    from liblcb_amd import ecdsa_wide
    exe = str(tmp_path / "ecdsa_wide_sign_caller")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "ecdsa_wide_sign_caller.c"), "-o", exe,
                           "-L" + LIBDIR, "-llcb_ecdsa_wide_sign_gpu", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath-link," + LIBDIR + ":/opt/rocm/lib"])
    lines, want = [], []
    for i, grp in enumerate(FX["groups"]):
        c, le = CURVES[grp["curve"]], grp["le"]
        rejected = [k for k in grp["sign"] if k["status"] != 0]
        # a valid one per group, and a rejected one of a kind that changes with the group
        for k in (grp["sign"][0], rejected[i % len(rejected)]):
            lines.append("%d %d %d %s %s %s" % (ecdsa_wide.CURVES.index(grp["curve"]), le, k["hash_size"], k["hash"],
                                                k["d"], k["rnd"]))
            kst, qx, qy = K.pub_key(c, bytes.fromhex(k["d"]), le)
            want.append("%d %s %d %s" % (k["status"], k["r"] + k["s"], kst, (qx + qy).hex()))
    assert {g["curve"] for g in FX["groups"]} == set(CURVES)
    out = subprocess.run([exe, "sign"], input="\n".join(lines).encode(), stdout=subprocess.PIPE, check=True)
    assert out.stdout.decode().splitlines() == want
