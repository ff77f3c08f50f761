"""Batched ECDH key agreement on the MI355X (include/lcb_ecdsa_dh_gpu.h)
against the reference-generated fixture tests/golden/ecdsa_dh.json (every
status and byte there is what the reference returned and wrote) and, for
inputs the tests make themselves, the Python-int model tests/ecdsa_model.py
(the plain d Q) and the signing library's pub_key_batch.

One lane serves one item, so the shapes that matter are counts around the
64-lane wave (1, 63, 64, 65, 130) with accepted and every kind of rejected
item sharing a wave, both byte orders, and the two key tables with a bad
index in each."""
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
with open(os.path.join(ROOT, "tests", "golden", "ecdsa_dh.json")) as f:
    FX = json.load(f)
CURVES = M.load_curves()
GROUP_IDS = ["%s-%s" % (g["curve"], "le" if g["le"] else "be") for g in FX["groups"]]
EINVAL = errno.EINVAL
PAIRS = [("secp256k1", False), ("id-gostR3410-2001-CryptoPro-B-ParamSet", True)]


@pytest.fixture(scope="module")
def D(gpu):
    from liblcb_amd import ecdsa_dh
    ecdsa_dh.ecdsa_dh_lib()
    return ecdsa_dh


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
    return next(g for g in FX["groups"] if g["curve"] == name and bool(g["le"]) == le)


def arrays(grp):
    """(pub (n, 64), priv (n, 32), shared (n, 32), status (n,)) of a group's records."""
    recs = grp["records"]
    return (cat(recs, "Qx", "Qy").reshape(-1, 64), cat(recs, "d").reshape(-1, 32),
            cat(recs, "shared").reshape(-1, 32), statuses(recs))


def model_dh(c, qx, qy, d, le):
    """(status, shared) of one item by the Python-int model (ints in)."""
    if qx >= c["p"] or qy >= c["p"] or not M.on_curve(c, qx, qy):
        return -1, bytes(32)
    if d >= c["n"]:
        return EINVAL, bytes(32)
    R = M.mult(c, d, (qx, qy)) if d else None
    return (-1, bytes(32)) if R is None else (0, M.to_bytes(R[0], le))


def check_rows(what, recs, got, want):
    bad = [(k["name"], bytes(g).hex(), bytes(w).hex()) for k, g, w in zip(recs, got, want) if bytes(g) != bytes(w)]
    assert not bad, (what, bad[:4])


@pytest.mark.parametrize("grp", FX["groups"], ids=GROUP_IDS)
def test_every_fixture_record_in_both_memory_modes(D, torch_, grp):
    torch = torch_
    name, le = grp["curve"], grp["le"]
    for mode in ("device", "host"):
        put = (lambda a: dev(torch, a)) if mode == "device" else (lambda a: a)
        seen = 0
        for cof in (0, 1):  # use_cofactor is one flag per call
            recs = [k for k in grp["records"] if k["use_cofactor"] == cof]
            shared, st = D.dh_batch(name, put(cat(recs, "Qx", "Qy")), put(cat(recs, "d")), le=le,
                                    use_cofactor=bool(cof))
            torch.cuda.synchronize()
            assert shared.shape == (len(recs), 32) and st.shape == (len(recs),)
            assert (mode == "host") == isinstance(st, np.ndarray)
            assert host(st).tolist() == statuses(recs).tolist(), (mode, cof)
            check_rows((mode, cof), recs, host(shared), cat(recs, "shared").reshape(-1, 32))
            assert not host(shared)[host(st) != 0].any()
            seen += len(recs)
        assert seen == len(grp["records"])


@pytest.mark.parametrize("grp", FX["groups"], ids=GROUP_IDS)
def test_mixed_batches_around_the_wave(D, torch_, grp):
    """A group's records repeated cyclically: lanes that leave early (-1 for
    the key, EINVAL, -1 for d = 0) share their wave with lanes that run all
    256 steps, the tail lanes of the last wave are masked; statuses and bytes
    compared position by position."""
    torch = torch_
    name, le = grp["curve"], grp["le"]
    pub, priv, want, wst = arrays(grp)
    assert {0, -1, EINVAL} <= set(wst.tolist())
    for count in (1, 63, 64, 65, 130):
        # start each count at another record, so that lane 0 is not always the same
        idx = (np.arange(count) + count) % len(wst)
        shared, st = D.dh_batch(name, dev(torch, pub[idx].reshape(-1)), dev(torch, priv[idx].reshape(-1)), le=le)
        torch.cuda.synchronize()
        assert st.shape == (count,) and st.dtype == torch.int32 and shared.shape == (count, 32)
        assert np.array_equal(host(st), wst[idx]), (count, np.nonzero(host(st) != wst[idx])[0][:8])
        assert np.array_equal(host(shared), want[idx]), count
        if count >= 63:
            assert {0, -1, EINVAL} <= set(wst[idx].tolist())


@pytest.mark.parametrize("name,le", PAIRS)
def test_one_private_key_many_peers(D, torch_, name, le):
    """npriv = 1, priv_idx of zeros, 130 peers: the fixture's keys, refused
    ones among them, cycled."""
    torch = torch_
    c = CURVES[name]
    grp = group(name, le)
    pub = arrays(grp)[0]
    uniq = sorted({bytes(r) for r in pub})
    d = random.Random(130).randrange(1, c["n"])
    by_key = {q: model_dh(c, M.num(q[:32], le), M.num(q[32:], le), d, le) for q in uniq}
    n = 130
    peers = [bytes(pub[(7 * i) % len(pub)]) for i in range(n)]
    want_st = np.array([by_key[q][0] for q in peers], np.int32)
    want = np.frombuffer(b"".join(by_key[q][1] for q in peers), np.uint8).reshape(n, 32)
    assert {0, -1} <= set(want_st.tolist())
    keys, one = np.frombuffer(b"".join(peers), np.uint8).copy(), np.frombuffer(M.to_bytes(d, le), np.uint8).copy()
    zeros = np.zeros(n, np.uint32)
    shared, st = D.dh_batch(name, dev(torch, keys), dev(torch, one), le=le, priv_idx=dev(torch, zeros.view(np.int32)))
    torch.cuda.synchronize()
    assert np.array_equal(host(st), want_st) and np.array_equal(host(shared), want)
    shared, st = D.dh_batch(name, keys, one, le=le, priv_idx=zeros)
    assert np.array_equal(st, want_st) and np.array_equal(shared, want)


@pytest.mark.parametrize("name,le", PAIRS)
def test_both_key_tables_and_bad_indices(D, torch_, name, le):
    """npub = 3, npriv = 5 with both index arrays; one index past each table
    gives EINVAL and zeros and leaves its neighbours as they are."""
    torch = torch_
    c = CURVES[name]
    rng = random.Random(35)
    ds = [rng.randrange(1, c["n"]) for _ in range(5)]
    qs = [M.mult(c, rng.randrange(1, c["n"]), M.base(c)) for _ in range(3)]
    cell = {(i, j): model_dh(c, qs[i][0], qs[i][1], ds[j], le) for i in range(3) for j in range(5)}
    n = 70
    pidx = np.array([rng.randrange(3) for _ in range(n)], np.uint32)
    didx = np.array([rng.randrange(5) for _ in range(n)], np.uint32)
    clean_st = np.array([cell[(int(i), int(j))][0] for i, j in zip(pidx, didx)], np.int32)
    clean = np.frombuffer(b"".join(cell[(int(i), int(j))][1] for i, j in zip(pidx, didx)), np.uint8).reshape(n, 32)
    assert not clean_st.any() and clean.any(axis=1).all()
    pidx[17] = 3                           # the first index past the public table
    didx[40] = 5                           # the first index past the private table
    pidx[64], didx[64] = 0xFFFFFFFF, 0xFFFFFFFF
    want_st, want = clean_st.copy(), clean.copy()
    for i in (17, 40, 64):
        want_st[i], want[i] = EINVAL, 0
    pubs = np.frombuffer(b"".join(M.to_bytes(x, le) + M.to_bytes(y, le) for x, y in qs), np.uint8).copy()
    privs = np.frombuffer(b"".join(M.to_bytes(d, le) for d in ds), np.uint8).copy()
    for as_int32 in (False, True):
        pi, di = (pidx.view(np.int32), didx.view(np.int32)) if as_int32 else (pidx, didx)
        shared, st = D.dh_batch(name, dev(torch, pubs), dev(torch, privs), le=le, pub_idx=dev(torch, pi),
                                priv_idx=dev(torch, di))
        torch.cuda.synchronize()
        assert np.array_equal(host(st), want_st) and np.array_equal(host(shared), want), ("device", as_int32)
        shared, st = D.dh_batch(name, pubs, privs, le=le, pub_idx=pi, priv_idx=di)
        assert np.array_equal(st, want_st) and np.array_equal(shared, want), ("host", as_int32)


@pytest.mark.parametrize("name,le", PAIRS)
def test_agreement_of_130_random_pairs(D, torch_, name, le):
    """Public keys from the signing library's pub_key_batch on the device;
    dh(dA, QB) == dh(dB, QA) byte for byte, both the model's dA QB, and
    use_cofactor changes nothing."""
    from liblcb_amd import ecdsa_sign
    torch = torch_
    c = CURVES[name]
    rng = random.Random(0xD4)
    n = 130
    da = [rng.randrange(1, c["n"]) for _ in range(n)]
    db = [rng.randrange(1, c["n"]) for _ in range(n)]
    pa = dev(torch, np.frombuffer(b"".join(M.to_bytes(d, le) for d in da), np.uint8).copy())
    pb = dev(torch, np.frombuffer(b"".join(M.to_bytes(d, le) for d in db), np.uint8).copy())
    qa, sta = ecdsa_sign.pub_key_batch(name, pa, le=le)
    qb, stb = ecdsa_sign.pub_key_batch(name, pb, le=le)
    sab, st1 = D.dh_batch(name, qb.reshape(-1), pa, le=le)
    sba, st2 = D.dh_batch(name, qa.reshape(-1), pb, le=le, use_cofactor=True)
    sab1, st3 = D.dh_batch(name, qb.reshape(-1), pa, le=le, use_cofactor=True)
    torch.cuda.synchronize()
    assert not host(sta).any() and not host(stb).any()
    assert not host(st1).any() and not host(st2).any() and not host(st3).any()
    assert torch.equal(sab, sba) and torch.equal(sab, sab1)
    G = M.base(c)
    want = b"".join(M.to_bytes(M.mult(c, a * b % c["n"], G)[0], le) for a, b in zip(da, db))
    assert bytes(host(sab).reshape(-1)) == want
    # the model's dA QB from the device's own QB, for the first items
    for i in range(4):
        q = bytes(host(qb)[i])
        assert model_dh(c, M.num(q[:32], le), M.num(q[32:], le), da[i], le) == (0, want[32 * i:32 * i + 32])


@pytest.mark.parametrize("name,alg,le", [("secp256r1", "sha256", False),
                                         ("id-gostR3410-2001-CryptoPro-A-ParamSet", "gost256", True)])
def test_dh_digest(D, torch_, oracle, name, alg, le):
    """The digests of the fixture's secrets by the oracle; a rejected item
    hashes its 32 zero bytes and carries its status beside the digest."""
    import liblcb_amd
    torch = torch_
    alg_id = liblcb_amd.ALG_IDS[alg]
    grp = group(name, le)
    pub, priv, want, wst = arrays(grp)
    n = len(wst)
    exp = oracle.batch(alg_id, want.reshape(-1), np.arange(n, dtype=np.uint64) * 32, np.full(n, 32, np.uint32))
    zero_digest = oracle.batch(alg_id, np.zeros(32, np.uint8), np.zeros(1, np.uint64), np.full(1, 32, np.uint32))[0]
    dig, st = D.dh_digest(alg_id, name, dev(torch, pub.reshape(-1)), dev(torch, priv.reshape(-1)), le=le)
    torch.cuda.synchronize()
    assert dig.shape == exp.shape and np.array_equal(host(st), wst) and np.array_equal(host(dig), exp)
    assert (wst != 0).any() and all(np.array_equal(host(dig)[i], zero_digest) for i in np.nonzero(wst)[0])
    dig, st = D.dh_digest(alg_id, name, pub.reshape(-1), priv.reshape(-1), le=le)      # host memory goes the same way
    assert isinstance(dig, np.ndarray) and np.array_equal(st, wst) and np.array_equal(dig, exp)


@pytest.mark.parametrize("shift", [0, 1, 3])
def test_canaries_inputs_and_odd_alignment(D, torch_, shift):
    """Nothing past shared[count - 1] and status[count - 1] is written, no
    input byte changes, and key and output pointers at odd addresses do."""
    torch = torch_
    name, le = "secp256r1", False
    pub, priv, want, wst = arrays(group(name, le))
    count = 67
    idx = np.arange(count) % len(wst)
    guard = np.full(48, 0xA5, np.uint8)
    pre = np.full(shift, 0xA5, np.uint8)
    hin = [np.concatenate([pre, a, guard]) for a in (pub[idx].reshape(-1), priv[idx].reshape(-1))]
    bufs = [dev(torch, a) for a in hin]
    before = [b.clone() for b in bufs]
    obuf = torch.full((shift + 32 * (count + 16),), 0x5A, dtype=torch.uint8, device="cuda:0")
    ost = torch.full((count + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    osh = obuf[shift:]
    assert osh.data_ptr() % 4 == shift % 4 and bufs[0][shift:].data_ptr() % 4 == shift % 4
    shared, st = D.dh_batch(name, bufs[0][shift:], bufs[1][shift:], le=le, count=count, out=(osh, ost))
    torch.cuda.synchronize()
    assert shared.data_ptr() == osh.data_ptr() and st.data_ptr() == ost.data_ptr()
    assert np.array_equal(host(st), wst[idx]) and np.array_equal(host(shared), want[idx])
    assert (obuf[:shift] == 0x5A).all().item() and (osh[32 * count:] == 0x5A).all().item()
    assert (ost[count:] == 0x5A5A5A5A).all().item()
    for b, a in zip(before, bufs):
        assert torch.equal(b, a)
    # host mode: the same through numpy, outputs guarded
    hbuf, hst = np.full(shift + 32 * (count + 16), 0x5A, np.uint8), np.full(count + 16, 0x5A5A5A5A, np.int32)
    keep = [a.copy() for a in hin]
    D.dh_batch(name, hin[0][shift:], hin[1][shift:], le=le, count=count, out=(hbuf[shift:], hst))
    assert np.array_equal(hst[:count], wst[idx])
    assert np.array_equal(hbuf[shift:shift + 32 * count].reshape(count, 32), want[idx])
    assert (hbuf[:shift] == 0x5A).all() and (hbuf[shift + 32 * count:] == 0x5A).all() and (hst[count:] == 0x5A5A5A5A).all()
    assert all(np.array_equal(a, b) for a, b in zip(hin, keep))


def test_async_on_a_side_stream(D, torch_):
    """Device mode enqueues on torch's current stream and returns: inputs
    written by an earlier copy of that stream are seen, the call comes back
    while its 2^16 items (milliseconds of device time) are still running, and
    the answers are there after synchronize."""
    torch = torch_
    name, le = "secp256k1", False
    pub, priv, want, wst = arrays(group(name, le))
    count = 1 << 16
    idx = np.arange(count) % len(wst)
    hp, hd = pub[idx].reshape(-1), priv[idx].reshape(-1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dp = torch.zeros(hp.size, dtype=torch.uint8, device="cuda:0")
        dd = torch.zeros(hd.size, dtype=torch.uint8, device="cuda:0")
        dp.copy_(dev(torch, hp))                     # enqueued on s, ahead of the agreement
        dd.copy_(dev(torch, hd))
        shared, st = D.dh_batch(name, dp, dd, le=le)
        done = torch.cuda.Event()
        done.record(s)
        returned_early = not done.query()
    s.synchronize()
    assert returned_early
    assert np.array_equal(host(st), wst[idx]) and np.array_equal(host(shared), want[idx])


def test_c_caller_agrees_one_case_per_curve(D, tmp_path):
    from liblcb_amd import ecdsa
    exe = str(tmp_path / "ecdsa_dh_caller")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "ecdsa_dh_caller.c"), "-o", exe,
                           "-L" + LIBDIR, "-llcb_ecdsa_dh_gpu", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath-link," + LIBDIR + ":/opt/rocm/lib"])
    lines, want = [], []
    for i, grp in enumerate(FX["groups"]):
        rejected = [k for k in grp["records"] if k["status"] != 0]
        accepted = [k for k in grp["records"] if k["status"] == 0]
        # an accepted one per group, and a rejected one of a kind that changes with the group
        for k in (accepted[i % len(accepted)], rejected[i % len(rejected)]):
            lines.append("%d %d %d %s %s %s" % (ecdsa.CURVES.index(grp["curve"]), grp["le"], k["use_cofactor"],
                                                k["Qx"], k["Qy"], k["d"]))
            want.append("%d %s" % (k["status"], k["shared"]))
    assert {g["curve"] for g in FX["groups"]} == set(CURVES)
    out = subprocess.run([exe, "dh"], input="\n".join(lines).encode(), stdout=subprocess.PIPE, check=True)
    assert out.stdout.decode().splitlines() == want
