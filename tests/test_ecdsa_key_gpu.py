"""Batched public-key import and export on the MI355X
(include/lcb_ecdsa_key_gpu.h) against the reference-generated fixture
tests/golden/ecdsa_key.json (every status and byte there is what the reference
returned and wrote) and, for keys the tests make themselves, the signing
library's pub_key_batch and the verification library.

One lane serves one item, so the shapes that matter are counts around the
64-lane wave (1, 63, 64, 65, 129) with every key form and every kind of
refused key sharing a wave, both byte orders, both memory modes, the strides
33, 65 and 80 with one size for all and a size per item, and the curves with
p = 1 (mod 8), whose square root takes the Tonelli-Shanks steps."""
import errno
import json
import os
import random
import subprocess

import numpy as np
import pytest

from tests import ecdsa_key_cases as KC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = KC.load()
GROUP_IDS = ["%s-%s" % (g["curve"], "le" if g["le"] else "be") for g in FX["groups"]]
EINVAL = errno.EINVAL
TS_B = "id-gostR3410-2001-CryptoPro-B-ParamSet"      # p = 1 (mod 8), p - 1 = 2^3 odd
TS_T = "id-gostR3410-2001-Test_ParamSet"             # p = 1 (mod 8), p - 1 = 2^4 odd
FILL = 0xA5
LIBDIR = os.path.join(ROOT, "liblcb_amd")


@pytest.fixture(scope="module")
def K(gpu):
    from liblcb_amd import ecdsa_key
    ecdsa_key.ecdsa_key_lib()
    return ecdsa_key


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


def dev(torch, a):
    return torch.as_tensor(np.array(a), device="cuda:0")


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def group(name, le):
    return next(g for g in FX["groups"] if g["curve"] == name and g["le"] == le)


def pack(recs, stride, fill=0xEE):
    """(keys (n, stride) with filler past every key, sizes (n,), keys_y (n, 32))."""
    keys = np.full((len(recs), stride), fill, np.uint8)
    keys_y = np.full((len(recs), 32), fill, np.uint8)
    for i, k in enumerate(recs):
        b = k["key"][:stride]
        keys[i, :len(b)] = np.frombuffer(b, np.uint8)
        if k["key_y"] is not None:
            keys_y[i] = np.frombuffer(k["key_y"], np.uint8)
    return keys, np.array([len(k["key"]) for k in recs], np.uint32), keys_y


def want_of(recs, stride=80, with_y=True):
    """(status, x || y, infinity) by the fixture; an item past the stride, or
    of size 32 without keys_y, is EINVAL with zeros."""
    st, xy, inf = [], [], []
    for k in recs:
        bad = len(k["key"]) > stride or (len(k["key"]) == 32 and not with_y)
        st.append(EINVAL if bad else k["status"])
        xy.append(KC.ZERO64 if bad else k["xy"])
        inf.append(0 if bad else k["infinity"])
    return np.array(st, np.int32), np.frombuffer(b"".join(xy), np.uint8).reshape(-1, 64), np.array(inf, np.uint8)


def check_import(what, recs, got, want):
    (pub, st, inf), (wst, wxy, winf) = got, want
    pub, st = host(pub), host(st)
    bad = [(k["name"], int(s), int(w)) for k, s, w in zip(recs, st, wst) if s != w]
    assert not bad, (what, bad[:6])
    bad = [(k["name"], bytes(g).hex(), bytes(w).hex()) for k, g, w in zip(recs, pub, wxy) if bytes(g) != bytes(w)]
    assert not bad, (what, bad[:4])
    if inf is not None:
        assert np.array_equal(host(inf), winf), what
    assert len(st) == len(recs)


def run_import(K, torch, grp, recs, stride, on_device, with_y=True, per_item=True, want_infinity=True):
    keys, sizes, keys_y = pack(recs, stride)
    mv = (lambda a: dev(torch, a)) if on_device else (lambda a: a)
    got = K.import_batch(grp["curve"], mv(keys), key_stride=stride,
                         sizes=mv(sizes.astype(np.int32)) if per_item else None,
                         key_size=None if per_item else int(sizes[0]), keys_y=mv(keys_y) if with_y else None,
                         le=grp["le"], want_infinity=want_infinity)
    if on_device:
        torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("on_device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("gi", range(len(FX["groups"])), ids=GROUP_IDS)
def test_fixture_groups(K, torch_, gi, on_device):
    grp = FX["groups"][gi]
    with_y = [k for k in grp["imports"] if not (len(k["key"]) == 32 and k["key_y"] is None)]
    no_y = [k for k in grp["imports"] if k["key_y"] is None]
    assert len(with_y) + 11 == len(grp["imports"]) and len(no_y) > 100
    check_import("keys_y given", with_y, run_import(K, torch_, grp, with_y, 80, on_device), want_of(with_y))
    check_import("keys_y NULL", no_y, run_import(K, torch_, grp, no_y, 80, on_device, with_y=False),
                 want_of(no_y, with_y=False))
    mv = (lambda a: dev(torch_, a)) if on_device else (lambda a: a)
    for form in (K.PACKED, K.COMPRESSED):
        ex = [k for k in grp["exports"] if k["compress"] == form]
        xy = np.frombuffer(b"".join(k["xy"] for k in ex), np.uint8)
        out, sizes, st = K.export_batch(grp["curve"], mv(xy), form=form, le=grp["le"],
                                        infinity=mv(np.array([k["infinity"] for k in ex], np.uint8)))
        if on_device:
            torch_.cuda.synchronize()
        got = [bytes(r[:n]) for r, n in zip(host(out), host(sizes).tolist())]
        assert got == [k["out"] for k in ex], [k["name"] for k, g in zip(ex, got) if g != k["out"]]
        assert not host(st).any() and out.shape == (len(ex), K.FORM_SIZE[form])


@pytest.mark.parametrize("name,le", [("secp256r1", False), (TS_T, True), (TS_B, False)])
def test_all_forms_shuffled_into_one_call(K, torch_, name, le):
    grp = group(name, le)
    recs = [k for k in grp["imports"] if not (len(k["key"]) == 32 and k["key_y"] is None)]
    ordered = list(recs)
    for seed in range(64):                                 # the first order whose first wave holds every form
        recs = list(ordered)
        random.Random(seed).shuffle(recs)
        if {1, 32, 33, 64, 65} <= {len(k["key"]) for k in recs[:64]}:
            break
    assert {1, 32, 33, 64, 65} <= {len(k["key"]) for k in recs[:64]}       # one wave mixes them
    assert {0, -1, EINVAL} <= {k["status"] for k in recs[:64]}
    for count in (1, 63, 64, 65, 129):
        sub = recs[:count]
        check_import(count, sub, run_import(K, torch_, grp, sub, 80, True), want_of(sub))
    sub = recs[7:7 + 65]
    check_import("host 65", sub, run_import(K, torch_, grp, sub, 80, False), want_of(sub))


@pytest.mark.parametrize("on_device", [True, False], ids=["device", "host"])
def test_strides_and_sizes(K, torch_, on_device):
    grp = group(TS_B, True)
    recs = [k for k in grp["imports"] if k["key_y"] is None and len(k["key"]) != 32]
    for stride, size in ((33, 33), (65, 65), (80, 33), (80, 65), (80, 64), (65, 1), (1, 1)):
        sub = [k for k in recs if len(k["key"]) == size]                   # one size for all: sizes == NULL
        assert len(sub) >= 2
        check_import((stride, size), sub, run_import(K, torch_, grp, sub, stride, on_device, with_y=False,
                                                     per_item=False), want_of(sub, stride))
    for stride in (33, 65, 80):                                            # a size per item, some past the stride
        want = want_of(recs, stride)
        past = sum(1 for k in recs if len(k["key"]) > stride)
        assert (past > 0) == (stride < 80) and int((want[0] == 0).sum()) > 10
        check_import(stride, recs, run_import(K, torch_, grp, recs, stride, on_device, with_y=False),
                     want)
    # key_size past the stride with sizes == NULL: every item EINVAL, nothing read
    sub = [k for k in recs if len(k["key"]) == 65][:3]
    got = run_import(K, torch_, grp, sub, 33, on_device, with_y=False, per_item=False)
    assert (host(got[1]) == EINVAL).all() and not host(got[0]).any() and not host(got[2]).any()


def test_infinity_null(K, torch_):
    grp = group("secp256k1", False)
    recs = [k for k in grp["imports"] if k["key_y"] is None and len(k["key"]) != 32]
    assert any(k["infinity"] for k in recs)
    for on_device in (True, False):
        got = run_import(K, torch_, grp, recs, 80, on_device, with_y=False, want_infinity=False)
        assert got[2] is None
        check_import("infinity NULL", recs, got, want_of(recs))


@pytest.mark.parametrize("name,le", [("secp256k1", False), ("id-gostR3410-2001-CryptoPro-A-ParamSet", True),
                                     (TS_T, False)])
def test_export_import_round_trip(K, torch_, name, le):
    from liblcb_amd import ecdsa_sign
    n = 1024
    rng = np.random.default_rng(0x6B32)
    priv = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    priv[:, 31 if le else 0] &= 0x3F                                      # below every n of the table
    pub, pst = ecdsa_sign.pub_key_batch(name, dev(torch_, priv.reshape(-1)), le=le)
    assert not host(pst).any()
    hp = host(pub)
    par = hp[:, 32 if le else 63] & 1
    assert 300 < int(par.sum()) < 724                                      # both roots are asked for
    for form in (K.COMPRESSED, K.PACKED):
        out, sizes, st = K.export_batch(name, pub.reshape(-1), form=form, le=le)
        back, bst, inf = K.import_batch(name, out, le=le)
        torch_.cuda.synchronize()
        ho = host(out)
        assert (host(sizes) == K.FORM_SIZE[form]).all() and not host(st).any()
        if form == K.COMPRESSED:
            assert np.array_equal(ho[:, 0], 2 | par) and np.array_equal(ho[:, 1:], hp[:, :32])
        else:
            assert (ho[:, 0] == 4).all() and np.array_equal(ho[:, 1:], hp)
        assert not host(bst).any() and not host(inf).any() and np.array_equal(host(back), hp)
    # the other prefix: the other root, x unchanged, and a different y
    out, _, _ = K.export_batch(name, pub.reshape(-1), form=K.COMPRESSED, le=le)
    out[:, 0] ^= 1
    back, bst, _ = K.import_batch(name, out, le=le)
    hb = host(back)
    assert not host(bst).any() and np.array_equal(hb[:, :32], hp[:, :32])
    assert np.array_equal(hb[:, 32 if le else 63] & 1, par ^ 1)


def test_verify_wire_over_the_signing_fixture(K, torch_):
    from liblcb_amd import ecdsa_sign
    with open(os.path.join(ROOT, "tests", "golden", "ecdsa_sign.json")) as f:
        sfx = json.load(f)
    verified = 0
    for grp in sfx["groups"]:
        name, le = grp["curve"], bool(grp["le"])
        cat = lambda recs, *fs: dev(torch_, np.frombuffer(  # noqa: E731
            bytes.fromhex("".join("".join(k[f] for f in fs) for k in recs)), np.uint8))
        for hs in sorted({k["hash_size"] for k in grp["sign"]}):
            recs = [k for k in grp["sign"] if k["hash_size"] == hs and k["status"] == 0 and int(k["d"], 16) != 0]
            if not recs:
                continue
            pub, pst = ecdsa_sign.pub_key_batch(name, cat(recs, "d"), le=le)
            assert not host(pst).any()
            wire, _, _ = K.export_batch(name, pub.reshape(-1), form=K.COMPRESSED, le=le)
            vst, kst = K.verify_wire(name, cat(recs, "hash"), cat(recs, "r", "s"), wire, le=le, hash_size=hs)
            assert not host(vst).any() and not host(kst).any(), (name, le, hs)
            # through key_idx, reversed, with one key of an unknown prefix
            n = len(recs)
            wire[0, 0] = 5
            idx = dev(torch_, np.arange(n - 1, -1, -1, dtype=np.int32))
            rev = recs[::-1]
            vst, kst = K.verify_wire(name, cat(rev, "hash"), cat(rev, "r", "s"), wire, key_idx=idx, le=le,
                                     hash_size=hs)
            assert host(kst).tolist() == [-1] + [0] * (n - 1) and host(vst).tolist() == [0] * (n - 1) + [-1]
            verified += n
    assert verified > 100


def test_host_mode_across_a_chunk_boundary(K, torch_):
    grp = group(TS_B, True)
    k = next(k for k in grp["imports"] if k["name"] == "rand0/compressed_other")
    n = (1 << 18) + 65
    keys = np.tile(np.frombuffer(k["key"], np.uint8), n)
    pub, st, inf = K.import_batch(grp["curve"], keys, key_size=33, le=True)
    assert st.shape == (n,) and not st.any() and not inf.any()
    assert (pub == np.frombuffer(k["xy"], np.uint8)).all()
    out, sizes, est = K.export_batch(grp["curve"], pub.reshape(-1), form=K.COMPRESSED, le=True)
    assert (sizes == 33).all() and not est.any() and (out == np.frombuffer(k["key"], np.uint8)).all()


@pytest.mark.parametrize("on_device", [True, False], ids=["device", "host"])
def test_bytes_past_an_exported_item_are_untouched(K, torch_, on_device):
    grp = group("brainpoolP256r1", False)
    ex = [k for k in grp["exports"]]
    xy = np.frombuffer(b"".join(k["xy"] for k in ex), np.uint8)
    inf = np.array([k["infinity"] for k in ex], np.uint8)
    mv = (lambda a: dev(torch_, a)) if on_device else (lambda a: a)
    for form in (K.PACKED, K.COMPRESSED):
        for stride in (K.FORM_SIZE[form], 80):
            buf = mv(np.full(len(ex) * stride + 16, FILL, np.uint8))
            out, sizes, st = K.export_batch(grp["curve"], mv(xy), form=form, infinity=mv(inf), out_stride=stride,
                                            out=buf)
            if on_device:
                torch_.cuda.synchronize()
            hb, hs = host(buf), host(sizes).tolist()
            want = [1 if i else K.FORM_SIZE[form] for i in inf]
            assert hs == want and (hb[len(ex) * stride:] == FILL).all() and not host(st).any()
            for i, k in enumerate(ex):
                row = hb[i * stride:(i + 1) * stride]
                assert (row[hs[i]:] == FILL).all(), (form, stride, k["name"])
                if k["compress"] == form:
                    assert bytes(row[:hs[i]]) == k["out"], (form, stride, k["name"])


def test_c_caller_agrees_per_group(K, tmp_path):
    """A plain C program: host-mode import, then export, through the reference-named entry points."""
    from liblcb_amd import ecdsa
    exe = str(tmp_path / "ecdsa_key_caller")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "ecdsa_key_caller.c"), "-o", exe,
                           "-L" + LIBDIR, "-llcb_ecdsa_key_gpu", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath-link," + LIBDIR + ":/opt/rocm/lib"])
    lines, want = [], []
    for i, grp in enumerate(FX["groups"]):
        recs = [k for k in grp["imports"] if k["key_y"] is None and len(k["key"]) not in (0, 32)]
        accepted = [k for k in recs if k["status"] == 0 and not k["infinity"]]
        rejected = [k for k in recs if k["status"] != 0]
        infinite = [k for k in recs if k["infinity"]]
        # of every group an accepted compressed key, another accepted form, a refused key and the point at infinity
        comp = [k for k in accepted if len(k["key"]) == 33]
        for k in (comp[i % len(comp)], accepted[(7 * i) % len(accepted)], rejected[(5 * i) % len(rejected)],
                  infinite[0]):
            lines.append("%d %d %s" % (ecdsa.CURVES.index(grp["curve"]), grp["le"], k["key"].hex()))
            y_low = k["xy"][32 if grp["le"] else 63] & 1
            form = b"\x00" if k["infinity"] else bytes([2 | y_low]) + k["xy"][:32]   # what the export writes for x || y
            want.append("%d %d %s %d %s" % (k["status"], k["infinity"], k["xy"].hex(), len(form), form.hex()))
    assert len({g["curve"] for g in FX["groups"]}) == 10
    out = subprocess.run([exe, "import"], input="\n".join(lines).encode(), stdout=subprocess.PIPE, check=True)
    assert out.stdout.decode().splitlines() == want
