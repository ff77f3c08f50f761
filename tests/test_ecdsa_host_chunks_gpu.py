"""Host mode (numpy in, numpy out) of the three ECDSA libraries where the
other tests never take it: across the staging chunk of 2^18 items, and through
a staging context that a later call has to grow.  Expectations are the
reference-generated fixtures tests/golden/ecdsa.json, ecdsa_sign.json and
ecdsa_dh.json, position by position; nothing here is compared with a
device-mode run.

COUNT = 2^18 + 65 is one full chunk, then a chunk of one full wave plus one
lane: the smallest count with a second iteration of the chunk loop (its
`i > 0` offsets into the caller's arrays), a final copy back that is shorter
than the staging buffers, and a masked tail wave.  With a key table the index
array holds one index equal to the table's length in each chunk."""
import errno
import json
import os
import threading

import numpy as np
import pytest

from tests import ecdsa_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


FX_V, FX_S, FX_D = M.load_fixture(), _load("ecdsa_sign.json"), _load("ecdsa_dh.json")
EINVAL = errno.EINVAL
CHUNK = 1 << 18
COUNT = CHUNK + 65
BAD_AT = (CHUNK - 7, CHUNK + 64)     # in the first chunk / the last lane of the second


@pytest.fixture(scope="module")
def E(gpu):
    from liblcb_amd import ecdsa
    ecdsa.ecdsa_lib()
    return ecdsa


@pytest.fixture(scope="module")
def S(gpu):
    from liblcb_amd import ecdsa_sign
    ecdsa_sign.ecdsa_sign_lib()
    return ecdsa_sign


@pytest.fixture(scope="module")
def D(gpu):
    from liblcb_amd import ecdsa_dh
    ecdsa_dh.ecdsa_dh_lib()
    return ecdsa_dh


def u8(h):
    return np.frombuffer(bytes.fromhex(h), np.uint8).copy()


def cat(recs, width, *fields):
    return u8("".join("".join(k[f] for f in fields) for k in recs)).reshape(-1, width)


def statuses(recs):
    return np.array([k["status"] for k in recs], np.int32)


def group(groups, name, le):
    return next(g for g in groups if g["curve"] == name and bool(g["le"]) == le)


def cycle(count, nrec):
    """Record of every item: the records repeated, starting at another record for each count."""
    return (np.arange(count) + count) % nrec


def same(what, got, want):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = np.nonzero((got != want).reshape(len(want), -1).any(axis=1))[0]
    assert diff.size == 0, (what, diff.size, diff[:8].tolist())


def with_bad(idx, nkeys, at):
    """idx as the index array of a table of nkeys keys, one past the table at `at`."""
    kidx = idx.astype(np.uint32)
    kidx[list(at)] = nkeys
    return kidx


def verify_arrays(name, le):
    recs = [k for k in group(FX_V["cases"], name, le)["records"] if k["hash_size"] == 32]
    assert {0, -1, -2, EINVAL} <= {k["status"] for k in recs}
    hashes = u8("".join(k["hash"][:64] for k in recs)).reshape(-1, 32)    # a record may carry more than it passes
    return hashes, cat(recs, 64, "r", "s"), cat(recs, 64, "Qx", "Qy"), statuses(recs)


def sign_arrays(name, le):
    recs = [k for k in group(FX_S["groups"], name, le)["sign"] if k["hash_size"] == 32]
    assert {0, -1, EINVAL} <= {k["status"] for k in recs}
    return cat(recs, 32, "hash"), cat(recs, 32, "d"), cat(recs, 32, "rnd"), cat(recs, 64, "r", "s"), statuses(recs)


def dh_arrays(name, le):
    recs = group(FX_D["groups"], name, le)["records"]
    assert {0, -1, EINVAL} <= {k["status"] for k in recs}
    return cat(recs, 64, "Qx", "Qy"), cat(recs, 32, "d"), cat(recs, 32, "shared"), statuses(recs)


# ------------------------------------------------- a. across the chunk boundary
def test_verify_across_the_chunk(E):
    name, le = "secp256r1", False
    h, s, q, w = verify_arrays(name, le)
    idx = cycle(COUNT, len(w))
    hashes, sigs = h[idx].reshape(-1), s[idx].reshape(-1)
    st = E.verify_batch(name, hashes, sigs, q[idx].reshape(-1), le=le)
    assert isinstance(st, np.ndarray) and st.dtype == np.int32
    same("per-item keys", st, w[idx])
    want = w[idx].copy()
    want[list(BAD_AT)] = EINVAL
    st = E.verify_batch(name, hashes, sigs, q.reshape(-1), key_idx=with_bad(idx, len(w), BAD_AT), le=le)
    same("key table", st, want)


def test_sign_across_the_chunk(S):
    name, le = "id-gostR3410-2001-CryptoPro-A-ParamSet", True
    h, d, k, rs, w = sign_arrays(name, le)
    idx = cycle(COUNT, len(w))
    hashes, rnd = h[idx].reshape(-1), k[idx].reshape(-1)
    sigs, st = S.sign_batch(name, hashes, d[idx].reshape(-1), rnd, le=le)
    assert isinstance(st, np.ndarray) and isinstance(sigs, np.ndarray)
    same("per-item keys: status", st, w[idx])
    same("per-item keys: r || s", sigs, rs[idx])
    want_st, want = w[idx].copy(), rs[idx].copy()
    want_st[list(BAD_AT)], want[list(BAD_AT)] = EINVAL, 0
    sigs, st = S.sign_batch(name, hashes, d.reshape(-1), rnd, key_idx=with_bad(idx, len(w), BAD_AT), le=le)
    same("key table: status", st, want_st)
    same("key table: r || s", sigs, want)
    assert not sigs[list(BAD_AT)].any()


def test_key_gen_across_the_chunk(S):
    name, le = "brainpoolP256r1", False
    recs = group(FX_S["groups"], name, le)["key_gen"]
    idx = cycle(COUNT, len(recs))
    priv, pub, st = S.key_gen_batch(name, cat(recs, 32, "rnd")[idx].reshape(-1), le=le)
    assert isinstance(st, np.ndarray)
    same("status", st, statuses(recs)[idx])
    same("d", priv, cat(recs, 32, "d")[idx])
    same("Q", pub, cat(recs, 64, "Qx", "Qy")[idx])


def test_pub_key_across_the_chunk(S):
    name, le = "id-GostR3410-2001-ParamSet-cc", True
    recs = group(FX_S["groups"], name, le)["pub_key"]
    idx = cycle(COUNT, len(recs))
    pub, st = S.pub_key_batch(name, cat(recs, 32, "d")[idx].reshape(-1), le=le)
    assert isinstance(st, np.ndarray)
    same("status", st, statuses(recs)[idx])
    same("Q", pub, cat(recs, 64, "Qx", "Qy")[idx])


def test_dh_across_the_chunk(D):
    name, le = "secp256k1", False
    q, d, x, w = dh_arrays(name, le)
    idx = cycle(COUNT, len(w))
    shared, st = D.dh_batch(name, q[idx].reshape(-1), d[idx].reshape(-1), le=le)
    assert isinstance(st, np.ndarray) and isinstance(shared, np.ndarray)
    same("per-item keys: status", st, w[idx])
    same("per-item keys: shared", shared, x[idx])
    # both tables indexed; each index array is past its table once per chunk, at items of its own
    bad_q, bad_d = BAD_AT, (BAD_AT[0] - 64, BAD_AT[1] - 1)
    want_st, want = w[idx].copy(), x[idx].copy()
    for i in bad_q + bad_d:
        want_st[i], want[i] = EINVAL, 0
    shared, st = D.dh_batch(name, q.reshape(-1), d.reshape(-1), le=le, pub_idx=with_bad(idx, len(w), bad_q),
                            priv_idx=with_bad(idx, len(w), bad_d))
    same("key tables: status", st, want_st)
    same("key tables: shared", shared, want)
    assert not shared[list(bad_q + bad_d)].any()


# ------------------------------------ b. staging that shrinks and grows, one thread
# Three calls on one thread: 3 items with their own keys, 200 items over a
# table of five keys (both staging buffers have to be allocated again, larger,
# and the key buffers for the first time), 2 items with their own keys in the
# larger buffers.  The staging context belongs to the thread and only grows,
# and the thread that runs the tests has staged larger batches by now, so the
# three calls run on a thread of their own.  The five keys are those of five
# records spread over the group.
SIZES = (3, 200, 2)


def five_of(w):
    pick = np.linspace(0, len(w) - 1, 5).astype(np.int64)
    assert (w[pick] == 0).any() and (w[pick] != 0).any()
    return pick


def on_a_new_thread(body):
    """body() on a thread that has never staged anything; its exception is raised here."""
    box = []

    def run():
        try:
            body()
        except BaseException as e:  # noqa: B902 -- handed to the caller
            box.append(e)
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if box:
        raise box[0]


def test_verify_staging_grows_and_is_reused(E):
    name, le = "id-gostR3410-2001-CryptoPro-B-ParamSet", True
    h, s, q, w = verify_arrays(name, le)
    pick = five_of(w)

    def body():
        for count in SIZES:
            if count == 200:
                kidx = cycle(count, 5)
                idx = pick[kidx]
                st = E.verify_batch(name, h[idx].reshape(-1), s[idx].reshape(-1), q[pick].reshape(-1),
                                    key_idx=kidx.astype(np.uint32), le=le)
            else:
                idx = cycle(count, len(w))
                st = E.verify_batch(name, h[idx].reshape(-1), s[idx].reshape(-1), q[idx].reshape(-1), le=le)
            same(count, st, w[idx])
    on_a_new_thread(body)


def test_sign_staging_grows_and_is_reused(S):
    name, le = "secp256k1", False
    h, d, k, rs, w = sign_arrays(name, le)
    pick = five_of(w)

    def body():
        for count in SIZES:
            if count == 200:
                kidx = cycle(count, 5)
                idx = pick[kidx]
                sigs, st = S.sign_batch(name, h[idx].reshape(-1), d[pick].reshape(-1), k[idx].reshape(-1),
                                        key_idx=kidx.astype(np.uint32), le=le)
            else:
                idx = cycle(count, len(w))
                sigs, st = S.sign_batch(name, h[idx].reshape(-1), d[idx].reshape(-1), k[idx].reshape(-1), le=le)
            same((count, "status"), st, w[idx])
            same((count, "r || s"), sigs, rs[idx])
    on_a_new_thread(body)


def test_dh_staging_grows_and_is_reused(D):
    name, le = "id-gostR3410-2001-CryptoPro-XchA-ParamSet", True
    q, d, x, w = dh_arrays(name, le)
    pick = five_of(w)

    def body():
        for count in SIZES:
            if count == 200:
                kidx = cycle(count, 5)
                idx = pick[kidx]
                shared, st = D.dh_batch(name, q[pick].reshape(-1), d[pick].reshape(-1), le=le,
                                        pub_idx=kidx.astype(np.uint32), priv_idx=kidx.astype(np.uint32))
            else:
                idx = cycle(count, len(w))
                shared, st = D.dh_batch(name, q[idx].reshape(-1), d[idx].reshape(-1), le=le)
            same((count, "status"), st, w[idx])
            same((count, "shared"), shared, x[idx])
    on_a_new_thread(body)
