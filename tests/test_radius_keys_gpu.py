"""Key tables of the RADIUS library (include/lcb_radius_gpu.h,
liblcb_amd.radius_batch), which repacks the caller's table for its own
password kernel (MD5(secret || 16 bytes) per 16-byte block) and hands the
caller's table on to the keyed batches, against the REFERENCE:

  tests/golden/radius.json       its 481 packets, their five secrets hidden in
                                 a 300-key table of decoys at shuffled, gapped
                                 key_offsets
  tests/golden/radius_keys.json  306 packets it signed and verified with 17
                                 secrets of 1..200 bytes on MD5's block and
                                 padding boundaries (make_golden_radius_keys.py)

and key_offsets None with several keys (every key starts at the table's first
byte).  The CPU test pins radius_keys.json to the oracle-backed host logic
(liblcb_amd.radius) before any GPU sees it.
"""
import json
import os

import numpy as np
import pytest

from tests.test_radius_batch_gpu import _find, _reqs, gaps_intact, run

G = os.path.join(os.path.dirname(__file__), "golden")
SECRET_LENGTHS = [1, 39, 40, 47, 48, 49, 55, 56, 63, 64, 65, 103, 104, 111, 112, 128, 200]


def _load(name):
    j = json.load(open(os.path.join(G, name)))
    j["secrets"] = [bytes.fromhex(s) for s in j["secrets"]]
    return j


@pytest.fixture(scope="module")
def rad():
    return _load("radius.json")


@pytest.fixture(scope="module")
def radk():
    return _load("radius_keys.json")


def _passwords_decoded(P, out):
    """The verified packets hold the plaintext the reference encoded -> how many."""
    n = 0
    for p, o in zip(P, out):
        if p["kind"] == "request" and p.get("password"):
            pw = bytes.fromhex(p["password"])
            a = _find(o, 2)
            assert o[a + 2:a + 2 + len(pw)] == pw
            assert not any(o[a + 2 + len(pw):a + o[a + 1]])        # zero padding to 16 bytes
            n += 1
    return n


# ---------------------------------------------------------------- decoy table
def decoy_table(secrets, nkeys=300, seed=300):
    """(key_table, where): `secrets` at random indices `where` of a table of
    nkeys keys, the others random decoys of 0..140 bytes; the keys lie in the
    blob in shuffled order with 0..9 decoy bytes between them."""
    rng = np.random.default_rng(seed)
    where = sorted(rng.permutation(nkeys)[:len(secrets)].tolist())
    where = [where[i] for i in rng.permutation(len(secrets))]          # secret j is key where[j]
    keys = [rng.integers(0, 256, int(rng.integers(0, 141)), dtype=np.uint8).tobytes() for _ in range(nkeys)]
    for j, k in enumerate(where):
        keys[k] = secrets[j]
    klen = np.array([len(k) for k in keys], np.uint32)
    koff = np.zeros(nkeys, np.uint64)
    pos = int(rng.integers(1, 10))
    for k in rng.permutation(nkeys):
        koff[k] = pos
        pos += len(keys[k]) + int(rng.integers(0, 10))
    blob = rng.integers(0, 256, pos + 5, dtype=np.uint8)
    for k in range(nkeys):
        blob[int(koff[k]):int(koff[k]) + len(keys[k])] = np.frombuffer(keys[k], np.uint8)
    return (blob, koff, klen), where


def test_decoy_table_geometry(rad):
    (blob, koff, klen), where = decoy_table(rad["secrets"])
    o = koff.astype(np.int64)
    assert len(klen) == 300 and (np.diff(o) < 0).sum() > 100 and (np.diff(o) > 0).sum() > 100
    assert int((koff + klen).max()) <= blob.size and len(set(where)) == 5
    order = np.argsort(o)
    assert (o[order][1:] >= (o + klen)[order][:-1]).all()             # no overlap: gaps only
    assert ((o[order][1:] - (o + klen)[order][:-1]) > 0).sum() > 100
    for s, k in zip(rad["secrets"], where):
        assert bytes(blob[int(koff[k]):int(koff[k]) + int(klen[k])]) == s


@pytest.mark.gpu
@pytest.mark.parametrize("reps", [1, 9])           # 481 and 4,329 packets: per-lane and tile keyed kernels
@pytest.mark.parametrize("device", [True, False])
def test_decoy_table_matches_reference(gpu, rad, device, reps):
    """The fixture's packets signed and verified with their secrets at
    remapped indices of a 300-key table given as key_table=: the library's
    own repacked table (password kernel) and the hash library's (keyed HMAC
    and suffix passes; two prep blocks of 64 keys and more) must both find
    the right bytes."""
    from liblcb_amd import radius_batch as rb
    table, where = decoy_table(rad["secrets"])
    P = rad["packets"] * reps
    kidx = [where[p["key"]] for p in P]
    err, got, _, after, offs, bsz = run(rb, False, device, [bytes.fromhex(p["pre"]) for p in P], None, kidx,
                                        seed=reps, key_table=table)
    assert err == [0] * len(P)
    bad = [i for i, p in enumerate(P) if got[i].hex() != p["signed"]]
    assert not bad, (len(bad), [(P[i]["code"], P[i]["key"], P[i]["msg_authr"]) for i in bad[:10]])
    assert gaps_intact(after, offs, bsz)
    err, out, _, after, offs, bsz = run(rb, True, device, [bytes.fromhex(p["signed"]) for p in P], None, kidx,
                                        _reqs(P), seed=reps + 100, key_table=table)
    assert err == [0] * len(P)
    bad = [i for i, p in enumerate(P) if out[i].hex() != p["verified"]]
    assert not bad, (len(bad), [(P[i]["code"], P[i]["key"], P[i]["msg_authr"]) for i in bad[:10]])
    assert _passwords_decoded(P[:481], out) > 50
    assert gaps_intact(after, offs, bsz)


# ------------------------------------------------- secrets on block boundaries
def test_radius_keys_fixture_shape(radk):
    """Every secret length of the issue is there (the reference refused
    none), with the packet shapes listed in make_golden_radius_keys.py."""
    assert [len(s) for s in radk["secrets"]] == SECRET_LENGTHS == radk["secret_lengths"]
    P = radk["packets"]
    assert len(P) == 18 * len(SECRET_LENGTHS)
    for k in range(len(SECRET_LENGTHS)):
        mine = [p for p in P if p["key"] == k]
        reqs = [p for p in mine if p["kind"] == "request"]
        assert sorted((p["code"], len(p["password"] or "") // 2, p["msg_authr"]) for p in reqs) == \
            sorted([(1, n, ma) for n in (1, 16, 17, 128) for ma in (0, 1)] + [(4, 0, 0)])
        reps = [p for p in mine if p["kind"] == "reply"]
        assert sorted(p["request"] for p in reps) == sorted(p["signed"] for p in reqs)


@pytest.fixture
def oracle_keyed(monkeypatch, oracle):
    """liblcb_amd.radius with its keyed batches served by the oracle (as in
    tests/test_radius_gpu.py)."""
    import liblcb_amd.radius as R

    def fake(alg, mode, keys, data, key_index=None, offsets=None, lengths=None, **kw):
        return oracle.batch_keyed(alg, mode, keys, data, key_index, offsets, lengths)
    monkeypatch.setattr(R, "hash_batch_keyed", fake)
    return R


def _check_host_model(R, radk, **kw):
    P = radk["packets"]
    kidx = [p["key"] for p in P]
    err, got = R.radius_pkt_sign_batch([bytes.fromhex(p["pre"]) for p in P], radk["secrets"], kidx, **kw)
    assert err.tolist() == [0] * len(P)
    bad = [i for i, p in enumerate(P) if got[i].hex() != p["signed"]]
    assert not bad, (len(bad), [(P[i]["code"], len(radk["secrets"][P[i]["key"]])) for i in bad[:10]])
    err, out = R.radius_pkt_verify_batch([bytes.fromhex(p["signed"]) for p in P], radk["secrets"], kidx, _reqs(P),
                                         **kw)
    assert err.tolist() == [0] * len(P)
    assert [o.hex() for o in out] == [p["verified"] for p in P]
    assert _passwords_decoded(P, out) == 8 * len(SECRET_LENGTHS)


def test_radius_keys_host_logic(oracle_keyed, radk):
    """CPU: the new fixture against the CPU restatement of the hashes under
    the host packet logic."""
    _check_host_model(oracle_keyed, radk)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
def test_radius_keys_host_model_on_gpu(gpu, radk, device):
    """liblcb_amd.radius: the User-Password chain as keyed-prefix batches of
    the hash library (mid-state after the secret's whole blocks, the rest of
    the secret and 16 bytes as one virtual message)."""
    import liblcb_amd.radius as R
    _check_host_model(R, radk, device=device)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
def test_radius_keys_match_reference(gpu, radk, device):
    """sign_packed / verify_packed reproduce the reference byte for byte for
    secrets of every boundary length: radius_password_kernel's
    MD5(secret || 16 bytes) with the terminator and length in the same or the
    next block, keyed HMAC with a key of one block, one byte more and longer,
    the secret as a suffix across the last block."""
    from liblcb_amd import radius_batch as rb
    P = radk["packets"]
    kidx = [p["key"] for p in P]
    err, got, _, after, offs, bsz = run(rb, False, device, [bytes.fromhex(p["pre"]) for p in P], radk["secrets"],
                                        kidx, seed=17)
    assert err == [0] * len(P)
    bad = [i for i, p in enumerate(P) if got[i].hex() != p["signed"]]
    assert not bad, (len(bad), [(P[i]["code"], len(radk["secrets"][P[i]["key"]])) for i in bad[:10]])
    assert gaps_intact(after, offs, bsz)
    err, out, _, after, offs, bsz = run(rb, True, device, [bytes.fromhex(p["signed"]) for p in P], radk["secrets"],
                                        kidx, _reqs(P), seed=18)
    assert err == [0] * len(P)
    bad = [i for i, p in enumerate(P) if out[i].hex() != p["verified"]]
    assert not bad, (len(bad), [(P[i]["code"], len(radk["secrets"][P[i]["key"]])) for i in bad[:10]])
    assert _passwords_decoded(P, out) == 8 * len(SECRET_LENGTHS)
    assert gaps_intact(after, offs, bsz)


# -------------------------------------------------------- key_offsets None
def test_host_wrapper_passes_null_key_offsets(monkeypatch):
    """CPU: the host-mode branch of sign_packed / verify_packed hands the key
    table on as it is -- a NULL key_offsets pointer for offsets None, the
    caller's arrays otherwise (the library is replaced by a recorder)."""
    from liblcb_amd import radius_batch as rb
    seen = []

    class Recorder:
        def radius_pkt_sign_batch(self, *a):
            seen.append(a)
            return 0
        radius_pkt_verify_batch = radius_pkt_sign_batch
    monkeypatch.setattr(rb, "radius_lib", lambda: Recorder())
    pk = np.zeros(4 * 64, np.uint8)
    blob, klen = np.arange(50, dtype=np.uint8), np.array([50, 7, 20], np.uint32)
    koff = np.array([0, 40, 3], np.uint64)
    for fn, at in ((rb.sign_packed, 6), (rb.verify_packed, 6)):
        for ko in (None, koff):
            err = fn(pk, None, count=4, stride=64, fixed_size=64, key_table=(blob, ko, klen))
            assert err.shape == (4,) and err.dtype == np.int32
            a = seen.pop()
            assert a[at] == blob.ctypes.data and a[at + 2] == klen.ctypes.data and a[at + 3] == 3
            assert a[at + 1] == (None if ko is None else ko.ctypes.data)
    assert not seen


@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
def test_null_key_offsets_several_keys(gpu, rad, device):
    """key_offsets None with three keys of different lengths: every key
    starts at the table's first byte (include/lcb_radius_gpu.h), so the
    packets equal those of the same call with an explicit all-zero offsets
    array.  Key 0 is the whole blob, the fixture's 100-byte secret, so the
    packets signed with it are also checked against the fixture.  Device and
    host mode (the wrapper passes a NULL pointer on in both)."""
    from liblcb_amd import radius_batch as rb
    blob = np.frombuffer(rad["secrets"][4], np.uint8)
    klen = np.array([100, 37, 5], np.uint32)
    P = rad["packets"]
    # the fixture's packets of secret 4 keep it (key 0); the others are signed with its 37- and 5-byte prefixes
    kidx = [0 if p["key"] == 4 else 1 + i % 2 for i, p in enumerate(P)]
    assert kidx.count(0) > 50 and kidx.count(1) > 50 and kidx.count(2) > 50
    pre = [bytes.fromhex(p["pre"]) for p in P]
    err, got, _, after, offs, bsz = run(rb, False, device, pre, None, kidx, seed=31, key_table=(blob, None, klen))
    assert err == [0] * len(P) and gaps_intact(after, offs, bsz)
    err, want, _, _, _, _ = run(rb, False, device, pre, None, kidx, seed=31,
                                key_table=(blob, np.zeros(3, np.uint64), klen))
    assert err == [0] * len(P)
    assert got == want
    for k in (0, 1, 2):                                                   # signing changed packets of every key
        assert sum(1 for g, p, kk in zip(got, pre, kidx) if kk == k and g != p) > 40
    for p, g, k in zip(P, got, kidx):
        if k == 0:
            assert g.hex() == p["signed"]
    # and back: verify with the same table decodes what sign encoded
    err, out, _, _, _, _ = run(rb, True, device, got, None, kidx, _reqs(P), seed=32, key_table=(blob, None, klen))
    assert err == [0] * len(P)
    for p, o, k in zip(P, out, kidx):
        if k == 0:
            assert o.hex() == p["verified"]
