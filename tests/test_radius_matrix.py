"""The RADIUS code tables and packet geometry against the REFERENCE called
without its semantic filter: tests/golden/radius_matrix.json holds what
radius_pkt_sign and radius_pkt_verify (NOT behind radius_pkt_chk) return for
20 codes x 13 attribute layouts x 7 requests, and SHA-256 of the buffers they
leave (tests/golden/make_golden_radius_matrix.py; the packets are rebuilt by
tests/radius_matrix_util.py).  Codes radius.h does not know, replies paired
with a request of another family, code 5 with and without Status-Server, two
Message-Authenticators, two User-Passwords, attributes of refused lengths, a
20-byte packet and two 4096-byte ones (2022 attributes; 255-byte attributes).

CPU: the fixture's shape, and liblcb_amd.radius (the host model) with its
keyed batches served by the oracle.  GPU: liblcb_amd.radius_batch
(liblcb_radius_gpu.so) over the whole matrix as one batch, in device and host
mode, below and above the count at which the keyed batches switch kernels,
across host-mode staging chunks that one packet fills exactly, and the rule
that a request record with code 0 is no request.
"""
import errno
import hashlib
import os

import numpy as np
import pytest

from tests import radius_matrix_util as M
from tests.test_radius_batch_gpu import gaps_intact, run

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "radius_matrix.json")
KINDS = {"sign": ("sign", "signed_sha256"), "verify": ("verify", "verified_sha256"),
         "tampered": ("tampered", "tampered_sha256")}
# lcb_internal.hpp kBucketMinCount: from this many messages on, a keyed batch
# with a length array is bucketed and goes to the tile kernel.
TILE_MIN_COUNT = 4096
# lcb_radius_gpu.cpp chunk_bytes(): LCB_RADIUS_CHUNK_BYTES is clamped to at
# least kPktMax, so this is the smallest chunk, and a full packet fills it.
MIN_CHUNK_BYTES = 4096


def sha(b):
    return hashlib.sha256(b).hexdigest()


class Matrix:
    """The fixture and the packets rebuilt from its parameters.  signed /
    tam: the verify inputs as the host model makes them (they are the
    reference's bytes exactly when test_host_model_matches_reference passes;
    a GPU test checks the hashes of the ones it uses)."""

    def __init__(self, oracle, verify=True):
        import liblcb_amd.radius as R
        fx = M.load(FIXTURE)
        self.fx, self.secrets, self.cases = fx, fx["secrets"], fx["cases"]
        built = [M.build(c["index"], (c["code"], c["layout"], c["request"], c["key"])) for c in self.cases]
        self.pre = [b[0] for b in built]
        self.req = [b[1] for b in built]
        self.kidx = [c["key"] for c in self.cases]
        self.layout = [fx["layouts"][c["layout"]] for c in self.cases]

        def fake(alg, mode, keys, data, key_index=None, offsets=None, lengths=None, **kw):
            return oracle.batch_keyed(alg, mode, keys, data, key_index, offsets, lengths)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(R, "hash_batch_keyed", fake)
            self.sign_err, self.signed = R.radius_pkt_sign_batch(self.pre, self.secrets, self.kidx)
            self.tam = [M.tampered(s) for s in self.signed]
            if verify:
                self.ver_err, self.ver_out = R.radius_pkt_verify_batch(self.signed, self.secrets, self.kidx, self.req)
                self.tam_err, self.tam_out = R.radius_pkt_verify_batch(self.tam, self.secrets, self.kidx, self.req)

    def inputs(self, kind, idx=None):
        """The input packets of `kind` for the cases idx (default: all); the
        verify inputs must be what the reference signed."""
        idx = range(len(self.cases)) if idx is None else idx
        if kind == "sign":
            return [self.pre[i] for i in idx]
        for i in idx:
            c = self.cases[i]
            assert sha(self.signed[i]) == (c["signed_sha256"] or sha(self.pre[i])), ("host-model sign", i)
        return [(self.signed if kind == "verify" else self.tam)[i] for i in idx]

    def mismatches(self, kind, err, out, inp, idx=None):
        """The cases whose result code or buffer differs from the reference's:
        [(index, code, layout, request, got rc, want rc, buffer ok)]."""
        idx = range(len(self.cases)) if idx is None else idx
        rc_col, sha_col = KINDS[kind]
        bad = []
        for i, e, o, p in zip(idx, err, out, inp):
            c = self.cases[i]
            same = (o == p) if (c[sha_col] is None or c[rc_col]) else (sha(o) == c[sha_col])
            if int(e) != c[rc_col] or not same:
                bad.append((i, c["code"], self.layout[i], c["request"], int(e), c[rc_col], same))
        return bad


@pytest.fixture(scope="module")
def mx(oracle):
    return Matrix(oracle)


# ------------------------------------------------------------------- CPU
def test_fixture_shape(mx):
    fx, C = mx.fx, mx.cases
    assert fx["codes"] == M.CODES and fx["requests"] == M.REQUESTS and fx["layouts"] == M.LAYOUTS
    assert fx["secrets"] == M.secrets() and [len(s) for s in fx["secrets"]] == [1, 10, 64, 100]
    assert [(c["code"], c["layout"], c["request"], c["key"]) for c in C] == M.cases()
    assert {(c["code"], c["layout"], c["request"]) for c in C} == \
        {(a, b, r) for a in M.CODES for b in range(len(M.LAYOUTS)) for r in M.REQUESTS}
    assert {0, 1, 2, 3, 4, 5, 11, 12, 13, 40, 41, 42, 43, 44, 45} < set(M.CODES) and len(M.CODES) == 20
    assert len(M.LAYOUTS) >= 13 and set(M.REQUESTS) == {0, 1, 4, 12, 40, 43, 2}
    assert os.path.getsize(FIXTURE) < 256 << 10
    # every key under every layout and code
    assert {(c["layout"], c["key"]) for c in C} == {(b, k) for b in range(len(M.LAYOUTS)) for k in range(4)}
    M.conditions([(c["sign"], c["verify"], c["tampered"]) for c in C])
    # the packets: structurally good as built and tampered, the full ones exactly 4096 bytes
    for c, p, name in zip(C, mx.pre, mx.layout):
        A = M.walk(p)
        assert A is not None and M.walk(M.tampered(p)) is not None, c
        assert len(p) == int.from_bytes(p[2:4], "big") and p[0] == c["code"]
        if name in M.FULL_LAYOUTS:
            assert len(p) == 4096
        if name == "minimal":
            assert len(p) == 20
        # the tampered byte is attribute data or the authenticator, never structure
        assert len(p) == 20 or len(p) - 1 >= A[-1][0] + 2
    by = {name: M.walk(p) for name, p in zip(mx.layout, mx.pre)}
    assert len(by["full_two_byte"]) == 2022 and [a[2] for a in by["full_two_byte"]].count(2) == 2020
    assert [a[2] for a in by["full_255"]].count(255) == 15 and by["full_255"][-1][1:] == (80, 18)
    assert [a[1:] for a in by["two_ma"] if a[1] == 80] == [(80, 18)] * 2
    assert [a[1:] for a in by["ma17"] if a[1] == 80] == [(80, 17)]
    assert [a[1:] for a in by["badpw20_ma17"] if a[1] in (2, 80)] == [(2, 22), (80, 17)]
    assert [a[1:] for a in by["badpw17_ma"] if a[1] in (2, 80)] == [(2, 19), (80, 18)]
    assert len(M.full_two_byte_only()) == 4096 and len(M.walk(M.full_two_byte_only())) == 2038
    # the authenticator before signing, as radius_pkt_init leaves it
    for c, p, r in zip(C, mx.pre, mx.req):
        assert (r is None) == (c["request"] == 0) and (r is None or (r[0] == c["request"] and len(r) == 20))
        if c["code"] in (4, 40, 43):
            assert p[4:20] == bytes(16)
        elif c["code"] in (2, 3, 5, 11, 41, 42, 44, 45) and r is not None:
            assert p[4:20] == r[4:20]


def test_host_model_matches_reference(mx):
    """liblcb_amd.radius, keyed batches served by the oracle: the reference's
    code and buffer for sign, verify and verify of the tampered packet, for
    every case.  (Before radius_pkt_sign_batch refused a first
    Message-Authenticator whose length is not 18, this failed on the 140 cases
    of layout ma17: sign returned 0 and wrote 16 bytes across the attribute's
    end where the reference returns EBADMSG.)"""
    bad = mx.mismatches("sign", mx.sign_err, mx.signed, mx.pre)
    assert not bad, (len(bad), sorted({b[2] for b in bad}), bad[:5])
    bad = mx.mismatches("verify", mx.ver_err, mx.ver_out, mx.signed)
    assert not bad, (len(bad), sorted({b[2] for b in bad}), bad[:5])
    bad = mx.mismatches("tampered", mx.tam_err, mx.tam_out, mx.tam)
    assert not bad, (len(bad), sorted({b[2] for b in bad}), bad[:5])
    # two Message-Authenticators: the second one's nonzero bytes stayed through sign
    for i, name in enumerate(mx.layout):
        if name == "two_ma":
            a = [x for x in M.walk(mx.pre[i]) if x[1] == 80][1][0]
            assert mx.signed[i][a:a + 18] == mx.pre[i][a:a + 18] and 0 not in mx.pre[i][a + 2:a + 18]


# ------------------------------------------------------------------- GPU
def _three_kinds(mx, rb, device, layout, idx, seed, gap_max=16):
    """Sign, verify and verify-tampered of the cases idx as one batch each:
    the reference's codes and buffers, refused packets byte-identical, the
    canaries between the buffers intact.  -> {kind: (errors, buffers)}."""
    res = {}
    for k, kind in enumerate(KINDS):
        inp = mx.inputs(kind, idx)
        err, out, before, after, offs, bsz = run(
            rb, kind != "sign", device, inp, mx.secrets, [mx.kidx[i] for i in idx],
            [mx.req[i] for i in idx] if kind != "sign" else None, layout=layout, seed=seed + k, gap_max=gap_max)
        if layout == "offsets":
            assert set((offs % 16).tolist()) == set(range(16))          # every start phase mod 16
        bad = mx.mismatches(kind, err, out, inp, idx)
        assert not bad, (kind, len(bad), sorted({b[2] for b in bad}), bad[:5])
        for e, o, p in zip(err, out, inp):
            assert not e or o == p                                      # include/lcb_radius_gpu.h, difference 1
        assert gaps_intact(after, offs, bsz), kind
        res[kind] = (err, out)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["offsets", "stride"])
@pytest.mark.parametrize("device", [True, False])
def test_matrix_one_batch(gpu, mx, device, layout):
    from liblcb_amd import radius_batch as rb
    n = len(mx.cases)
    assert n < TILE_MIN_COUNT                       # the per-lane keyed kernels
    res = _three_kinds(mx, rb, device, layout, list(range(n)), seed=11)
    assert {0, errno.EBADMSG, errno.EOVERFLOW} == set(res["sign"][0])
    assert {0, errno.EBADMSG, errno.EINVAL} == set(res["verify"][0])


@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
def test_matrix_above_tile_threshold(gpu, mx, device):
    """The matrix three times over, 5,460 packets >= kBucketMinCount: the tile
    kernels of both keyed passes get 4096-byte lanes, mid-sized lanes and
    length-0 lanes (packets not in that pass) in the same tiles."""
    from liblcb_amd import radius_batch as rb
    n = len(mx.cases)
    reps = -(-TILE_MIN_COUNT // n)
    idx = [i for _ in range(reps) for i in range(n)]
    assert len(idx) >= TILE_MIN_COUNT
    _three_kinds(mx, rb, device, "offsets", idx, seed=21)


@pytest.mark.gpu
def test_verify_restores_the_matrix(gpu, mx):
    """Every case without a User-Password or with a nonzero verify code: the
    blob after verify equals the blob before, the two-Message-Authenticator
    packets included (second attribute not zeroed, first put back)."""
    from liblcb_amd import radius_batch as rb
    for kind in ("verify", "tampered"):
        idx = [i for i, c in enumerate(mx.cases)
               if c[KINDS[kind][0]] or not any(a[1] == 2 for a in M.walk(mx.pre[i]))]
        assert len(idx) > 1000 and sum(1 for i in idx if mx.layout[i] == "two_ma") == 140
        if kind == "verify":                    # some of them pass both checks: both fields substituted and put back
            assert sum(1 for i in idx if mx.cases[i]["verify"] == 0 and mx.layout[i] == "two_ma") >= 40
        inp = mx.inputs(kind, idx)
        err, out, before, after, offs, bsz = run(rb, True, True, inp, mx.secrets, [mx.kidx[i] for i in idx],
                                                 [mx.req[i] for i in idx], seed=31, gap_max=16)
        assert err == [mx.cases[i][KINDS[kind][0]] for i in idx]
        assert np.array_equal(before, after)


@pytest.mark.gpu
def test_host_mode_full_packets_across_chunks(gpu, mx, monkeypatch):
    """The 4096-byte packets in host mode with the smallest staging chunk (one
    packet fills it exactly) and with 8192: the one-chunk results."""
    from liblcb_amd import radius_batch as rb
    idx = [i for i, name in enumerate(mx.layout) if name in M.FULL_LAYOUTS]
    assert len(idx) == 280 and all(len(mx.pre[i]) == MIN_CHUNK_BYTES for i in idx)
    args = lambda kind: (mx.inputs(kind, idx), mx.secrets, [mx.kidx[i] for i in idx],      # noqa: E731
                         [mx.req[i] for i in idx] if kind != "sign" else None)
    monkeypatch.delenv("LCB_RADIUS_CHUNK_BYTES", raising=False)
    one = {kind: run(rb, kind != "sign", False, *args(kind), seed=41, gap_max=16)[:2] for kind in KINDS}
    for kind in KINDS:
        assert not mx.mismatches(kind, *one[kind], args(kind)[0], idx), kind
    for chunk in (MIN_CHUNK_BYTES, 8192):
        monkeypatch.setenv("LCB_RADIUS_CHUNK_BYTES", str(chunk))
        for kind in KINDS:
            err, out, before, after, offs, bsz = run(rb, kind != "sign", False, *args(kind), seed=41, gap_max=16)
            assert (err, out) == one[kind], (chunk, kind)
            assert gaps_intact(after, offs, bsz)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
def test_request_record_with_code_zero_is_no_request(gpu, mx, device):
    """req_hdrs rule of include/lcb_radius_gpu.h: a record whose code byte is 0
    stands for pkt_req == NULL whatever its other 19 bytes hold."""
    from liblcb_amd import radius_batch as rb
    idx = [i for i, c in enumerate(mx.cases) if c["request"] == 0]
    assert len(idx) == len(M.CODES) * len(M.LAYOUTS)
    inp = mx.inputs("verify", idx)
    recs = [bytes([0]) + bytes(x | 1 for x in M.request_header(i, 2)[1:]) for i in idx]
    err, out, _, _, _, _ = run(rb, True, device, inp, mx.secrets, [mx.kidx[i] for i in idx], recs, seed=51)
    assert not mx.mismatches("verify", err, out, inp, idx)
    assert errno.EINVAL in err and 0 in err
