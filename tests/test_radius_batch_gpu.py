"""Batched radius_pkt_sign / radius_pkt_verify on the device
(include/lcb_radius_gpu.h, liblcb_amd.radius_batch) against the REFERENCE:

  tests/golden/radius.json        481 packets radius.h built, signed, verified
  tests/golden/radius_edge.json   its sign results for refused User-Passwords
                                  and for buffers longer than the packet
  tests/golden/radius_batch.json  its verify / sign results for tampered
                                  packets, missing or foreign requests and
                                  the wrong secret

in device and host mode, packed at every start phase and at a fixed stride,
below and above the batch size at which the keyed batches switch kernels; plus
the structural guard with canaries around every buffer, two streams over the
same inputs, in-place restoration and the wrapper's argument checks.
"""
import errno
import json
import os

import numpy as np
import pytest

G = os.path.join(os.path.dirname(__file__), "golden")
CANARY = 0x5A


@pytest.fixture(scope="module")
def rad():
    j = json.load(open(os.path.join(G, "radius.json")))
    j["secrets"] = [bytes.fromhex(s) for s in j["secrets"]]
    return j


def _reqs(P):
    return [bytes.fromhex(p["request"]) if p["kind"] == "reply" else None for p in P]


def _find(pkt, t):
    from liblcb_amd.radius import find_attr
    return find_attr(pkt, t)


def run(rb, verify, device, packets, keys, kidx, reqs=None, layout="offsets", seed=1, sizes=None, key_table=None,
        gap_max=7):
    """Sign or verify `packets` (list of bytes buffers) laid out with random
    0..gap_max-1-byte gaps (0..6: every start phase mod 8) or at stride 4096,
    canary bytes everywhere else; the secrets as the list `keys`, or keys None and
    key_table=(blob, key_offsets or None, key_lengths).
    -> (errors list, buffers list, blob before, blob after, offsets, buffer sizes)."""
    import torch
    n = len(packets)
    rng = np.random.default_rng(seed)
    if layout == "offsets":
        blob, offs, bsz = rb.pack(packets, gaps=rng.integers(0, gap_max, n) + (np.arange(n) == 0) * 3, fill=CANARY)
        blob = np.concatenate([blob, np.full(16, CANARY, np.uint8)])
        kw = dict(offsets=offs, buf_sizes=bsz)
    else:
        blob = np.full(n * 4096, CANARY, np.uint8)
        offs = np.arange(n, dtype=np.uint64) * 4096
        bsz = np.array([len(p) for p in packets], np.uint32)
        for p, o in zip(packets, offs):
            blob[int(o):int(o) + len(p)] = np.frombuffer(p, np.uint8)
        kw = dict(stride=4096, count=n)
        kw.update(dict(buf_sizes=bsz) if sizes is None else dict(fixed_size=sizes))
    before = blob.copy()
    ki = np.asarray(kidx, np.uint32)
    rh = rb.req_headers(reqs) if reqs is not None else None
    if key_table is not None:
        kw["key_table"] = key_table
    if device:
        dev = lambda a, dt=None: torch.as_tensor(a if dt is None else a.astype(dt), device="cuda")  # noqa: E731
        d = dev(blob)
        kw = {k: (dev(v, np.int64) if k == "offsets" else dev(v, np.int32) if k == "buf_sizes" else v)
              for k, v in kw.items()}
        if verify:
            err = rb.verify_packed(d, keys, dev(ki, np.int32), req_hdrs=None if rh is None else dev(rh), **kw)
        else:
            err = rb.sign_packed(d, keys, dev(ki, np.int32), **kw)
        torch.cuda.synchronize()
        after, err = d.cpu().numpy(), err.cpu().numpy()
    else:
        if verify:
            err = rb.verify_packed(blob, keys, ki, req_hdrs=rh, **kw)
        else:
            err = rb.sign_packed(blob, keys, ki, **kw)
        after = blob
    return err.tolist(), rb.unpack(after, offs, bsz), before, after, offs, bsz


def gaps_intact(after, offs, bsz):
    """Every byte outside the described buffers still holds the canary."""
    inside = np.zeros(after.size, bool)
    for o, n in zip(offs, bsz):
        inside[int(o):int(o) + int(n)] = True
    return bool((after[~inside] == CANARY).all())


# ------------------------------------------------------- against the fixture
@pytest.mark.gpu
@pytest.mark.parametrize("reps", [1, 9])           # 481 and 4,329 packets: per-lane and tile keyed kernels
@pytest.mark.parametrize("layout", ["offsets", "stride"])
@pytest.mark.parametrize("device", [True, False])
def test_sign_verify_match_reference(gpu, rad, device, layout, reps):
    from liblcb_amd import radius_batch as rb
    P = rad["packets"] * reps
    kidx = [p["key"] for p in P]
    err, got, before, after, offs, bsz = run(rb, False, device, [bytes.fromhex(p["pre"]) for p in P],
                                             rad["secrets"], kidx, layout=layout, seed=reps)
    assert err == [0] * len(P)
    bad = [i for i, p in enumerate(P) if got[i].hex() != p["signed"]]
    assert not bad, (len(bad), [(P[i]["code"], P[i]["msg_authr"]) for i in bad[:10]])
    err, out, before, after, offs, bsz = run(rb, True, device, [bytes.fromhex(p["signed"]) for p in P],
                                             rad["secrets"], kidx, _reqs(P), layout=layout, seed=reps + 100)
    assert err == [0] * len(P)
    bad = [i for i, p in enumerate(P) if out[i].hex() != p["verified"]]
    assert not bad, (len(bad), [(P[i]["code"], P[i]["msg_authr"]) for i in bad[:10]])
    n = 0
    for p, o in zip(P[:481], out):
        if p["kind"] == "request" and p.get("password"):
            pw = bytes.fromhex(p["password"])
            a = _find(o, 2)
            assert o[a + 2:a + 2 + len(pw)] == pw
            n += 1
    assert n > 50
    assert gaps_intact(after, offs, bsz)          # nothing between the buffers was written


@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
def test_edge_cases_match_reference(gpu, rad, device):
    """Refused User-Passwords (EINVAL / EOVERFLOW, packet unchanged) and
    buffers longer than the packet (tail never written)."""
    from liblcb_amd import radius_batch as rb
    from liblcb_amd.radius import pkt_len
    cases = json.load(open(os.path.join(G, "radius_edge.json")))["cases"]
    pk = [bytes.fromhex(c["pre"]) for c in cases]
    err, got, _, _, _, _ = run(rb, False, device, pk, rad["secrets"], [c["key"] for c in cases])
    assert err == [c["rc"] for c in cases]
    assert {errno.EINVAL, errno.EOVERFLOW, 0} == set(err)
    for c, p, g in zip(cases, pk, got):
        if c["rc"]:
            assert g == p, c["what"]
        else:
            n = pkt_len(p)
            assert g[:n].hex() == c["signed"], c["what"]
            assert g[n:] == p[n:], c["what"]
    # the signed requests verify with their tails in place, tails unchanged
    req = [(c, g) for c, g in zip(cases, got) if c["rc"] == 0 and g[0] in (1, 4, 12, 13, 40, 43)]
    assert len(req) > 20
    err, out, _, _, _, _ = run(rb, True, device, [g for _, g in req], rad["secrets"], [c["key"] for c, _ in req])
    assert err == [0] * len(req)
    for (c, g), o in zip(req, out):
        assert o[pkt_len(g):] == g[pkt_len(g):]
    # verify refuses the User-Password lengths radius_pkt_attr_password_decode refuses: EINVAL, untouched
    bad = [p for c, p in zip(cases, pk) if c["rc"] and p[0] == 1 and _find(p, 80) is None]
    assert len(bad) >= 5
    err, out, _, _, _, _ = run(rb, True, device, bad, rad["secrets"], [0] * len(bad))
    assert err == [errno.EINVAL] * len(bad) and out == bad


@pytest.mark.gpu
def test_password_encode_vectors(gpu, rad):
    """radius_pkt_attr_password_encode (radius.h:745-790) for every password
    length 1..128 through the encode chain, and back through decode."""
    from liblcb_amd import radius_batch as rb
    pk, ki, want = [], [], []
    for v in rad["password_encode"]:
        pw = bytes.fromhex(v["password"])
        tm = (len(pw) + 15) // 16 * 16
        attr = bytes([2, 2 + tm]) + pw + bytes(tm - len(pw))
        hdr = bytes([1, 0]) + (20 + len(attr)).to_bytes(2, "big") + bytes.fromhex(v["authenticator"])
        pk.append(hdr + attr)
        ki.append(v["key"])
        want.append(v["encoded"])
    err, got, _, _, _, _ = run(rb, False, True, pk, rad["secrets"], ki)
    assert err == [0] * len(pk)
    assert [g[22:].hex() for g in got] == want
    err, back, _, _, _, _ = run(rb, True, True, got, rad["secrets"], ki, seed=5)
    assert err == [0] * len(pk) and back == pk


# ------------------------------------------- error codes from the reference
@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
def test_error_codes_match_reference(gpu, rad, device):
    """tests/golden/radius_batch.json: a case is [kind, base, flip, key, req,
    rc] over the packets of radius.json, `diffs` the byte runs the reference
    changed (tests/golden/make_golden_radius_batch.py)."""
    from liblcb_amd import radius_batch as rb
    fx = json.load(open(os.path.join(G, "radius_batch.json")))
    P, sign_kind = rad["packets"], fx["kinds"].index("sign_other")
    cases = []          # (kind, packet, key, request, rc, expected buffer)
    for n, (kind, base, flip, key, req, rc) in enumerate(fx["cases"]):
        pkt = bytearray.fromhex(P[base]["pre" if kind == sign_kind else "signed"])
        if flip >= 0:
            pkt[flip] ^= 0x40
        want = bytearray(pkt)
        for at, h in fx["diffs"].get(str(n), []):
            want[at:at + len(h) // 2] = bytes.fromhex(h)
        cases.append((kind, bytes(pkt), key, bytes.fromhex(P[req]["request"]) if req >= 0 else None, rc, bytes(want)))
    ver = [c for c in cases if c[0] != sign_kind]
    sig = [c for c in cases if c[0] == sign_kind]
    assert len(ver) >= 100 and sig and {0, errno.EBADMSG, errno.EINVAL} <= {c[4] for c in ver}
    assert {c[0] for c in cases} == set(range(len(fx["kinds"])))
    for group, verify in ((ver, True), (sig, False)):
        pk = [c[1] for c in group]
        err, out, _, _, _, _ = run(rb, verify, device, pk, rad["secrets"], [c[2] for c in group],
                                   [c[3] for c in group] if verify else None)
        bad = [(fx["kinds"][c[0]], c[4], e) for c, e in zip(group, err) if e != c[4]]
        assert not bad, (len(bad), bad[:10])
        for c, p, o in zip(group, pk, out):
            assert o == c[5], fx["kinds"][c[0]]
            if c[4]:
                assert o == p


# ---------------------------------------------------- guard and isolation
def _guard_batch(rad):
    """(packets, key indices, requests, expected sign rc, expected verify rc,
    good flags): good fixture packets mixed with structurally bad ones."""
    P = rad["packets"]
    E = errno.EBADMSG
    items = []          # (sign input, verify input, kidx, req, sign rc, verify rc)
    withattr = [p for p in P if 24 < len(p["pre"]) // 2 <= 200 and p["msg_authr"]]
    for n, p in enumerate(P[:60]):
        pre, sg = bytes.fromhex(p["pre"]), bytes.fromhex(p["signed"])
        req = bytes.fromhex(p["request"]) if p["kind"] == "reply" else None
        items.append((pre, sg, p["key"], req, 0, 0))
        q = withattr[n % len(withattr)]
        b, k = bytes.fromhex(q["signed"]), q["key"]
        rq = bytes.fromhex(q["request"]) if q["kind"] == "reply" else None
        L = len(b)
        kind = n % 9
        if kind == 0:
            m = b[:L - 1 - n % 5]                                   # truncated buffer: Length > buffer
        elif kind == 1:
            m = b[:2] + (L + 1 + n).to_bytes(2, "big") + b[4:]      # Length > buffer
        elif kind == 2:
            m = b[:2] + (n % 20).to_bytes(2, "big") + b[4:]         # Length < 20
        elif kind == 3:
            m = b[:21] + bytes([n % 2]) + b[22:]                    # attribute len 0 / 1
        elif kind == 4:
            m = b[:21] + bytes([min(255, L - 20 + 1 + n % 3)]) + b[22:]   # attribute runs past Length
        elif kind == 5:
            m = b[:n % 20]                                          # buffer shorter than a header
        elif kind == 6:
            m = b[:2] + (L - 1).to_bytes(2, "big") + b[4:]          # last attribute cut: past Length / 1 byte left
        elif kind == 7:
            m = b[:20] + bytes([0]) + b[21:]                        # attribute type 0
        else:
            m, k = b, len(rad["secrets"]) + n                        # bad key index
            items.append((m, m, k, rq, errno.EINVAL, errno.EINVAL))
            continue
        items.append((m, m, k, rq, E, E))
    # a Message-Authenticator of length 17: structurally fine, EBADMSG from both functions
    last = [q for q in withattr if _find(bytes.fromhex(q["signed"]), 80) + 18 == len(q["signed"]) // 2][:4]
    assert last
    for q in last:
        b = bytearray.fromhex(q["signed"])
        a = _find(b, 80)
        b[a + 1] = 17
        b[2:4] = (len(b) - 1).to_bytes(2, "big")
        items.append((bytes(b), bytes(b), q["key"], bytes.fromhex(q["request"]) if q["kind"] == "reply" else None,
                      E, E))
    # Length > 4096 in a buffer that holds it
    big = bytearray(5000)
    big[0], big[2:4] = 4, (4500).to_bytes(2, "big")
    items.append((bytes(big), bytes(big), 0, None, E, E))
    return items


@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
def test_guard_and_isolation(gpu, rad, device):
    """Bad packets are refused by the guard with the documented code and stay
    byte-identical, good ones are still right, nothing outside a good
    packet's [0, Length) changes, and errors is fully written."""
    from liblcb_amd import radius_batch as rb
    items = _guard_batch(rad)
    assert sum(1 for i in items if i[4] == errno.EBADMSG) >= 50
    P = rad["packets"]
    for verify in (False, True):
        pk = [i[1] if verify else i[0] for i in items]
        err, out, before, after, offs, bsz = run(rb, verify, device, pk, rad["secrets"], [i[2] for i in items],
                                      [i[3] for i in items] if verify else None, seed=9)
        assert err == [i[5] if verify else i[4] for i in items]
        good = 0
        for i, p, o in zip(items, pk, out):
            if (i[5] if verify else i[4]):
                assert o == p
            else:
                want = P[good]["verified" if verify else "signed"]
                assert o.hex() == want
                good += 1
        assert good == 60
        # canaries around and between all buffers; every changed byte lies in a good packet
        assert gaps_intact(after, offs, bsz)
        inside = np.zeros(before.size, bool)
        for i, o, n in zip(items, offs, bsz):
            if not (i[5] if verify else i[4]):
                inside[int(o):int(o) + int(n)] = True
        assert inside[np.nonzero(before != after)[0]].all()


@pytest.mark.gpu
def test_fixed_size_layout_and_single_key(gpu, rad):
    """stride / fixed_size description (no per-packet arrays) with one key
    (the keyed passes then take no key index) and trailing canary bytes."""
    from liblcb_amd import radius_batch as rb
    P = [p for p in rad["packets"] if p["key"] == 0]
    assert len(P) > 50
    pk = [bytes.fromhex(p["pre"]) for p in P]
    err, _, _, after, _, _ = run(rb, False, True, pk, rad["secrets"][:1], [0] * len(P), layout="stride", sizes=4096)
    assert err == [0] * len(P)
    for i, p in enumerate(P):
        n = len(p["signed"]) // 2
        assert bytes(after[i * 4096:i * 4096 + n]).hex() == p["signed"]
        assert (after[i * 4096 + n:(i + 1) * 4096] == CANARY).all()


# ------------------------------------------------------ cross-check at scale
@pytest.mark.gpu
def test_two_streams_agree_at_scale(gpu, rad):
    """20,000 packets sampled from the fixture, verified on the default
    stream and on a second stream back to back: same results, the fixture's."""
    import torch
    from liblcb_amd import radius_batch as rb
    P = rad["packets"]
    pick = np.random.default_rng(20).integers(0, len(P), 20000)
    signed = [bytes.fromhex(p["signed"]) for p in P]
    verified = [bytes.fromhex(p["verified"]) for p in P]
    reqs = _reqs(P)
    blob, offs, bsz = rb.pack([signed[i] for i in pick], gaps=np.random.default_rng(21).integers(0, 7, len(pick)))
    want, _, _ = rb.pack([verified[i] for i in pick], gaps=np.random.default_rng(21).integers(0, 7, len(pick)))
    dev = lambda a: torch.as_tensor(a, device="cuda")  # noqa: E731
    o, s = dev(offs.astype(np.int64)), dev(bsz.astype(np.int32))
    ki = dev(np.array([P[i]["key"] for i in pick], np.int32))
    rh = dev(rb.req_headers([reqs[i] for i in pick]))
    a, b = dev(blob), dev(blob)
    torch.cuda.synchronize()
    ea = rb.verify_packed(a, rad["secrets"], ki, o, s, req_hdrs=rh)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eb = rb.verify_packed(b, rad["secrets"], ki, o, s, req_hdrs=rh)
    torch.cuda.synchronize()
    assert not ea.cpu().numpy().any() and not eb.cpu().numpy().any()
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert np.array_equal(a.cpu().numpy(), want)


# -------------------------------------------------------- in-place restoration
@pytest.mark.gpu
def test_verify_restores_every_substituted_byte(gpu, rad):
    """Without a User-Password verify changes nothing: the whole blob, the
    failing packets included, equals its input."""
    from liblcb_amd import radius_batch as rb
    P = [p for p in rad["packets"] if not p.get("password")]
    assert len(P) > 300
    pk, reqs = [], _reqs(P)
    for n, p in enumerate(P):
        b = bytearray.fromhex(p["signed"])
        if n % 3 == 1:
            b[4 + n % 16] ^= 1                    # fails a check: still restored
        if n % 3 == 2 and p["kind"] == "reply":
            reqs[n] = None
        pk.append(bytes(b))
    err, out, before, after, offs, bsz = run(rb, True, True, pk, rad["secrets"], [p["key"] for p in P], reqs, seed=3)
    assert np.array_equal(before, after)
    assert 0 in err and errno.EBADMSG in err and errno.EINVAL in err


@pytest.mark.gpu
def test_host_mode_chunks(gpu, rad, monkeypatch):
    """Host mode across staging chunk boundaries gives the one-chunk result."""
    from liblcb_amd import radius_batch as rb
    monkeypatch.setenv("LCB_RADIUS_CHUNK_BYTES", "8192")
    P = rad["packets"]
    err, got, _, _, _, _ = run(rb, False, False, [bytes.fromhex(p["pre"]) for p in P], rad["secrets"],
                         [p["key"] for p in P])
    assert err == [0] * len(P) and [g.hex() for g in got] == [p["signed"] for p in P]


# ---------------------------------------------------------- wrapper validation
@pytest.mark.gpu
def test_wrapper_validation(gpu, rad):
    import torch
    from liblcb_amd import radius_batch as rb
    n = 8
    d = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    offs = torch.arange(n, dtype=torch.int64, device="cuda") * 64
    bsz = torch.full((n,), 64, dtype=torch.int32, device="cuda")
    ki = torch.zeros(n, dtype=torch.int32, device="cuda")
    rh = torch.zeros(n * 20, dtype=torch.uint8, device="cuda")
    K = rad["secrets"]
    bad = [dict(offsets=offs, buf_sizes=bsz.to(torch.int64)),
           dict(offsets=offs.to(torch.int32), buf_sizes=bsz),
           dict(offsets=offs[:4], buf_sizes=bsz),
           dict(offsets=offs, buf_sizes=bsz, key_index=ki.to(torch.int64)),
           dict(offsets=offs, buf_sizes=bsz, key_index=ki[:3]),
           dict(offsets=offs, buf_sizes=bsz, key_index=ki.cpu()),
           dict(offsets=offs + 1, buf_sizes=bsz),                       # runs past the blob
           dict(offsets=offs, buf_sizes=bsz, req_hdrs=rh[:20]),
           dict(offsets=offs, buf_sizes=bsz, req_hdrs=rh.cpu()),
           dict(offsets=offs, buf_sizes=bsz, req_hdrs=rh.to(torch.int32))]
    for kw in bad:
        with pytest.raises((TypeError, ValueError)):
            rb.verify_packed(d, K, **kw)
    with pytest.raises((TypeError, ValueError)):
        rb.sign_packed(d.to(torch.int32), K, offsets=offs, buf_sizes=bsz)
    with pytest.raises((TypeError, ValueError)):          # host packets with device arrays
        rb.sign_packed(np.zeros(n * 64, np.uint8), K, offsets=offs, buf_sizes=bsz)
    with pytest.raises((TypeError, ValueError)):
        rb.sign_packed(bytes(n * 64), K, count=n, stride=64, fixed_size=64)    # not writable in place
    with pytest.raises((TypeError, ValueError)):
        rb.sign_packed(np.zeros(n * 64, np.uint8), K, key_index=np.zeros(3, np.uint32), count=n, stride=64,
                       fixed_size=64)
    # zeroed 64-byte buffers: Length 0 -> EBADMSG for every packet, nothing raised, nothing written
    err = rb.verify_packed(d, K, ki, offs, bsz, req_hdrs=rh)
    torch.cuda.synchronize()
    assert err.cpu().numpy().tolist() == [errno.EBADMSG] * n and not d.cpu().numpy().any()
