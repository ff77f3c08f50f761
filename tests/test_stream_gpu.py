"""Batched streaming digests on the GPU (liblcb_amd.stream,
include/lcb_hash_stream_gpu.h).  Expected values come from the oracle
(oracle.batch over the concatenated messages, or_ctx_t driven through ctypes)
and from the reference's own contexts (tests/golden/stream.json); every
comparison is exact."""
import ctypes
import errno
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "liblcb_amd")
FX = json.load(open(os.path.join(ROOT, "tests", "golden", "stream.json")))
ALGS = list(range(1, 9))
KEY20 = bytes(range(0x40, 0x54))
E = errno.EINVAL


def blk(alg):
    return 128 if alg in (5, 6) else 64


@pytest.fixture(scope="module")
def S(gpu):
    from liblcb_amd import stream
    return stream


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


class OrCtx(ctypes.Structure):
    """or_ctx_t (oracle/lcb_oracle.h)."""
    _fields_ = [("alg", ctypes.c_int), ("used", ctypes.c_size_t), ("count", ctypes.c_uint64),
                ("count_hi", ctypes.c_uint64), ("h32", ctypes.c_uint32 * 8), ("h64", ctypes.c_uint64 * 8),
                ("gn", ctypes.c_uint64 * 8), ("gs", ctypes.c_uint64 * 8), ("buf", ctypes.c_uint8 * 128)]


def ctx_from_record(oracle, rec):
    c = OrCtx()
    alg = int(rec["alg"])
    assert oracle.lib.or_init(ctypes.byref(c), alg) == 0
    c.used, c.count, c.count_hi = int(rec["used"]), int(rec["count"]), int(rec["count_hi"])
    h = bytes(rec["h"])
    if alg <= 4:
        ctypes.memmove(c.h32, h, 32)
    else:
        ctypes.memmove(c.h64, h, 64)
    ctypes.memmove(c.gn, bytes(rec["n"]), 64)
    ctypes.memmove(c.gs, bytes(rec["sigma"]), 64)
    ctypes.memmove(c.buf, bytes(rec["buf"]), 128)
    return c


def record_from_ctx(S, c):
    r = np.zeros(1, S.STATE_DTYPE)
    alg = c.alg
    r["alg"], r["used"] = alg, c.used
    hb = {1: 16, 2: 20, 3: 32, 4: 32}.get(alg, 64)
    h = bytes(c.h32) if alg <= 4 else bytes(c.h64)
    r["h"][0, :hb] = np.frombuffer(h[:hb], np.uint8)
    r["buf"][0, :c.used] = np.frombuffer(bytes(c.buf)[:c.used], np.uint8)
    if alg >= 7:
        r["n"][0] = np.frombuffer(bytes(c.gn), np.uint8)
        r["sigma"][0] = np.frombuffer(bytes(c.gs), np.uint8)
        r["count"] = ((int.from_bytes(bytes(c.gn)[:16], "little") >> 3) + c.used) & (2 ** 64 - 1)
    else:
        r["count"], r["count_hi"] = c.count, c.count_hi
    return r


def or_update(oracle, c, data):
    oracle.lib.or_update(ctypes.byref(c), bytes(data), len(data))


def or_final(oracle, c):
    from oracle.pyoracle import DSIZE
    out = ctypes.create_string_buffer(64)
    alg = c.alg
    oracle.lib.or_final(ctypes.byref(c), out)
    return out.raw[:DSIZE[alg]]


def pack(chunks, phase=0):
    """Chunks in one blob, chunk i at a byte offset = (i + phase) mod 16 past a 16-byte boundary."""
    offs, lens, parts, pos = [], [], [], 0
    for i, c in enumerate(chunks):
        pad = (-pos) % 16 + (i + phase) % 16
        parts.append(b"\xa5" * pad)
        pos += pad
        offs.append(pos)
        lens.append(len(c))
        parts.append(bytes(c))
        pos += len(c)
    blob = np.frombuffer(b"".join(parts) + b"\xa5" * 16, np.uint8)
    return blob, np.array(offs, np.uint64), np.array(lens, np.uint32)


def dev(torch, a):
    if a.dtype == np.uint64:
        a = a.astype(np.int64)
    elif a.dtype == np.uint32:
        a = a.astype(np.int32)
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def update_dev(torch, st, chunks, index=None, phase=0):
    blob, offs, lens = pack(chunks, phase)
    st.update(dev(torch, blob), lengths=dev(torch, lens), offsets=dev(torch, offs),
              index=None if index is None else dev(torch, np.asarray(index, np.uint32)))


def digests(oracle, alg, msgs, key=None):
    blob, offs, lens = pack(msgs)
    return oracle.batch(alg, blob, offs, lens, key=key)


def rnd_bytes(seed, n):
    from oracle.pyoracle import gen_stream
    return gen_stream(0x57AE0000 + seed, n).tobytes()


# ---------------------------------------------------------------- parity
def plan_lengths(B, s, k, used):
    """Rounds 2k / 2k+1 of stream s: first a chunk that leaves `left` bytes
    over, then a chunk of the length under test."""
    combo = (3 * s + k) % 24
    left = (0, 1, B - 1)[combo % 3]
    setup = (left - used) % B + B * (s % 2)
    test = (0, 1, B - left - 1, B - left, B - left + 1, B, 2 * B + 1, 3 * B - 1)[combo // 3]
    return left, setup, test


def test_plan_covers_every_combination():
    for B in (64, 128):
        seen = set()
        for s in range(130):
            for k in range(3):
                left, _, test = plan_lengths(B, s, k, 0)
                seen.add((left, test))
        want = {(l, t) for l in (0, 1, B - 1) for t in (0, 1, B - l - 1, B - l, B - l + 1, B, 2 * B + 1, 3 * B - 1)}
        assert seen == want


@pytest.mark.parametrize("keyed", [False, True], ids=["plain", "hmac"])
@pytest.mark.parametrize("alg", ALGS)
def test_parity_six_rounds(S, torch_, oracle, alg, keyed):
    B, n = blk(alg), 130
    key = KEY20 if keyed else None
    st = S.StreamSet(alg, n, key=key)
    msgs = [b""] * n
    used = [0] * n
    for r in range(6):
        chunks = []
        for s in range(n):
            left, setup, test = plan_lengths(B, s, r // 2, used[s])
            ln = setup if r % 2 == 0 else test
            if r % 2:
                assert used[s] == left
            chunks.append(rnd_bytes(1000 * r + s, ln))
            used[s] = (used[s] + ln) % B
        update_dev(torch_, st, chunks, phase=r)
        msgs = [m + c for m, c in zip(msgs, chunks)]
        got = st.final(keep=True).cpu().numpy()
        assert np.array_equal(got, digests(oracle, alg, msgs, key)), "round %d" % r
    exp = digests(oracle, alg, msgs, key)
    assert np.array_equal(st.final().cpu().numpy(), exp)          # consumes the streams
    fresh = S.StreamSet(alg, n, key=key)
    assert st.export_states().tobytes() == fresh.export_states().tobytes()
    more = [rnd_bytes(9000 + s, (37 * s) % (2 * B + 3)) for s in range(n)]
    update_dev(torch_, st, more)
    assert np.array_equal(st.final().cpu().numpy(), digests(oracle, alg, more, key))
    st.close()
    fresh.close()


# ---------------------------------------------------------------- stream counts
@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("alg", [1, 6, 7])
def test_stream_counts(S, torch_, oracle, alg, n):
    B = blk(alg)
    with S.StreamSet(alg, n) as st:
        a = [rnd_bytes(s, (s * 29 + 5) % (3 * B)) for s in range(n)]
        b = [rnd_bytes(100 + s, (s * 53 + B - 3) % (2 * B + 7)) for s in range(n)]
        update_dev(torch_, st, a)
        update_dev(torch_, st, b, phase=5)
        assert np.array_equal(st.final().cpu().numpy(), digests(oracle, alg, [x + y for x, y in zip(a, b)]))


@pytest.mark.parametrize("alg", [1, 6, 7])
def test_long_chunk(S, torch_, oracle, alg):
    with S.StreamSet(alg, 3, key=b"k") as st:
        head = [rnd_bytes(s, s * 9 + 1) for s in range(3)]
        big = [rnd_bytes(50 + s, 65537) for s in range(3)]
        update_dev(torch_, st, head)
        update_dev(torch_, st, big, phase=3)
        exp = digests(oracle, alg, [x + y for x, y in zip(head, big)], b"k")
        assert np.array_equal(st.final().cpu().numpy(), exp)


# ---------------------------------------------------------------- index lists
@pytest.mark.parametrize("alg", [2, 5, 8])
def test_index_lists(S, torch_, oracle, alg):
    n, B = 40, blk(alg)
    st = S.StreamSet(alg, n)
    msgs = [rnd_bytes(s, s + 1) for s in range(n)]
    update_dev(torch_, st, msgs)
    rev = list(range(n - 1, -1, -1))
    ch = [rnd_bytes(200 + i, B - 1 + i % 3) for i in range(n)]
    update_dev(torch_, st, ch, index=rev)                          # chunk i goes to stream n-1-i
    for i, s in enumerate(rev):
        msgs[s] += ch[i]
    before = st.export_states()
    sub = [5, 17, 3, 39]
    ch = [rnd_bytes(300 + i, 2 * B + i) for i in range(len(sub))]
    update_dev(torch_, st, ch, index=sub)
    for i, s in enumerate(sub):
        msgs[s] += ch[i]
    after = st.export_states()
    rest = [s for s in range(n) if s not in sub]
    assert after[rest].tobytes() == before[rest].tobytes()
    assert all(after[s].tobytes() != before[s].tobytes() for s in sub)
    assert st.export_states(np.array(sub, np.uint32)).tobytes() == after[sub].tobytes()
    # final on a subset list, in the list's order; the others are untouched
    got = st.final(index=dev(torch_, np.array(sub, np.uint32)), keep=True).cpu().numpy()
    assert np.array_equal(got, digests(oracle, alg, [msgs[s] for s in sub]))
    assert st.export_states().tobytes() == after.tobytes()
    # reset on a subset
    rs = [0, 17, 38]
    st.reset(dev(torch_, np.array(rs, np.uint32)))
    for s in rs:
        msgs[s] = b""
    now = st.export_states()
    keep = [s for s in range(n) if s not in rs]
    assert now[keep].tobytes() == after[keep].tobytes()
    assert np.array_equal(st.final().cpu().numpy(), digests(oracle, alg, msgs))
    st.close()


@pytest.mark.parametrize("alg", [1, 7])
def test_index_errors(S, torch_, oracle, gpu, alg):
    n = 70
    st = S.StreamSet(alg, n)
    msgs = [rnd_bytes(s, 3 * s + 1) for s in range(n)]
    update_dev(torch_, st, msgs)
    before = st.export_states().tobytes()
    ch = [rnd_bytes(400 + i, 100) for i in range(4)]
    for bad in ([1, 2, n, 4], [1, 2, 3, 2], [69, 0, 69, 5]):
        idx = dev(torch_, np.array(bad, np.uint32))
        for call in (lambda: update_dev(torch_, st, ch, index=bad), lambda: st.final(index=idx),
                     lambda: st.final(index=idx, keep=True), lambda: st.reset(idx)):
            with pytest.raises(gpu.LcbHashError) as e:
                call()
            assert e.value.errno == E
            assert st.export_states().tobytes() == before
        # host mode refuses the same lists
        with pytest.raises(gpu.LcbHashError):
            st.final(index=np.array(bad, np.uint32))
        with pytest.raises(gpu.LcbHashError):
            st.import_states(st.export_states()[:4], index=np.array(bad, np.uint32))
        with pytest.raises(gpu.LcbHashError):
            st.export_states(np.array(bad, np.uint32))
        assert st.export_states().tobytes() == before
    ok = [1, 2, 3, 4]
    update_dev(torch_, st, ch, index=ok)                           # a following valid call still works
    for i, s in enumerate(ok):
        msgs[s] += ch[i]
    assert np.array_equal(st.final().cpu().numpy(), digests(oracle, alg, msgs))
    st.close()


def test_argument_errors_with_a_set(S, torch_, gpu):
    """Decided from the arguments alone (no HIP call): unknown flags, count
    past the set without an index, NULL data / digests / states."""
    L = S.stream_lib()
    st = S.StreamSet(gpu.MD5, 8)
    h = st._h
    d = torch_.zeros(1024, dtype=torch_.uint8, device="cuda")
    out = torch_.zeros(16 * 16, dtype=torch_.uint8, device="cuda")
    rec = np.zeros(16, S.STATE_DTYPE)
    before = st.export_states().tobytes()
    p, o, r = d.data_ptr(), out.data_ptr(), rec.ctypes.data
    for flags in (0x10, 0x4, S.F_KEEP, 0x100 | 1):
        assert L.lcb_hash_stream_update(h, None, p, None, None, 8, 64, 64, flags, None) == E
        assert L.lcb_hash_stream_reset(h, None, 8, flags, None) == E
    for flags in (0x10, 0x4, 0x8001):
        assert L.lcb_hash_stream_final(h, None, 8, o, flags, None) == E
    assert L.lcb_hash_stream_update(h, None, p, None, None, 9, 64, 64, 1, None) == E
    assert L.lcb_hash_stream_final(h, None, 9, o, 1, None) == E
    assert L.lcb_hash_stream_reset(h, None, 9, 1, None) == E
    assert L.lcb_hash_stream_export(h, None, 9, r) == E and L.lcb_hash_stream_import(h, None, 9, r) == E
    assert L.lcb_hash_stream_update(h, None, None, None, None, 8, 64, 64, 1, None) == E
    assert L.lcb_hash_stream_final(h, None, 8, None, 1, None) == E
    assert L.lcb_hash_stream_export(h, None, 8, None) == E and L.lcb_hash_stream_import(h, None, 8, None) == E
    assert L.lcb_hash_stream_update(h, None, p, None, None, 0, 64, 64, 1, None) == 0     # empty calls
    assert L.lcb_hash_stream_final(h, None, 0, None, 1, None) == 0
    assert L.lcb_hash_stream_count(h) == 8 and L.lcb_hash_stream_alg(h) == gpu.MD5
    assert st.export_states().tobytes() == before
    # import refuses records before anything changes
    good = st.export_states()
    bad = good.copy()
    bad["alg"][5] = gpu.SHA1
    with pytest.raises(gpu.LcbHashError):
        st.import_states(bad)
    bad = good.copy()
    bad["used"][7], bad["count"][7] = 64, 64
    with pytest.raises(gpu.LcbHashError):
        st.import_states(bad)
    bad = good.copy()
    bad["count"][0] = 5                                            # used stays 0
    with pytest.raises(gpu.LcbHashError):
        st.import_states(bad)
    assert st.export_states().tobytes() == before
    st.close()
    with pytest.raises(ValueError):
        st.final()


# ---------------------------------------------------------------- counters at their carries
def carry_case(S, torch_, oracle, alg, rec, data):
    """Import `rec`, absorb `data`: export and digest as an or_ctx_t given the same fields."""
    with S.StreamSet(alg, 3) as st:
        recs = np.concatenate([rec, rec, rec])
        st.import_states(recs)
        assert st.export_states().tobytes() == recs.tobytes()
        c = ctx_from_record(oracle, rec[0])
        or_update(oracle, c, data)
        update_dev(torch_, st, [data, data[:0], data], phase=7)    # stream 1 takes an empty chunk
        got = st.export_states()
        want = record_from_ctx(S, c)
        assert got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[0].tobytes()
        assert got[1].tobytes() == rec[0].tobytes()
        dig = st.final(keep=True).cpu().numpy()
        assert bytes(dig[0]) == or_final(oracle, c)
        c1 = ctx_from_record(oracle, rec[0])
        assert bytes(dig[1]) == or_final(oracle, c1)
        return got[0]


def base_record(S, torch_, alg, nbytes):
    """A real chaining value: the record after `nbytes` bytes."""
    with S.StreamSet(alg, 1) as st:
        update_dev(torch_, st, [rnd_bytes(77, nbytes)])
        return st.export_states()


@pytest.mark.parametrize("alg", [1, 2, 3, 4, 5, 6])
def test_count_carries_32(S, torch_, oracle, alg):
    B = blk(alg)
    rec = base_record(S, torch_, alg, 2 * B)
    rec["count"] = 2 ** 32 - B
    got = carry_case(S, torch_, oracle, alg, rec, rnd_bytes(1, 100))
    assert int(got["count"]) == 2 ** 32 - B + 100


@pytest.mark.parametrize("alg", [1, 2, 4, 5, 6])
def test_count_carries_61(S, torch_, oracle, alg):
    """count << 3 wraps 64 bits (MD5 / SHA-1 / SHA-256: the length field is
    modulo 2^64; SHA-384/512: bit 61 moves into the high length word)."""
    rec = base_record(S, torch_, alg, 256)
    rec["count"] = 2 ** 61 - 128
    got = carry_case(S, torch_, oracle, alg, rec, rnd_bytes(2, 200))
    assert int(got["count"]) == 2 ** 61 + 72


def test_count_carries_64_sha512(S, torch_, oracle):
    rec = base_record(S, torch_, 6, 256)
    rec["count"], rec["count_hi"] = 2 ** 64 - 128, 0
    got = carry_case(S, torch_, oracle, 6, rec, rnd_bytes(3, 200))
    assert int(got["count"]) == 72 and int(got["count_hi"]) == 1


@pytest.mark.parametrize("alg", [7, 8])
def test_gost_counter_and_sigma_carries(S, torch_, oracle, alg):
    rec = base_record(S, torch_, alg, 64 + 9)
    rec["n"][0, :8] = np.frombuffer((2 ** 64 - 512).to_bytes(8, "little"), np.uint8)
    rec["sigma"][0, :32] = 0xFF
    rec["count"] = ((2 ** 64 - 512) >> 3) + 9
    got = carry_case(S, torch_, oracle, alg, rec, rnd_bytes(4, 200))
    assert int.from_bytes(bytes(got["n"]), "little") == 2 ** 64 - 512 + 3 * 512   # the carry left the low word
    assert int(got["used"]) == (9 + 200) % 64


# ---------------------------------------------------------------- pinned to the reference
@pytest.mark.parametrize("case", FX["cases"], ids=[c["name"] for c in FX["cases"]])
def test_reference_records(S, torch_, case):
    from oracle.pyoracle import gen_stream
    alg = case["alg"]
    key = bytes.fromhex(case["key"]) if case["key"] is not None else None
    msg = gen_stream(FX["seed"], case["length"]).tobytes()
    pre = [r["prefix"] for r in case["records"]]
    want = np.frombuffer(b"".join(bytes.fromhex(r["record"]) for r in case["records"]), S.STATE_DTYPE)
    with S.StreamSet(alg, len(pre), key=key) as st:
        update_dev(torch_, st, [msg[:n] for n in pre])
        got = st.export_states()
        for g, w, n in zip(got, want, pre):
            assert g.tobytes() == w.tobytes(), (case["name"], n)
    with S.StreamSet(alg, len(pre), key=key) as st:
        st.import_states(want)
        update_dev(torch_, st, [msg[n:] for n in pre], phase=9)
        got = st.final().cpu().numpy()
        assert [bytes(d).hex() for d in got] == [case["digest"]] * len(pre)


@pytest.mark.parametrize("alg", [1, 6])
def test_hmac_key_lengths(S, torch_, oracle, alg):
    B = blk(alg)
    for kl in (0, 1, B - 1, B, B + 1, 3 * B + 5):
        key = rnd_bytes(500 + kl, kl)
        with S.StreamSet(alg, 4, key=key) as st:
            a = [rnd_bytes(s, 10 * s) for s in range(4)]
            b = [rnd_bytes(10 + s, B + s) for s in range(4)]
            update_dev(torch_, st, a)
            update_dev(torch_, st, b)
            exp = digests(oracle, alg, [x + y for x, y in zip(a, b)], key)
            assert np.array_equal(st.final().cpu().numpy(), exp), kl


# ---------------------------------------------------------------- host mode, C caller
@pytest.mark.parametrize("alg", ALGS)
def test_host_mode_matches_device_mode(S, torch_, oracle, alg, monkeypatch):
    monkeypatch.setenv("LCB_HASH_STREAM_CHUNK_BYTES", "4096")     # several staging chunks per call
    n, B = 65, blk(alg)
    hs, ds = S.StreamSet(alg, n, key=b"host"), S.StreamSet(alg, n, key=b"host")
    msgs = [b""] * n
    for r in range(3):
        ch = [rnd_bytes(600 + 100 * r + s, (s * (r + 3) * 11) % (3 * B + 2)) for s in range(n)]
        blob, offs, lens = pack(ch, phase=r)
        if r == 1:       # an index list too
            idx = np.arange(n - 1, -1, -1).astype(np.uint32)
            hs.update(blob, lengths=lens, offsets=offs, index=idx)
            update_dev(torch_, ds, ch, index=idx, phase=r)
            for i, s in enumerate(idx):
                msgs[s] += ch[i]
        else:
            hs.update(blob, lengths=lens, offsets=offs)
            update_dev(torch_, ds, ch, phase=r)
            msgs = [m + c for m, c in zip(msgs, ch)]
        assert hs.export_states().tobytes() == ds.export_states().tobytes()
    exp = digests(oracle, alg, msgs, b"host")
    got = hs.final_host(keep=True)
    assert isinstance(got, np.ndarray) and np.array_equal(got, exp)
    sub = np.array([64, 0, 33], np.uint32)
    assert np.array_equal(hs.final(index=sub), exp[sub])           # numpy index: host mode, consumed
    hs.reset(np.array([1], np.uint32))
    fresh = S.StreamSet(alg, 1, key=b"host").export_states()
    now = hs.export_states()
    assert all(now[s].tobytes() == fresh[0].tobytes() for s in (64, 0, 33, 1))
    assert np.array_equal(ds.final().cpu().numpy(), exp)
    hs.close()
    ds.close()


@pytest.mark.parametrize("alg,key", [(1, "-"), (6, "secret"), (7, "-"), (8, "radius-shared-secret")])
def test_c_caller_drives_the_abi(gpu, oracle, tmp_path, alg, key):
    exe = str(tmp_path / "stream_caller")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "stream_caller.c"), "-o", exe,
                           "-L" + LIBDIR, "-llcb_hash_stream_gpu", "-llcb_hash_gpu", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath-link," + LIBDIR + ":/opt/rocm/lib"])
    n = 9
    out = subprocess.check_output([exe, str(alg), str(n), key], timeout=120).decode().split()
    i = np.arange(200 * n + 512, dtype=np.uint64)
    pat = ((i * 131 + (i >> 8) * 7 + 5) & 255).astype(np.uint8)
    offs = np.arange(n, dtype=np.uint64) * 200
    lens = (37 + np.arange(n) + 64 + 2 * np.arange(n)).astype(np.uint32)
    exp = oracle.batch(alg, pat, offs, lens, key=None if key == "-" else key.encode())
    assert out == [bytes(d).hex() for d in exp]
