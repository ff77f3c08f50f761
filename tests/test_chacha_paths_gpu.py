"""Oracle parity for every wave-uniform dispatch fork of chacha_lane_kernel
(liblcb_amd/csrc/chacha_kernels.hip) and of chacha_host
(liblcb_amd/csrc/lcb_chacha_gpu.cpp): the coalesced stream path in all four
round instantiations (prefetching DR 4/6, DR 10, generic), its partial last
tile, fixed-length batches on both sides of bpb = 64, the fixed-bpb-through-
offsets and lengths-with-stride modes, the ragged block prefix with a scan
carry and a four-level wave search, and host mode across chunk boundaries.

Every case is bit-exact against oracle.pyoracle.Oracle.chacha_batch over the
WHOLE destination: per-buffer counters (some with the low word at 0xfffffff0
or above, so the carry into word 13 happens inside a buffer), per-buffer ivs,
a sentinel-filled destination (bytes outside the described buffers must stay
untouched) and, for dense batches, a destination that is a view into a tensor
64 B longer at each end whose slack must still be zero."""
import functools

import numpy as np
import pytest
import torch

from oracle.pyoracle import Oracle
from tests.test_chacha_gpu import expected_with_sentinel, gapped_layout, run_dev

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
SLACK = 64


@functools.lru_cache(maxsize=None)
def _orc():
    return Oracle()


def _key(rng):
    return rng.integers(0, 256, 32, dtype=np.uint8).tobytes()


def _ksz(x, *parts):
    """One key size per combination: xchacha always 32, plain alternates."""
    return 32 if x or sum(parts) % 2 == 0 else 16


def make_counters(rng, count, carry_at=None):
    """Random 64-bit counters; buffer 0, every 5th buffer and those in
    `carry_at` start 0..15 blocks below a low-word wrap (low word 0xfffffff0
    .. 0xffffffff), so multi-block buffers carry into word 13 mid-buffer."""
    c = rng.integers(0, 256, (count, 8), dtype=np.uint8)
    idx = np.arange(0, count, 5)
    if carry_at is not None:
        idx = np.union1d(idx, np.asarray(carry_at, np.int64))
    c[idx, 0] = 0xff - (idx % 16).astype(np.uint8)
    c[idx, 1:4] = 0xff
    return c.reshape(-1)


def make_ivs(rng, count, x):
    return rng.integers(0, 256, (24 if x else 8) * count, dtype=np.uint8)


def buffer_mask(total, offs, lens):
    """True at every byte some (non-overlapping) buffer describes."""
    d = np.zeros(total + 1, np.int32)
    np.add.at(d, offs.astype(np.int64), 1)
    np.add.at(d, offs.astype(np.int64) + lens.astype(np.int64), -1)
    return np.cumsum(d[:total]) > 0


def assert_same(got, exp, what):
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got != exp)
        raise AssertionError("%s: %d of %d bytes differ, first at byte %d (block %d)"
                             % (what, bad.size, exp.size, bad[0], bad[0] // 64))


# ------------------------------------------------------------ 1. stream path
STREAM_SHAPES = [
    pytest.param(1, 64, id="1x64-one-block-no-full-tile"),
    pytest.param(63, 64, id="63x64-one-partial-tile"),
    pytest.param(64, 64, id="64x64-exactly-one-tile"),
    pytest.param(65, 64, id="65x64-one-tile-plus-1-block"),
    pytest.param(100, 192, id="100x192-bpb3-4-tiles-plus-44"),
    pytest.param(1000, 1024, id="1000x1024-250-tiles-grid-stride"),
    pytest.param(37, 4096, id="37x4096-bpb64-branch-boundary"),
    pytest.param(21, 8256, id="21x8256-bpb129-42-tiles-plus-21"),
    pytest.param(3, 65536, id="3x65536-bpb1024-tiles-inside-buffer"),
]
ROUNDS_IDS = {8: "r8-DR4-prefetch", 12: "r12-DR6-prefetch", 20: "r20-DR10", 6: "r6-generic", 0: "r0-generic"}


@functools.lru_cache(maxsize=None)
def dense_case(count, flen, x, rounds):
    """Inputs and both oracle outputs (encrypt, keystream) of one dense batch."""
    rng = np.random.default_rng([count, flen, int(x), rounds])
    n = count * flen
    ksz = _ksz(x, count, flen // 64, rounds // 2)
    key = _key(rng)
    src = rng.integers(0, 256, n, dtype=np.uint8)
    counters = make_counters(rng, count)
    ivs = make_ivs(rng, count, x)
    kw = dict(count=count, stride=flen, fixed_len=flen, counters=counters, ivs=ivs, x=x)
    enc = _orc().chacha_batch(key, ksz, rounds, src, **kw)[:n]
    ks = _orc().chacha_batch(key, ksz, rounds, None, nbytes=n, **kw)[:n]
    for a in (src, counters, ivs, enc, ks):
        a.setflags(write=False)
    return key, ksz, src, counters, ivs, enc, ks


def run_dense(count, flen, x, rounds, mode, shift=0):
    """One dense batch on the device -> (got, expected).  dst (and src when
    in place) is a view at byte SLACK + shift of a zeroed tensor with SLACK
    more bytes behind it; shift = 0 keeps the 16-B alignment of the stream
    path, out-of-place src is shifted alike."""
    from liblcb_amd.chacha import chacha_batch, xchacha_batch
    key, ksz, src, counters, ivs, enc, ks = dense_case(count, flen, x, rounds)
    n = count * flen
    lo = SLACK + shift
    full = torch.zeros(lo + n + SLACK, dtype=torch.uint8, device="cuda")
    view = full[lo:lo + n]
    assert view.data_ptr() % 16 == shift % 16
    s = None
    if mode == "inplace":
        view.copy_(torch.from_numpy(src.copy()))
        s = view
    else:
        view.fill_(SENTINEL)
        if mode == "encrypt":
            s = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")[shift:shift + n]
            s.copy_(torch.from_numpy(src.copy()))
    fn = xchacha_batch if x else chacha_batch
    out = fn(key, s, dst=view, key_size=ksz, rounds=rounds,
             counters=torch.from_numpy(counters.copy()).cuda(), ivs=torch.from_numpy(ivs.copy()).cuda(),
             count=count, stride=flen, fixed_len=flen)
    torch.cuda.synchronize()
    assert out.data_ptr() == view.data_ptr()
    got = full.cpu().numpy()
    assert not got[:lo].any() and not got[lo + n:].any(), "slack bytes around dst written"
    if s is not None and mode == "encrypt":
        assert np.array_equal(s.cpu().numpy(), src), "src modified"
    return got[lo:lo + n], (ks if mode == "keystream" else enc)


@pytest.mark.parametrize("mode", ["encrypt", "inplace", "keystream"])
@pytest.mark.parametrize("rounds", [8, 12, 20, 6, 0], ids=lambda r: ROUNDS_IDS[r])
@pytest.mark.parametrize("x", [False, True], ids=["chacha", "xchacha"])
@pytest.mark.parametrize("count,flen", STREAM_SHAPES)
def test_stream_path(gpu, count, flen, x, rounds, mode):
    """a.stream: dense, stride == fixed_len, whole blocks, 16-B aligned (the
    bench layout).  Full tiles take the LDS-redistributed coalesced path, the
    partial last tile falls to `fast`."""
    got, exp = run_dense(count, flen, x, rounds, mode)
    assert_same(got, exp, "stream %dx%d x=%d rounds=%d %s" % (count, flen, x, rounds, mode))


# ------------------------------------------- 2. fixed length, off the stream
FIXED_SHAPES = [
    pytest.param(40, 4224, 4160, id="40x4160-stride4224-fast-bpb65"),
    pytest.param(50, 4100, 4100, id="50x4100-misaligned-slice-bpb65"),
    pytest.param(500, 464, 448, id="500x448-stride464-fast-bpb7"),
    pytest.param(300, 208, 200, id="300x200-stride208-bpb4-partial-last-block"),
    pytest.param(9, 70000, 69999, id="9x69999-stride70000-misaligned-bpb1094"),
]


def check_described(x, rounds, src, offs, lens, total, keystream, seed, **layout):
    """Device run of one batch described by `layout` (what the library gets)
    against the oracle; offs/lens say where its buffers lie."""
    rng = np.random.default_rng(seed)
    count = len(offs)
    key = _key(rng)
    ksz = _ksz(x, count, rounds // 2)
    counters = make_counters(rng, count)
    ivs = make_ivs(rng, count, x)
    sentinel = np.full(total, SENTINEL, np.uint8)
    s = None if keystream else src
    full = _orc().chacha_batch(key, ksz, rounds, s, counters=counters, ivs=ivs, x=x, nbytes=total, **layout)
    exp = expected_with_sentinel(full, offs, lens, sentinel)
    got = run_dev(x, key, ksz, rounds, s, layout.get("offsets"), layout.get("lengths"), counters=counters,
                  ivs=ivs, count=layout.get("count"), stride=layout.get("stride") or None,
                  fixed_len=layout.get("fixed_len") or None, dst_init=sentinel)
    assert_same(got, exp, "x=%d rounds=%d keystream=%d %r" % (x, rounds, keystream, sorted(layout)))


@pytest.mark.parametrize("keystream", [False, True], ids=["encrypt", "keystream"])
@pytest.mark.parametrize("rounds", [20, 8], ids=lambda r: ROUNDS_IDS[r])
@pytest.mark.parametrize("x", [False, True], ids=["chacha", "xchacha"])
@pytest.mark.parametrize("count,stride,flen", FIXED_SHAPES)
def test_fixed_len_off_stream(gpu, count, stride, flen, x, rounds, keystream):
    """Fixed-length batches that are not one dense run of whole blocks: the
    jb0 + lane branch (bpb >= 64, one wrap into the next buffer) and the
    divide-per-lane branch (bpb < 64), through `fast` and the slice paths."""
    total = count * stride
    src = np.random.default_rng([count, stride]).integers(0, 256, total, dtype=np.uint8)
    offs = np.arange(count, dtype=np.uint64) * np.uint64(stride)
    lens = np.full(count, flen, np.uint32)
    check_described(x, rounds, src, offs, lens, total, keystream, [count, flen, int(x), rounds],
                    count=count, stride=stride, fixed_len=flen)


@pytest.mark.parametrize("mode", ["encrypt", "inplace", "keystream"])
@pytest.mark.parametrize("rounds", [20, 8], ids=lambda r: ROUNDS_IDS[r])
@pytest.mark.parametrize("x", [False, True], ids=["chacha", "xchacha"])
def test_dense_base_off_by_4_not_stream(gpu, x, rounds, mode):
    """Dense whole blocks whose base pointers sit 4 B off a 16-B boundary:
    a.stream == 0, every block goes through the dword-slot slice path."""
    got, exp = run_dense(100, 192, x, rounds, mode, shift=4)
    assert_same(got, exp, "dense+4 x=%d rounds=%d %s" % (x, rounds, mode))


@pytest.mark.parametrize("keystream", [False, True], ids=["encrypt", "keystream"])
@pytest.mark.parametrize("rounds", [20, 8], ids=lambda r: ROUNDS_IDS[r])
@pytest.mark.parametrize("x", [False, True], ids=["chacha", "xchacha"])
def test_offsets_with_fixed_len(gpu, x, rounds, keystream):
    """`offsets` + fixed_len = 200 and no `lengths`: fixed bpb = 4 located
    through the offsets array (misaligned, gapped)."""
    rng = np.random.default_rng(21)
    n = 300
    offs, _, _ = gapped_layout(rng, n, 64)
    offs = offs + np.arange(n, dtype=np.uint64) * np.uint64(200)  # spaced >= 200 B apart
    total = int(offs[-1]) + 200 + 64
    src = rng.integers(0, 256, total, dtype=np.uint8)
    check_described(x, rounds, src, offs, np.full(n, 200, np.uint32), total, keystream, [22, int(x), rounds],
                    offsets=offs, count=n, fixed_len=200)


@pytest.mark.parametrize("keystream", [False, True], ids=["encrypt", "keystream"])
@pytest.mark.parametrize("rounds", [20, 8], ids=lambda r: ROUNDS_IDS[r])
@pytest.mark.parametrize("x", [False, True], ids=["chacha", "xchacha"])
def test_lengths_with_stride(gpu, x, rounds, keystream):
    """`lengths` (0..256) + stride = 256 and no `offsets`: the ragged block
    prefix with buffers located by i * stride."""
    rng = np.random.default_rng(23)
    n = 300
    lens = rng.integers(0, 257, n).astype(np.uint32)
    lens[:4] = [0, 256, 255, 1]
    offs = np.arange(n, dtype=np.uint64) * np.uint64(256)
    total = n * 256
    src = rng.integers(0, 256, total, dtype=np.uint8)
    check_described(x, rounds, src, offs, lens, total, keystream, [24, int(x), rounds],
                    lengths=lens, count=n, stride=256)


# ------------------------------------------ 3. ragged prefix and its searches
RAGGED_COUNTS = [
    pytest.param(1, id="1-buffer"),
    pytest.param(64, id="64-one-search-level"),
    pytest.param(1024, id="1024-one-scan-workgroup"),
    pytest.param(1025, id="1025-two-scan-workgroups"),
    pytest.param(4097, id="4097-three-search-levels"),
    pytest.param(270001, id="270001-scan-carry-four-search-levels"),
]
BIG = 270001  # > 256 x 1024 = 64^3: second chacha_scan_parts pass, 4 cha_wave_search levels


@functools.lru_cache(maxsize=None)
def ragged_layout(count):
    """Lengths 0..199 at byte offsets with gaps 0..4; where the count allows
    (>= 4 x the run) runs of empty buffers at the start (3000), in the middle
    (5000) and at the end (2000) for the lane gallop; six buffers spread over
    the batch are 70,000 B so tiles begin in the middle of a buffer."""
    rng = np.random.default_rng([3, count])
    lens = rng.integers(0, 200, count).astype(np.int64)
    for first, n in ((0, 3000), (count // 2 - 2500, 5000), (count - 2000, 2000)):
        if count >= 4 * n:
            lens[first:first + n] = 0
    big = np.unique((2 * np.arange(6) + 1) * count // 12)
    lens[big] = 70000
    gaps = rng.integers(0, 5, count).astype(np.int64)
    ends = np.cumsum(gaps + lens)
    offs = (ends - lens + int(rng.integers(0, 16))).astype(np.uint64)
    total = int(offs[-1]) + int(lens[-1]) + 64
    src = rng.integers(0, 256, total, dtype=np.uint8)
    lens = lens.astype(np.uint32)
    mask = buffer_mask(total, offs, lens)
    mask.setflags(write=False)
    return offs, lens, total, src, big, mask


@functools.lru_cache(maxsize=None)
def ragged_case(count, x, rounds, keystream=False):
    """Key material and the oracle's output for ragged_layout(count)."""
    offs, lens, total, src, big, mask = ragged_layout(count)
    rng = np.random.default_rng([4, count, int(x), rounds])
    key = _key(rng)
    ksz = _ksz(x, count, rounds // 2)
    counters = make_counters(rng, count, carry_at=big)
    ivs = make_ivs(rng, count, x)
    full = _orc().chacha_batch(key, ksz, rounds, None if keystream else src, offs, lens, counters=counters,
                               ivs=ivs, x=x, nbytes=total)
    full.setflags(write=False)
    return key, ksz, counters, ivs, full


def check_ragged_dev(count, x, rounds, keystream):
    offs, lens, total, src, _, mask = ragged_layout(count)
    key, ksz, counters, ivs, full = ragged_case(count, x, rounds, keystream)
    sentinel = np.full(total, SENTINEL, np.uint8)
    got = run_dev(x, key, ksz, rounds, None if keystream else src, offs, lens, counters=counters, ivs=ivs,
                  dst_init=sentinel)
    assert_same(got, np.where(mask, full, sentinel), "ragged count=%d x=%d rounds=%d keystream=%d"
                % (count, x, rounds, keystream))


@pytest.mark.parametrize("rounds", [20, 8], ids=lambda r: ROUNDS_IDS[r])
@pytest.mark.parametrize("x", [False, True], ids=["chacha", "xchacha"])
@pytest.mark.parametrize("count", RAGGED_COUNTS)
def test_ragged_prefix_encrypt(gpu, count, x, rounds):
    """chacha_scan_* (one, two and > 256 workgroups: the parts carry),
    cha_wave_search (1..4 levels), cha_lane_search over long empty runs and
    tiles that begin in the middle of a 70,000-B buffer."""
    check_ragged_dev(count, x, rounds, False)


def test_ragged_prefix_keystream_scan_carry(gpu):
    check_ragged_dev(BIG, False, 20, True)


def test_ragged_all_empty(gpu):
    """5,000 empty buffers: total_blocks == 0, nothing written, no error."""
    n = 5000
    offs = np.arange(n, dtype=np.uint64) * np.uint64(3)
    lens = np.zeros(n, np.uint32)
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, 3 * n + 64, dtype=np.uint8)
    sentinel = np.full(src.size, SENTINEL, np.uint8)
    for x in (False, True):
        got = run_dev(x, _key(rng), 32, 20, src, offs, lens, counters=make_counters(rng, n),
                      ivs=make_ivs(rng, n, x), dst_init=sentinel)
        assert (got == SENTINEL).all(), x


# ------------------------------------------------ 4. host mode across chunks
def _host_fn(x):
    from liblcb_amd.chacha import chacha_batch, xchacha_batch
    return xchacha_batch if x else chacha_batch


@pytest.mark.parametrize("x", [False, True], ids=["chacha", "xchacha"])
def test_host_ragged_two_chunks_by_buffer_cap(gpu, x):
    """(a) 270,001 ragged buffers from pageable memory: kChaChunkMsgs = 2^18
    buffers per chunk, so chunk 2 holds the last 7,857 (pend_first, counters
    + i * 8, ivs + i * ivl indexing); out of place and in place."""
    offs, lens, total, src, _, mask = ragged_layout(BIG)
    key, ksz, counters, ivs, full = ragged_case(BIG, x, 20, False)
    sentinel = np.full(total, SENTINEL, np.uint8)
    dst = sentinel.copy()
    kw = dict(key_size=ksz, rounds=20, counters=counters, ivs=ivs, offsets=offs, lengths=lens)
    _host_fn(x)(key, src, dst=dst, **kw)
    assert_same(dst, np.where(mask, full, sentinel), "host chunk 2 out of place x=%d" % x)
    buf = src.copy()
    _host_fn(x)(key, buf, dst=buf, **kw)
    assert_same(buf, np.where(mask, full, src), "host chunk 2 in place x=%d" % x)


def test_host_strided_two_chunks_by_byte_cap(gpu):
    """(b) 80 buffers of 1 MiB + 17 at stride 1 MiB + 32 (not dense): 63 fit
    kChaChunkBytes = 64 MiB, the last 17 make chunk 2."""
    n, stride, flen = 80, (1 << 20) + 32, (1 << 20) + 17
    rng = np.random.default_rng(41)
    total = n * stride
    src = rng.integers(0, 256, total, dtype=np.uint8)
    key = _key(rng)
    counters = make_counters(rng, n)
    ivs = make_ivs(rng, n, False)
    full = _orc().chacha_batch(key, 32, 20, src, count=n, stride=stride, fixed_len=flen, counters=counters,
                               ivs=ivs)
    offs = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    mask = buffer_mask(total, offs, np.full(n, flen, np.uint32))
    dst = np.full(total, SENTINEL, np.uint8)
    _host_fn(False)(key, src, dst=dst, rounds=20, counters=counters, ivs=ivs, count=n, stride=stride,
                    fixed_len=flen)
    assert_same(dst, np.where(mask, full, np.uint8(SENTINEL)), "host byte-cap chunk 2")


@pytest.fixture(scope="module")
def dense_host():
    """Dense 80 x 1 MiB: 64 buffers fill kChaChunkBytes = 64 MiB, 16 more
    make chunk 2.  Shared by the page-locked and pageable tests."""
    n, flen = 80, 1 << 20
    rng = np.random.default_rng(43)
    src = rng.integers(0, 256, n * flen, dtype=np.uint8)
    key = _key(rng)
    counters = make_counters(rng, n)
    ivs = make_ivs(rng, n, False)
    kw = dict(count=n, stride=flen, fixed_len=flen, counters=counters, ivs=ivs)
    enc = _orc().chacha_batch(key, 32, 20, src, **kw)
    ks = _orc().chacha_batch(key, 32, 20, None, nbytes=n * flen, **kw)
    for a in (src, enc, ks):
        a.setflags(write=False)
    return key, kw, src, enc, ks


def _pinned(n, fill=None):
    a = torch.empty(n, dtype=torch.uint8).pin_memory().numpy()
    if fill is not None:
        a[:] = fill
    return a


def test_host_dense_pinned_direct_two_chunks(gpu, dense_host):
    """(c) page-locked src and dst: the `direct` path DMAs src + i * stride
    and dst + i * stride of chunk 2 without staging."""
    key, kw, src, enc, _ = dense_host
    dst = _pinned(src.size, SENTINEL)
    _host_fn(False)(key, _pinned(src.size, src), dst=dst, rounds=20, **kw)
    assert_same(dst, enc, "host direct chunk 2")


def test_host_dense_pageable_two_chunks(gpu, dense_host):
    """(d) the same dense batch from pageable memory (staged, dense kernel)."""
    key, kw, src, enc, _ = dense_host
    dst = np.full(src.size, SENTINEL, np.uint8)
    _host_fn(False)(key, src, dst=dst, rounds=20, **kw)
    assert_same(dst, enc, "host dense pageable chunk 2")


def test_host_dense_pinned_keystream_two_chunks(gpu, dense_host):
    """(e) keystream only (src None) into page-locked dst: `direct` without
    an upload."""
    key, kw, src, _, ks = dense_host
    dst = _pinned(src.size, SENTINEL)
    _host_fn(False)(key, None, dst=dst, rounds=20, **kw)
    assert_same(dst, ks, "host direct keystream chunk 2")
