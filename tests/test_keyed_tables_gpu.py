"""Key-table geometry and block-boundary sweeps for keyed batches
(lcb_hash_batch_keyed): every check is bit-exact on the full digest array
against the oracle (oracle.batch_keyed), which receives the same key table.

  a  boundary sweep   key lengths around B-9 / B-8 / B / 2B / 3B twice each,
                      long keys at all four dword phases of the packed blob,
                      every message length 0..2B+1 for every key (every residue
                      of (len + klen) % B), below and above the bucketing
                      threshold, device and host mode
  b  long messages    4 KiB .. 70 KB records in the per-lane keyed kernels and
                      as the top length classes of a bucketed batch
  c  table size       1 .. 1000 keys: one, several, full and partial blocks of
                      the key-prep kernels, every key index used
  d  caller geometry  key_table=(blob, offsets, lengths): gaps, shuffled
                      order, overlap, identical ranges, offsets None
  e  cache identity   same bytes split differently, one table in every mode,
                      one key as an HMAC key and as a one-key table
  f  cross-stream     a table used on a second stream while the stream that
                      prepares it is still busy

B is the hash's block: 64 bytes, 128 for SHA-384/512.  The inputs' own
properties (phase coverage, counts on either side of the threshold) are
asserted on the CPU (test_sweep_inputs_cover_what_they_claim).
"""
import numpy as np
import pytest

from oracle.pyoracle import gen_stream

BLOCK = {1: 64, 2: 64, 3: 64, 4: 64, 5: 128, 6: 128, 7: 64, 8: 64}
BUCKET_MIN, BUCKET_SMALL_MAX = 4096, 16384     # kBucketMinCount, kPfMaxCount (lcb_internal.hpp, md_kernels.hpp)
MODES = (1, 2, 3)                              # KEY_HMAC, KEY_PREFIX, KEY_SUFFIX


def _dev(a, dt=None):
    import torch
    return torch.as_tensor(a if dt is None else a.astype(dt), device="cuda")


def _run_dev(gpu, alg, mode, keys, d, offs, lens, kidx, **kw):
    """Device-mode keyed batch of host arrays; d: the data already on the device."""
    got = gpu.hash_batch_keyed(alg, mode, keys, d, key_index=None if kidx is None else _dev(kidx, np.int32),
                               offsets=_dev(offs, np.int64), lengths=_dev(lens, np.int32), **kw)
    return got.cpu().numpy()


def _place(lens, seed, count_from=0):
    """Starts at 16 * ceil + (i * 7) % 16 (every byte phase mod 16); with
    count_from, the messages of at least that many bytes are counted on their
    own, so that they too step through every phase -> (data, offsets)."""
    offs = np.zeros(len(lens), np.uint64)
    pos = i = 0
    for m, n in enumerate(lens):
        offs[m] = (pos + 15) // 16 * 16 + ((i if count_from and n >= count_from else m) * 7) % 16
        pos = int(offs[m]) + int(n)
        i += n >= count_from
    return gen_stream(seed, pos + 16), offs


# ------------------------------------------------------------ a. boundary sweep
def sweep_key_lengths(B):
    return [0, 1, 3, B - 9, B - 8, B - 1, B, B + 1, 2 * B - 9, 2 * B - 8, 2 * B, 2 * B + 1, 3 * B + 5]


def sweep_table(B):
    """(keys, real): the 13 lengths twice, a 1..4-byte filler key ahead of
    every key of B bytes or more so that the j-th such length starts at dword
    phase j % 4 in its first copy and (j + 2) % 4 in its second (the library
    packs the keys back to back in table order); real = the non-filler
    indices."""
    rng = np.random.default_rng(1000 + B)
    keys, real, pos = [], [], 0
    for rep in range(2):
        j = 0
        for n in sweep_key_lengths(B):
            if n >= B:
                fill = ((j + 2 * rep) - pos) % 4 or 4
                keys.append(rng.integers(0, 256, fill, dtype=np.uint8).tobytes())
                pos += fill
                j += 1
            real.append(len(keys))
            keys.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
            pos += n
    return keys, real


def long_key_phases(keys, at_least):
    """Dword phases, in the packed blob, of the keys of `at_least` bytes or more."""
    klen = np.array([len(k) for k in keys], np.uint64)
    koff = np.cumsum(klen) - klen
    return {int(o) % 4 for o, n in zip(koff, klen) if n >= at_least}


_SWEEP = {}


def sweep_inputs(B):
    """(keys, data, offsets, lengths, key_index) of block size B, built once."""
    if B not in _SWEEP:
        keys, real = sweep_table(B)
        lens = np.tile(np.arange(2 * B + 2, dtype=np.uint32), len(real))
        kidx = np.repeat(np.array(real, np.uint32), 2 * B + 2)
        data, offs = _place(lens, 0xB0 + B)
        _SWEEP[B] = (keys, data, offs, lens, kidx)
    return _SWEEP[B]


def sweep_chunks(n):
    """[lo, hi) ranges that split n messages evenly into as few calls as stay
    below the bucketing threshold: one call of 3,380 for B = 64, two of 3,354
    for B = 128."""
    parts = -(-n // (BUCKET_MIN - 1))
    per = -(-n // parts)
    return [(lo, min(n, lo + per)) for lo in range(0, n, per)]


def sweep_replica(n, B):
    """Message indices of the replicated, shuffled batch (3x for B = 64, 2x for B = 128)."""
    idx = np.tile(np.arange(n), 3 if B == 64 else 2)
    return idx[np.random.default_rng(B).permutation(idx.size)]


_REF = {}


def sweep_expected(oracle, alg, mode):
    """The oracle's digests of the sweep, computed once per (alg, mode) and
    shared by the device and host tests."""
    if (alg, mode) not in _REF:
        keys, data, offs, lens, kidx = sweep_inputs(BLOCK[alg])
        exp = oracle.batch_keyed(alg, mode, keys, data, kidx, offs, lens)
        exp.setflags(write=False)
        _REF[(alg, mode)] = exp
    return _REF[(alg, mode)]


@pytest.mark.parametrize("B", [64, 128])
def test_sweep_inputs_cover_what_they_claim(B):
    """CPU: conditions on the sweep's inputs.  Taken together the keys of B
    bytes or more start at all four dword phases of the packed blob (so do
    the keys longer than a block, which HMAC hashes first), every non-filler
    key meets every message length 0..2B+1 (every residue of (len + klen) % B),
    every start phase mod 16 occurs, and the two batch sizes lie on either side of the
    bucketing threshold."""
    keys, real = sweep_table(B)
    want = sweep_key_lengths(B)
    assert sorted(len(keys[k]) for k in real) == sorted(want * 2) and len(real) == 26
    assert all(1 <= len(k) <= 4 for i, k in enumerate(keys) if i not in real)
    assert long_key_phases(keys, B) == {0, 1, 2, 3}
    assert long_key_phases(keys, B + 1) == {0, 1, 2, 3}
    assert long_key_phases(keys, 2 * B) == {0, 1, 2, 3}
    _, data, offs, lens, kidx = sweep_inputs(B)
    assert len(lens) == 26 * (2 * B + 2)
    for k in real:
        mine = lens[kidx == k]
        assert sorted(mine.tolist()) == list(range(2 * B + 2))
        assert {(int(n) + len(keys[k])) % B for n in mine} == set(range(B))
    assert {int(o) % 16 for o in offs} == set(range(16))
    assert int((offs + lens).max()) <= data.size
    chunks = sweep_chunks(len(lens))
    assert len(chunks) == (1 if B == 64 else 2) and chunks[0][0] == 0 and chunks[-1][1] == len(lens)
    assert all(0 < hi - lo < BUCKET_MIN for lo, hi in chunks)
    idx = sweep_replica(len(lens), B)
    assert BUCKET_MIN <= idx.size < BUCKET_SMALL_MAX and set(idx.tolist()) == set(range(len(lens)))


@pytest.mark.gpu
@pytest.mark.parametrize("alg", range(1, 9))
@pytest.mark.parametrize("mode", MODES)
def test_boundary_sweep_device(gpu, oracle, mode, alg):
    """Below the threshold: md_keyed_kernel / gost_keyed_kernel after
    key_index_check_kernel.  Replicated above it: the keyed tile kernel (HMAC,
    suffix: MD5, SHA-1, SHA-224/256), md_keyed_kernel over the bucketing
    order (prefix, SHA-384/512), the GOST keyed kernel, the index check fused
    into the bucket count."""
    B = BLOCK[alg]
    keys, data, offs, lens, kidx = sweep_inputs(B)
    assert long_key_phases(keys, B) == {0, 1, 2, 3}
    exp = sweep_expected(oracle, alg, mode)
    d = _dev(data)
    for lo, hi in sweep_chunks(len(lens)):
        assert hi - lo < BUCKET_MIN
        got = _run_dev(gpu, alg, mode, keys, d, offs[lo:hi], lens[lo:hi], kidx[lo:hi])
        bad = np.nonzero((got != exp[lo:hi]).any(axis=1))[0]
        assert bad.size == 0, (alg, mode, [(int(lens[lo + i]), len(keys[kidx[lo + i]])) for i in bad[:8]])
    idx = sweep_replica(len(lens), B)
    assert BUCKET_MIN <= idx.size < BUCKET_SMALL_MAX
    got = _run_dev(gpu, alg, mode, keys, d, offs[idx], lens[idx], kidx[idx])
    bad = np.nonzero((got != exp[idx]).any(axis=1))[0]
    assert bad.size == 0, (alg, mode, [(int(lens[idx[i]]), len(keys[kidx[idx[i]]])) for i in bad[:8]])


@pytest.mark.gpu
@pytest.mark.parametrize("alg", [1, 6, 7])
@pytest.mark.parametrize("mode", MODES)
def test_boundary_sweep_host(gpu, oracle, mode, alg):
    keys, data, offs, lens, kidx = sweep_inputs(BLOCK[alg])
    exp = sweep_expected(oracle, alg, mode)
    for lo, hi in sweep_chunks(len(lens)):
        got = gpu.hash_batch_keyed(alg, mode, keys, data, key_index=kidx[lo:hi], offsets=offs[lo:hi],
                                   lengths=lens[lo:hi])
        assert np.array_equal(got, exp[lo:hi]), (alg, mode)


# ------------------------------------------------------------ b. long messages
LONG = (4095, 4096, 4097, 8192 + 3, 65535, 65536, 70001)
_LONG = {}


def long_inputs(B):
    """42 long records (6 keys x 7 lengths) with a 0..200-byte record after
    every third one, and 4,200 filler messages of 0..100 bytes behind them
    in the same buffer -> (keys, data, offsets, lengths, key_index, nlong)."""
    if B not in _LONG:
        rng = np.random.default_rng(2000 + B)
        keys = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (0, B - 1, B, B + 1, 2 * B + 1, 3 * B + 5)]
        lens, kidx = [], []
        for k in range(len(keys)):
            for j, n in enumerate(LONG):
                lens.append(n)
                kidx.append(k)
                if (k * len(LONG) + j) % 3 == 2:
                    lens.append(int(rng.integers(0, 201)))
                    kidx.append(int(rng.integers(0, len(keys))))
        nlong = len(lens)
        lens += rng.integers(0, 101, 4200).tolist()
        kidx += rng.integers(0, len(keys), 4200).tolist()
        lens, kidx = np.array(lens, np.uint32), np.array(kidx, np.uint32)
        data, offs = _place(lens, 0x10 + B, count_from=4095)   # the long records step through the phases
        _LONG[B] = (keys, data, offs, lens, kidx, nlong)
    return _LONG[B]


def test_long_inputs():
    """CPU: the long records start at different byte phases, end lanes of one
    wave at different blocks, and the bucketed batch is one."""
    for B in (64, 128):
        keys, data, offs, lens, kidx, nlong = long_inputs(B)
        assert [len(k) // B * B for k in keys] == [0, 0, B, B, 2 * B, 3 * B]
        big = lens[:nlong] >= 4095
        assert int(big.sum()) == 42 and 0 < int((~big).sum()) and int(lens[:nlong][~big].max()) <= 200
        assert {int(o) % 16 for o in offs[:nlong][big]} == set(range(16))
        assert nlong < 64 and BUCKET_MIN <= len(lens) < BUCKET_SMALL_MAX
        assert int(lens[nlong:].max()) <= 100 and int((offs + lens).max()) <= data.size


@pytest.mark.gpu
@pytest.mark.parametrize("alg", range(1, 9))
@pytest.mark.parametrize("mode", MODES)
def test_long_messages_keyed(gpu, oracle, mode, alg):
    """Multi-KiB messages in md_keyed_kernel (every hash and mode, prefix with
    0, B, 2B and 3B bytes of the key already in the mid-state: the bit length
    is full + rest + len) and gost_keyed_kernel; then the same records as the
    top length classes (above 4 KiB) of a bucketed batch, in shuffled order."""
    keys, data, offs, lens, kidx, nlong = long_inputs(BLOCK[alg])
    exp = oracle.batch_keyed(alg, mode, keys, data, kidx, offs, lens)
    d = _dev(data)
    got = _run_dev(gpu, alg, mode, keys, d, offs[:nlong], lens[:nlong], kidx[:nlong])
    bad = np.nonzero((got != exp[:nlong]).any(axis=1))[0]
    assert bad.size == 0, (alg, mode, [(int(lens[i]), len(keys[kidx[i]])) for i in bad[:8]])
    idx = np.random.default_rng(alg * 4 + mode).permutation(len(lens))
    got = _run_dev(gpu, alg, mode, keys, d, offs[idx], lens[idx], kidx[idx])
    bad = np.nonzero((got != exp[idx]).any(axis=1))[0]
    assert bad.size == 0, (alg, mode, [(int(lens[idx[i]]), len(keys[kidx[idx[i]]])) for i in bad[:8]])


# ---------------------------------------------------------------- c. table size
TABLE_COMBOS = ((1, 1), (1, 2), (1, 3), (4, 1), (6, 1), (7, 1), (8, 1), (7, 2))


def table_keys(nkeys, B, seed):
    """nkeys keys of random 0..2B+8 bytes; in every group of 64 keys (a wave
    of the MD key prep) one key longer than B and, where the group has a
    second key, one empty key, at random lanes."""
    rng = np.random.default_rng(seed)
    klen = rng.integers(0, 2 * B + 9, nkeys)
    for g in range(0, nkeys, 64):
        n = min(64, nkeys - g)
        lanes = rng.permutation(n)
        klen[g + lanes[0]] = B + 1 + int(rng.integers(0, B + 8))
        if n > 1:
            klen[g + lanes[1]] = 0
    return [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in klen]


def table_msgs(nkeys, count, seed):
    """count messages of 0..200 bytes; every key index used, the highest by
    the first and the last message."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 201, count).astype(np.uint32)
    kidx = rng.integers(0, nkeys, count).astype(np.uint32)
    assert count >= nkeys + 2
    kidx[1 + rng.permutation(count - 2)[:nkeys]] = np.arange(nkeys, dtype=np.uint32)
    kidx[0] = kidx[-1] = nkeys - 1
    data, offs = _place(lens, seed)
    return data, offs, lens, kidx


@pytest.mark.parametrize("nkeys", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_table_inputs(nkeys):
    """CPU: each 64-key group diverges and every index is used."""
    for B in (64, 128):
        keys = table_keys(nkeys, B, 3000 + nkeys)
        assert len(keys) == nkeys and max(len(k) for k in keys) <= 2 * B + 8
        for g in range(0, nkeys, 64):
            grp = [len(k) for k in keys[g:g + 64]]
            assert max(grp) > B and (len(grp) == 1 or min(grp) == 0)
    count = max(2 * nkeys, 600)
    _, _, lens, kidx = table_msgs(nkeys, count, 3100 + nkeys)
    assert set(kidx.tolist()) == set(range(nkeys)) and kidx[0] == kidx[-1] == nkeys - 1
    assert len(lens) == count < BUCKET_MIN and int(lens.max()) <= 200


@pytest.mark.gpu
@pytest.mark.parametrize("nkeys", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_table_size(gpu, oracle, nkeys):
    """One key .. 1000 keys: md_key_prep_kernel (64 keys per block: one lane,
    a partial, a full, several and a partial last block) for MD5 in HMAC and
    prefix mode (suffix has no prep: its table only carries the bytes),
    SHA-256, SHA-512 and GOST 512 HMAC, gost_key_prep_kernel (256-thread
    blocks) in HMAC and prefix mode; the batch then reads mid-state
    k * 2 * kMidWords for every k, the last one first and last."""
    count = max(2 * nkeys, 600)
    data, offs, lens, kidx = table_msgs(nkeys, count, 3100 + nkeys)
    d = _dev(data)
    for alg, mode in TABLE_COMBOS:
        keys = table_keys(nkeys, BLOCK[alg], 3000 + nkeys)
        exp = oracle.batch_keyed(alg, mode, keys, data, kidx, offs, lens)
        got = _run_dev(gpu, alg, mode, keys, d, offs, lens, kidx)
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert bad.size == 0, (alg, mode, nkeys, sorted({int(kidx[i]) for i in bad})[:16])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 3])
def test_table_1000_keys_tiles(gpu, oracle, mode):
    """1000 keys and 6000 messages: the keyed tile kernel of MD5 with a large table."""
    data, offs, lens, kidx = table_msgs(1000, 6000, 3200 + mode)
    keys = table_keys(1000, 64, 3300 + mode)
    exp = oracle.batch_keyed(1, mode, keys, data, kidx, offs, lens)
    got = _run_dev(gpu, 1, mode, keys, _dev(data), offs, lens, kidx)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (mode, sorted({int(kidx[i]) for i in bad})[:16])


@pytest.mark.gpu
def test_table_one_key_checked_and_unchecked(gpu, oracle):
    """One key without key_index (no index check) and with an all-zero index
    (key_index_check_kernel): the same digests, the oracle's."""
    data, offs, lens, _ = table_msgs(1, 600, 3400)
    d = _dev(data)
    zero = np.zeros(len(lens), np.uint32)
    for alg, mode in TABLE_COMBOS:
        keys = table_keys(1, BLOCK[alg], 3400 + alg)
        exp = oracle.batch_keyed(alg, mode, keys, data, None, offs, lens)
        assert np.array_equal(_run_dev(gpu, alg, mode, keys, d, offs, lens, None), exp), (alg, mode)
        assert np.array_equal(_run_dev(gpu, alg, mode, keys, d, offs, lens, zero), exp), (alg, mode)


# ----------------------------------------------------------- d. caller geometry
def scattered_table(seed=4000):
    """(key_table, ranges): 15 keys scattered in a blob of random decoy bytes
    with gaps, in shuffled order (key_offsets is not monotonic); key 13 is a
    strict substring of the 300-byte key's range, key 14 the same range as
    the 129-byte key."""
    rng = np.random.default_rng(seed)
    lens = [0, 1, 5, 64, 65, 127, 128, 129, 200, 263, 16, 300, 37]
    pos, ranges = 3, []
    for n in lens:
        ranges.append((pos, n))
        pos += n + int(rng.integers(1, 23))
    ranges = [ranges[i] for i in rng.permutation(len(ranges))]
    big = next(r for r in ranges if r[1] == 300)
    ranges.append((big[0] + 41, 130))                                     # inside the 300-byte key
    ranges.append(next(r for r in ranges if r[1] == 129))                 # identical ranges
    blob = rng.integers(0, 256, pos + 9, dtype=np.uint8)
    koff = np.array([o for o, _ in ranges], np.uint64)
    klen = np.array([n for _, n in ranges], np.uint32)
    return (blob, koff, klen), ranges


def geometry_msgs():
    rng = np.random.default_rng(4001)
    lens = rng.integers(0, 201, 600).astype(np.uint32)
    data, offs = _place(lens, 4002)
    return data, offs, lens


def test_scattered_table_is_scattered():
    (blob, koff, klen), ranges = scattered_table()
    o = koff.astype(np.int64)
    assert (np.diff(o) < 0).any() and (np.diff(o) > 0).any()             # not monotonic
    assert not np.array_equal(np.sort(o), np.cumsum(klen) - klen)        # not a running sum
    big = next(r for r in ranges if r[1] == 300)
    assert ranges[13][0] > big[0] and sum(ranges[13]) < sum(big)
    assert ranges[14][1] == 129 and ranges.count(ranges[14]) == 2 and int((koff + klen).max()) <= blob.size
    assert {0, 1} <= set(klen.tolist()) and int(klen.max()) > 2 * 128


@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("alg", [1, 6, 7])
def test_caller_key_geometry(gpu, oracle, alg, device):
    """key_offsets with gaps, out of order, overlapping and identical, and
    key_offsets None (every key starts at the blob's first byte); the oracle
    receives the same (blob, offsets, lengths).  The packed keys= list of the
    same keys gives the same digests."""
    table, ranges = scattered_table()
    blob = table[0]
    data, offs, lens = geometry_msgs()
    kidx = ((np.arange(len(lens)) * 7 + 3) % len(ranges)).astype(np.uint32)     # 15 keys, every one used
    assert set(kidx.tolist()) == set(range(len(ranges)))
    packed = [bytes(blob[o:o + n]) for o, n in ranges]
    none_table = (blob, None, np.array([130, 7, 66], np.uint32))
    kidx3 = (np.arange(len(lens)) % 3).astype(np.uint32)
    d = _dev(data) if device else None

    def run(mode, ki, **keys):
        if device:
            return _run_dev(gpu, alg, mode, keys.pop("keys", None), d, offs, lens, ki, **keys)
        return gpu.hash_batch_keyed(alg, mode, keys.pop("keys", None), data, key_index=ki, offsets=offs, lengths=lens,
                                    **keys)
    for mode in MODES:
        exp = oracle.batch_keyed(alg, mode, None, data, kidx, offs, lens, key_table=table)
        got = run(mode, kidx, key_table=table)
        assert np.array_equal(got, exp), (alg, mode)
        assert np.array_equal(run(mode, kidx, keys=packed), got), (alg, mode)
        exp = oracle.batch_keyed(alg, mode, None, data, kidx3, offs, lens, key_table=none_table)
        assert np.array_equal(run(mode, kidx3, key_table=none_table), exp), (alg, mode)
        # the header's reading of NULL offsets: keys 0..2 are the blob's first 130, 7 and 66 bytes
        first = [bytes(blob[:n]) for n in (130, 7, 66)]
        assert np.array_equal(exp, oracle.batch_keyed(alg, mode, first, data, kidx3, offs, lens)), (alg, mode)


# ------------------------------------------------------------ e. cache identity
@pytest.mark.gpu
def test_key_cache_identity(gpu, oracle):
    """The cache identity is (device, alg, kind, key bytes ++ key lengths):
    the same bytes split differently, one table in every mode, and one key as
    lcb_hash_batch's HMAC key (kind 0) and as a one-key table are distinct
    entries with their own mid-states; a table that comes back adds none."""
    import torch
    L = gpu.lib()
    torch.cuda.synchronize()
    assert L.lcb_hash_key_cache_flush() == 0 and L.lcb_hash_key_cache_entries() == 0
    data, offs, lens = geometry_msgs()
    d, do, dl = _dev(data), _dev(offs, np.int64), _dev(lens, np.int32)
    kidx = (np.arange(len(lens)) % 2).astype(np.uint32)
    entries = 0

    def keyed(alg, mode, keys, ki, new):
        nonlocal entries
        got = _run_dev(gpu, alg, mode, keys, d, offs, lens, ki)
        assert np.array_equal(got, oracle.batch_keyed(alg, mode, keys, data, ki, offs, lens)), (alg, mode, keys)
        entries += new
        assert L.lcb_hash_key_cache_entries() == entries, (alg, mode, keys)

    for mode in (1, 2):
        keyed(1, mode, [b"ab", b"c"], kidx, 1)
        keyed(1, mode, [b"a", b"bc"], kidx, 1)
        keyed(1, mode, [b"abc"], None, 1)
        keyed(1, mode, [b"ab", b"c"], kidx, 0)          # back again: found, not rebuilt
    # all-empty table against a zero byte (an empty blob is uploaded as one zero byte)
    keyed(1, 1, [b""], None, 1)
    keyed(1, 1, [b"\0"], None, 1)
    table = [bytes(range(70)), b"", bytes(range(3, 140))]
    kidx3 = (np.arange(len(lens)) % 3).astype(np.uint32)
    for mode, new in ((1, 1), (2, 1), (3, 1), (1, 0)):
        keyed(4, mode, table, kidx3, new)
    key = bytes(range(100, 180))                          # longer than MD5's block: H(key) in both preps
    got = gpu.hash_batch(1, d, offsets=do, lengths=dl, key=key).cpu().numpy()
    assert np.array_equal(got, oracle.batch(1, data, offs, lens, key=key))
    entries += 1
    assert L.lcb_hash_key_cache_entries() == entries
    keyed(1, 1, [key], None, 1)
    got = gpu.hash_batch(1, d, offsets=do, lengths=dl, key=key).cpu().numpy()
    assert np.array_equal(got, oracle.batch(1, data, offs, lens, key=key))
    assert L.lcb_hash_key_cache_entries() == entries <= 16


# -------------------------------------------------------- f. cross-stream readiness
@pytest.mark.gpu
def test_key_table_ready_on_a_second_stream(gpu, oracle):
    """A new key table is prepared on stream A behind work that keeps A busy
    (one key, no key_index: no host wait for the batch); the same table is
    then used at once on stream B, which must wait for A's prep (the cache
    entry's `ready` event).  Both batches equal the oracle.  The same for a
    single-key HMAC of lcb_hash_batch.  One pass.

    The key is 256 KiB long (32 KiB for GOST), so that the prep, one lane
    hashing the whole key, runs for 3..8 ms while B's call is enqueued
    within 0.3 ms of A's.  Measured on an MI355X: the upload of a new table
    (a pageable copy) holds the caller until stream A has drained the fills
    (call time 0.4 / 1.2 / 4.5 ms behind 8 / 32 / 128 fills), so the fills
    alone leave B nothing to wait for.

    What this test cannot do: on that machine B's batch finished only after
    A's prep even in a build with the hipStreamWaitEvent taken out (the
    runtime ran the two streams one after the other; five B streams made the
    B-side calls themselves block for the prep's 4 ms), and that build passes
    this test.  It checks the guarantee, and catches a table handed out
    unprepared wherever the streams do overlap; it does not prove the wait is
    what provides it."""
    import torch
    L = gpu.lib()
    torch.cuda.synchronize()
    assert L.lcb_hash_key_cache_flush() == 0
    data, offs, lens = geometry_msgs()
    offs, lens = offs[:64], lens[:64]
    half = len(lens) // 2
    d, do, dl = _dev(data), _dev(offs, np.int64), _dev(lens, np.int32)
    big = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    cases = [(1, 1), (1, 2), (6, 1), (7, 2), (1, 0), (7, 0)]              # mode 0: hash_batch(key=)
    for n, (alg, mode) in enumerate(cases):
        key = gen_stream(0xF00 + n, (32 if alg == 7 else 256) * 1024 + 9).tobytes()   # a new table each time

        def call(lo, hi):
            if mode == 0:
                return gpu.hash_batch(alg, d, offsets=do[lo:hi], lengths=dl[lo:hi], key=key)
            return gpu.hash_batch_keyed(alg, mode, [key], d, offsets=do[lo:hi], lengths=dl[lo:hi])
        before = L.lcb_hash_key_cache_entries()
        sa.wait_stream(torch.cuda.current_stream())
        sb.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(sa):
            for _ in range(8):
                big.fill_(1)                       # keeps A busy while the calls below return
            ga = call(0, half)
        with torch.cuda.stream(sb):
            gb = call(half, len(lens))
        torch.cuda.synchronize()
        assert L.lcb_hash_key_cache_entries() == before + 1, (alg, mode)   # B found A's entry
        if mode == 0:
            exp = oracle.batch(alg, data, offs, lens, key=key)
        else:
            exp = oracle.batch_keyed(alg, mode, [key], data, None, offs, lens)
        assert np.array_equal(ga.cpu().numpy(), exp[:half]), (alg, mode, "stream A")
        assert np.array_equal(gb.cpu().numpy(), exp[half:]), (alg, mode, "stream B")
