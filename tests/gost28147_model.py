"""numpy restatement of GOST 28147-89 as include/lcb_gost28147_gpu.h defines
the batch (the reference's aligned path, gost28147.h:244-566), vectorised over
blocks for ECB and over buffers for the MAC.  Test infrastructure: the GPU
tests compare against it on the machine that has no reference; its own
agreement with the reference is pinned by tests/golden/gost28147.json
(tests/test_gost28147_model.py)."""
import numpy as np


def rotl32(v, n):
    v = v.astype(np.uint32)
    return ((v << np.uint32(n)) | (v >> np.uint32(32 - n))).astype(np.uint32)


def tables(sbox):
    """The four expanded tables of gost28147_init (gost28147.h:494-507)."""
    s = np.frombuffer(bytes(sbox), np.uint8).astype(np.uint32).reshape(8, 16)
    i = np.arange(256)
    return np.stack([rotl32((s[2 * k][i & 15] | (s[2 * k + 1][i >> 4] << np.uint32(4))) << np.uint32(8 * k), 11)
                     for k in range(4)])


def packed_table(sbox):
    """P[i] = rotl32(t0[i] | t1[i] << 8 | t2[i] << 16 | t3[i] << 24, 11), tk
    the significant byte of table k (a Python copy of the library's)."""
    s = np.frombuffer(bytes(sbox), np.uint8).astype(np.uint32).reshape(8, 16)
    i = np.arange(256)
    v = np.zeros(256, np.uint32)
    for k in range(4):
        v |= (s[2 * k][i & 15] | (s[2 * k + 1][i >> 4] << np.uint32(4))) << np.uint32(8 * k)
    return rotl32(v, 11)


def _f(T, x):
    return T[0][x & 255] ^ T[1][(x >> 8) & 255] ^ T[2][(x >> 16) & 255] ^ T[3][x >> 24]


def _key_words(key, be):
    return np.frombuffer(bytes(key)[:32], ">u4" if be else "<u4").astype(np.uint32)


def _rounds(T, k, n1, n2, order):
    for idx, r in enumerate(order):
        if idx % 2 == 0:
            n2 = n2 ^ _f(T, (n1 + k[r]).astype(np.uint32))
        else:
            n1 = n1 ^ _f(T, (n2 + k[r]).astype(np.uint32))
    return n1, n2


ENC_ORDER = list(range(8)) * 3 + list(range(7, -1, -1))
DEC_ORDER = list(range(8)) + list(range(7, -1, -1)) * 3
MAC_ORDER = list(range(8)) * 2


def _load(blocks, be):
    """blocks: (n, 8) uint8 -> n1, n2 (gost28147.h:347-349 / 383-384)."""
    w = np.ascontiguousarray(blocks).view(">u4" if be else "<u4").astype(np.uint32)
    return (w[:, 1], w[:, 0]) if be else (w[:, 0], w[:, 1])


def _store(o1, o2, be):
    """Output words (dst_n1, dst_n2) -> (n, 8) uint8 (gost28147.h:350-351 / 387-388)."""
    w = np.stack([o2, o1] if be else [o1, o2], axis=1).astype(">u4" if be else "<u4")
    return w.view(np.uint8).reshape(-1, 8)


def crypt_blocks(op, key, sbox, blocks, be=False):
    """ECB over (n, 8) uint8 blocks; op 0 encrypt, 1 decrypt."""
    T = tables(sbox)
    n1, n2 = _load(blocks, be)
    with np.errstate(over="ignore"):
        n1, n2 = _rounds(T, _key_words(key, be), n1, n2, DEC_ORDER if op else ENC_ORDER)
    return _store(n2, n1, be)


def crypt_batch(op, key, sbox, src, offs, lens, be=False, dst=None):
    """The batch on a flat uint8 array: whole blocks of every buffer are
    transformed, every other byte of dst (default: zeros) is left alone."""
    src = np.asarray(src, np.uint8)
    out = np.zeros(src.size, np.uint8) if dst is None else dst
    offs = np.asarray(offs, np.int64)
    nb = np.asarray(lens, np.int64) >> 3
    if int(nb.sum()) == 0:
        return out
    # byte index of every block
    start = np.repeat(offs, nb) + 8 * (np.arange(int(nb.sum())) - np.repeat(np.cumsum(nb) - nb, nb))
    idx = start[:, None] + np.arange(8)[None, :]
    out[idx] = crypt_blocks(op, key, sbox, src[idx], be)
    return out


def mac_batch(key, sbox, data, offs, lens, be=False, mac_size=8):
    """(count, mac_size) uint8: gost28147_blocks_mac[_be] + gost28147_final[_be]."""
    data = np.asarray(data, np.uint8)
    offs = np.asarray(offs, np.int64)
    nb = np.asarray(lens, np.int64) >> 3
    T, k = tables(sbox), _key_words(key, be)
    m0 = np.zeros(len(offs), np.uint32)
    m1 = np.zeros(len(offs), np.uint32)
    with np.errstate(over="ignore"):
        for j in range(int(nb.max()) if len(nb) else 0):
            live = np.nonzero(nb > j)[0]
            idx = (offs[live] + 8 * j)[:, None] + np.arange(8)[None, :]
            n1, n2 = _load(data[idx], be)
            a, b = _rounds(T, k, m0[live] ^ n1, m1[live] ^ n2, MAC_ORDER)
            m0[live], m1[live] = a, b
    w = np.stack([m0, m1], axis=1).astype(">u4" if be else "<u4")
    return np.ascontiguousarray(w.view(np.uint8).reshape(-1, 8)[:, :mac_size])


def ragged(seed, n, hi):
    """The fixture's layout: n buffers of 0..hi-1 bytes packed back to back."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, hi, n).astype(np.uint32)
    offs = np.zeros(n, np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return offs, lens
