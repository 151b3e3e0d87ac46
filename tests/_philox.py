"""numpy Philox4x32-10 and the dropout mask contract of ndcn_amd/csrc/dropout.h - the reference the kernels are tested against.

    p32 = float32(p); s = float32(1) / (float32(1) - p32); T = floor(float64(p32) * 2^32)
    element i = row * H + col: counter (lo32(i >> 2), hi32(i >> 2), lo32(evaluation), hi32(evaluation)), key (lo32(seed), hi32(seed)),
    u = output word i & 3; kept iff u >= T; m = s if kept else 0
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two 32-bit ints; returns four uint64 arrays holding 32-bit words"""
    c = [np.asarray(x, dtype=np.uint64) for x in counter]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & LO, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & LO]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def threshold(p):
    return int(np.floor(np.float64(np.float32(p)) * 2.0 ** 32))


def scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def words(seed, evaluation, n_elems, first=0):
    """the 32-bit word of each element first .. first + n_elems - 1 (uint64 array)"""
    seed, evaluation = int(seed) & (2 ** 64 - 1), int(evaluation) & (2 ** 64 - 1)
    q0, q1 = first >> 2, (first + n_elems + 3) >> 2
    q = np.arange(q0, q1, dtype=np.uint64)
    e_lo, e_hi = np.uint64(evaluation & 0xFFFFFFFF), np.uint64(evaluation >> 32)
    out = philox4x32_10([q & LO, q >> S32, np.full(q.shape, e_lo), np.full(q.shape, e_hi)], (seed & 0xFFFFFFFF, seed >> 32))
    flat = np.stack(out, axis=1).reshape(-1)
    return flat[first - 4 * q0:first - 4 * q0 + n_elems]


def kept(p, seed, evaluation, n_elems, first=0):
    return words(seed, evaluation, n_elems, first) >= np.uint64(threshold(p))


def mask(p, seed, evaluation, n_rows, H, first=0):
    """float32 [n_rows, H]: the factor m of every element (0 or s)"""
    k = kept(p, seed, evaluation, n_rows * H, first)
    return np.where(k, scale(p), np.float32(0.0)).astype(np.float32).reshape(n_rows, H)
