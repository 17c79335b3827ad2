"""Restatement of the counter-based dropout keep function of csrc/dropout.h (Philox4x32-10, vectorised over element indices with numpy):
counter = (lo32(e >> 2), hi32(e >> 2), site, 0), key = (lo32(seed), hi32(seed)), word = output[e & 3], keep iff word >= min(floor(fp32(p) 2^32), 2^32 - 1),
kept values scaled by fp32(1 / (1 - fp32(p)))."""
import math

import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)


def _philox(c0, c1, c2, c3, k0, k1):
    """arrays of uint64 holding 32-bit lanes; k0 / k1 python ints"""
    for r in range(10):
        if r:
            k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)), (p1 & _LO), ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)), (p0 & _LO)
    return c0, c1, c2, c3


def philox4x32_10(ctr, key):
    """one block: ctr 4 x uint32, key 2 x uint32 -> 4 x uint32 (python ints)"""
    out = _philox(*(np.array([c], dtype=np.uint64) for c in ctr), int(key[0]), int(key[1]))
    return tuple(int(o[0]) for o in out)


def threshold(p):
    return min(int(math.floor(float(np.float32(p)) * 4294967296.0)), 0xFFFFFFFF)


def scale(p):
    return float(np.float32(1.0 / (1.0 - float(np.float32(p)))))


def words(seed, site, e):
    """the Philox word of each element index in the uint64 array e"""
    e = np.asarray(e, dtype=np.uint64)
    q = e >> np.uint64(2)
    zero = np.zeros_like(q)
    o = _philox(q & _LO, q >> np.uint64(32), zero + np.uint64(site), zero, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    sel = (e & np.uint64(3)).astype(np.int64)
    return np.choose(sel, o)


def keep_mask(seed, site, start, n, p):
    """bool keep decisions of elements start .. start + n - 1"""
    return words(seed, site, np.arange(start, start + n, dtype=np.uint64)) >= np.uint64(threshold(p))


def scaled_mask(seed, site, shape, p, start=0):
    """float32 keep / (1 - p) of a contiguous tensor of `shape` (element index = flat index + start)"""
    n = int(np.prod(shape))
    return (keep_mask(seed, site, start, n, p).astype(np.float32) * np.float32(scale(p))).reshape(shape)
