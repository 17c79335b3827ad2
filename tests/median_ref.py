"""numpy reference of the masked median rule of DESIGN §7.18 (sa_anomaly_median), one volume at a time:
  m0 = [b != 0] (all true without a mask);  m = m0 eroded e times with the 6-neighbourhood, everything outside the volume false
  a' = m ? a : +0.0f (a select);  f(v) = the element of rank (k^3 - 1) / 2 among a'(v + t), t in [-k/2, k/2]^3, +0.0f outside the volume, ordered by
  key = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000);  out = m ? f : +0.0f
and the summaries by the definitions of the sa_anomaly_map record.  The output is bits of the input: the kernel is held to this bit for bit."""
import numpy as np

ZERO_KEY = np.uint32(0x80000000)      # the key of +0.0f


def to_key(x):
    """uint32 keys of fp32 values: unsigned order of the keys = the rule's total order (-nan < -inf < ... < -0 < +0 < ... < +inf < +nan)"""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return bits ^ np.where(bits >> np.uint32(31) != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def from_key(key):
    key = np.ascontiguousarray(key, dtype=np.uint32)
    return (key ^ np.where(key >> np.uint32(31) != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


def erode(m0, e):
    """e times: a voxel stays where it and its six neighbours are set; a neighbour outside the volume is not"""
    m = np.asarray(m0, dtype=bool)
    for _ in range(e):
        p = np.pad(m, 1, constant_values=False)
        m = (p[1:-1, 1:-1, 1:-1] & p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2]
             & p[1:-1, 1:-1, 2:])
    return m


def eroded_mask(shape, mask, e):
    if mask is None:
        if e:
            raise ValueError("erosion without a mask")
        return np.ones(shape, dtype=bool)
    return erode(np.asarray(mask) != 0, e)


def rank_filter_keys(keys, k):
    """the key of rank (k^3 - 1) / 2 of every k^3 window of the uint32 volume ``keys``, padded with the key of +0.0f"""
    D, H, W = keys.shape
    r = k // 2
    p = np.pad(keys, r, constant_values=ZERO_KEY)
    stack = np.stack([p[z:z + D, y:y + H, x:x + W] for z in range(k) for y in range(k) for x in range(k)])
    return np.sort(stack, axis=0)[(k ** 3 - 1) // 2]


def median(a, k, mask=None, e=0):
    """out [D, H, W] fp32 of one volume ``a`` [D, H, W]; ``mask``: foreground where non-zero, or None"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    m = eroded_mask(a.shape, mask, e)
    keys = np.where(m, to_key(a), ZERO_KEY)
    return from_key(np.where(m, rank_filter_keys(keys, k), ZERO_KEY))


def summaries(out, inv_bin, labels=None, threshold=None):
    """the record's words for a finite non-negative ``out``: sum (fp64), max, hist [2, 256] (bin = min(255, int(out * inv_bin)), the product in fp32),
    and tp / fp / fn of [out >= threshold] (None without a threshold); without labels every voxel is class 0"""
    out = np.asarray(out, dtype=np.float32)
    y = np.zeros(out.shape, dtype=bool) if labels is None else np.asarray(labels) != 0
    scaled = out * np.float32(inv_bin)
    assert scaled.dtype == np.float32
    bins = np.minimum(scaled, np.float32(255.0)).astype(np.int64)
    hist = np.stack([np.bincount(bins[~y], minlength=256), np.bincount(bins[y], minlength=256)]).astype(np.int64)
    s = {"sum": float(out.astype(np.float64).sum()), "max": np.float32(max(out.max(), np.float32(0.0))), "hist": hist, "tp": None, "fp": None, "fn": None}
    if threshold is not None:
        pred = out >= np.float32(threshold)
        s.update(tp=int((pred & y).sum()), fp=int((pred & ~y).sum()), fn=int((~pred & y).sum()))
    return s
