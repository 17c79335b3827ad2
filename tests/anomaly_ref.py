"""fp64 restatement of the anomaly-map rule (csrc/anomaly.hip computes it in fp32).  numpy only.

    e = |x - r| / max(x - r, 0) / max(r - x, 0);  u(p) = m[p // f] inside the volume, 0 outside;  w = the separable "same" Gaussian of u with the
    given taps (the fp32 taps the kernel gets, used here as fp64 numbers);  a = e w  (a = e without a weight grid)

``cell_shift`` and ``taps`` are open on purpose: the GPU tests' witnesses are this reference with the wrong cell boundary ((p + 1) // f) and with taps
left unnormalised."""
import numpy as np


def unnormalised_taps(sigma):
    """exp(-i^2 / 2 sigma^2) over [-R, R], R = ceil(3 sigma), rounded to fp32 and NOT divided by their sum: a witness"""
    R = int(np.ceil(3.0 * sigma))
    i = np.arange(-R, R + 1, dtype=np.float64)
    return np.exp(-(i * i) / (2.0 * sigma * sigma)).astype(np.float32) if R else np.ones(1, dtype=np.float32)


def upsample(m, shape, cell_shift=0):
    """u[p] = m[(p + cell_shift) // f] per axis (indices past the last cell stay in it); cell_shift = 0 is the rule"""
    u = np.asarray(m, dtype=np.float64)
    for axis, n in enumerate(shape):
        f = n // u.shape[axis]
        assert f * u.shape[axis] == n
        idx = np.minimum((np.arange(n) + cell_shift) // f, u.shape[axis] - 1)
        u = np.take(u, idx, axis=axis)
    return u


def smooth(u, taps):
    """sum_t g(t_D) g(t_H) g(t_W) u(v + t) with zeros outside the volume, one axis after the other in fp64"""
    g = np.asarray(taps, dtype=np.float64)
    R = (len(g) - 1) // 2
    out = np.asarray(u, dtype=np.float64)
    for axis in range(3):
        n = out.shape[axis]
        pad = [(0, 0)] * 3
        pad[axis] = (R, R)
        p = np.pad(out, pad)
        acc = np.zeros_like(out)
        for t in range(-R, R + 1):
            acc += g[t + R] * np.take(p, np.arange(n) + t + R, axis=axis)
        out = acc
    return out


def residual(x, r, mode="abs"):
    d = np.asarray(x, dtype=np.float64) - np.asarray(r, dtype=np.float64)
    return {"abs": np.abs(d), "positive": np.maximum(d, 0.0), "negative": np.maximum(-d, 0.0)}[mode]


def weight_ref(m, shape, taps, cell_shift=0):
    return smooth(upsample(m, shape, cell_shift), taps)


def anomaly_ref(x, r, m, taps, mode="abs", cell_shift=0):
    """(a, w) in fp64 for one volume x, r [D, H, W] and latent grid m [d, h, w] (None: a = e, w = 1)"""
    e = residual(x, r, mode)
    if m is None:
        return e, np.ones_like(e)
    w = weight_ref(m, e.shape, taps, cell_shift)
    return e * w, w


def anomaly_brute(x, r, m, taps, mode="abs"):
    """the rule as written, voxel by voxel and tap by tap (tiny volumes only)"""
    D, H, W = x.shape
    f = [n // c for n, c in zip(x.shape, m.shape)]
    g = np.asarray(taps, dtype=np.float64)
    R = (len(g) - 1) // 2
    a = np.zeros(x.shape, dtype=np.float64)
    for vd in range(D):
        for vh in range(H):
            for vw in range(W):
                w = 0.0
                for td in range(-R, R + 1):
                    for th in range(-R, R + 1):
                        for tw in range(-R, R + 1):
                            pd, ph, pw = vd + td, vh + th, vw + tw
                            if 0 <= pd < D and 0 <= ph < H and 0 <= pw < W:
                                w += g[td + R] * g[th + R] * g[tw + R] * float(m[pd // f[0], ph // f[1], pw // f[2]])
                d = float(x[vd, vh, vw]) - float(r[vd, vh, vw])
                e = abs(d) if mode == "abs" else max(d, 0.0) if mode == "positive" else max(-d, 0.0)
                a[vd, vh, vw] = e * w
    return a


def bins(a, inv_bin):
    """min(255, int(a * inv_bin)) with the product one fp32 multiply: bit for bit what the kernel bins"""
    p = np.asarray(a, dtype=np.float32) * np.float32(inv_bin)
    return np.minimum(255, p.astype(np.int64))


def histograms(a, labels, inv_bin):
    """[2, 256] int64: label class, bin"""
    b = bins(a, inv_bin).ravel()
    cls = np.zeros(b.shape, dtype=np.int64) if labels is None else (np.asarray(labels).ravel() != 0).astype(np.int64)
    return np.bincount(cls * 256 + b, minlength=512).reshape(2, 256)


def counts(a, labels, t):
    """(TP, FP, FN) of [a >= t] (both fp32) against the label"""
    pred = np.asarray(a, dtype=np.float32) >= np.float32(t)
    lab = np.zeros(pred.shape, dtype=bool) if labels is None else np.asarray(labels) != 0
    return int((pred & lab).sum()), int((pred & ~lab).sum()), int((~pred & lab).sum())
