"""numpy references of sa_taps_unfold / sa_taps_fold (csrc/taps.hip), written from their definitions in include/synthanatomy_hip.h: plain loops over the
k^3 taps, whole-array arithmetic over the cells."""
import numpy as np


def conv_out(I, k, s, p, d):
    return (I + 2 * p - d * (k - 1) - 1) // s + 1


def convT_out(I, k, s, p, op, d):
    return (I - 1) * s - 2 * p + d * (k - 1) + op + 1


def _axis(n, mult, t, step, off, size):
    i = np.arange(n) * mult + t * step + off
    return i, (i >= 0) & (i < size)


def unfold(x, grid, k, mult, step, off, ld):
    """Xc[n][m][t] = x[n][m * mult + t * step + off] per axis, zero outside; float32 [N, *grid, ld], columns k^3 .. ld - 1 zero"""
    N, D, H, W = x.shape
    out = np.zeros((N, *grid, ld), dtype=np.float32)
    for td in range(k):
        idx_d, ok_d = _axis(grid[0], mult, td, step, off, D)
        for th in range(k):
            idx_h, ok_h = _axis(grid[1], mult, th, step, off, H)
            for tw in range(k):
                idx_w, ok_w = _axis(grid[2], mult, tw, step, off, W)
                t = (td * k + th) * k + tw
                md, mh, mw = np.nonzero(ok_d)[0], np.nonzero(ok_h)[0], np.nonzero(ok_w)[0]
                if len(md) and len(mh) and len(mw):
                    out[np.ix_(range(N), md, mh, mw, [t])] = x[np.ix_(range(N), idx_d[md], idx_h[mh], idx_w[mw])][..., None]
    return out


def fold(P, bias, odims, k, s, p, d):
    """(out, A) in float64: out[n][o] = bias + sum of P[n][(o + p - t * d) / s][t] over the taps whose quotient is an integer inside the cell grid;
    A the same over absolute values"""
    N, Dc, Hc, Wc, ld = P.shape
    P = P.astype(np.float64)
    out = np.full((N, *odims), float(bias), dtype=np.float64)
    A = np.full((N, *odims), abs(float(bias)), dtype=np.float64)

    def axis(O, C, t):
        nmr = np.arange(O) + p - t * d
        ok = (nmr % s == 0) & (nmr // s >= 0) & (nmr // s < C)
        return np.nonzero(ok)[0], (nmr // s)[ok]

    for td in range(k):
        od, qd = axis(odims[0], Dc, td)
        for th in range(k):
            oh, qh = axis(odims[1], Hc, th)
            for tw in range(k):
                ow, qw = axis(odims[2], Wc, tw)
                if not (len(od) and len(oh) and len(ow)):
                    continue
                t = (td * k + th) * k + tw
                v = P[np.ix_(range(N), qd, qh, qw, [t])][..., 0]
                out[np.ix_(range(N), od, oh, ow)] += v
                A[np.ix_(range(N), od, oh, ow)] += np.abs(v)
    return out, A
