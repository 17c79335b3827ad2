"""Restatement of csrc/augment.hip (sa_augment) in numpy: the spatial modes and the intensity stage in fp64 (the truth the GPU tests compare with), the
same formulas in float32 (the yardstick: what another correct fp32 evaluation loses against fp64), and the Philox / Box-Muller noise.

Conventions (include/synthanatomy_hip.h): axis 0 = D, 1 = H, 2 = W; SIGNED_PERM: source axis perm[a] takes off[perm[a]] + (sign[a] > 0 ? o_a : n_a - 1 - o_a);
AFFINE: p = M . [o - (n_out - 1) / 2; 1] + (ext - 1) / 2 inside the window [off, off + ext), trilinear, a corner outside the window counts as 0.
Noise of voxel e (flat index inside the sample's output), q = e >> 2: words = Philox4x32-10(counter (lo32 q, hi32 q, sample, 0), key (lo32 seed, hi32 seed)),
u_k = (float32(w_k >> 8) + 0.5) * 2^-24 in float32; (n(4q), n(4q + 1)) = sqrt(-2 ln u_0) (cos, sin)(2 pi u_1), (n(4q + 2), n(4q + 3)) the same from (u_2, u_3)."""
import itertools

import numpy as np

from dropout_ref import _LO, _philox

EPS32 = float(np.finfo(np.float32).eps)
GAMMA, SHIFT, NOISE, CLAMP = 1, 2, 4, 8


def signed_perm(x, off, perm, sign, out_dims):
    """x [D, H, W] -> the gather of SA_AUG_SIGNED_PERM, by explicit indices (the tests hold it against np.flip / np.rot90 themselves)"""
    idx = [None] * 3
    grids = np.meshgrid(*(np.arange(n) for n in out_dims), indexing="ij")
    for a in range(3):
        c = grids[a] if sign[a] > 0 else out_dims[a] - 1 - grids[a]
        idx[perm[a]] = off[perm[a]] + c
    return x[idx[0], idx[1], idx[2]]


def affine_positions(M, out_dims, ext):
    """fp64 positions [3, Do, Ho, Wo] inside the source window"""
    M = np.asarray(M, dtype=np.float64).reshape(3, 4)
    g = np.stack(np.meshgrid(*(np.arange(n, dtype=np.float64) - (n - 1) / 2 for n in out_dims), indexing="ij"))
    return np.einsum("ij,j...->i...", M[:, :3], g) + M[:, 3].reshape(3, 1, 1, 1) + ((np.asarray(ext, dtype=np.float64) - 1) / 2).reshape(3, 1, 1, 1)


def _corners(win, pos):
    """the eight corner values [2, 2, 2, ...] (0 outside the window) and the fractions [3, ...] at fp64 positions pos [3, ...]"""
    f = np.floor(pos)
    i = f.astype(np.int64)
    c = np.zeros((2, 2, 2) + pos.shape[1:], dtype=np.float64)
    for a, b, k in itertools.product((0, 1), repeat=3):
        j0, j1, j2 = i[0] + a, i[1] + b, i[2] + k
        ok = (j0 >= 0) & (j0 < win.shape[0]) & (j1 >= 0) & (j1 < win.shape[1]) & (j2 >= 0) & (j2 < win.shape[2])
        c[a, b, k] = np.where(ok, win[np.clip(j0, 0, win.shape[0] - 1), np.clip(j1, 0, win.shape[1] - 1), np.clip(j2, 0, win.shape[2] - 1)], 0.0)
    return c, pos - f


def affine(x, M, out_dims, off=(0, 0, 0), ext=None):
    """fp64 value and the per-voxel error bound of an fp32 evaluation:  delta_a = 8 eps32 max(|p_a|, 1) is what four fp32 operations can move coordinate a,
    the interpolant moves by at most delta_a times the largest corner difference along a -- bounded here by the SUM of the four differences along a, taken
    as the worst over the cells that p +- delta reaches -- and the eight-term fp32 blend adds 8 eps32 max|corner|."""
    ext = list(x.shape) if ext is None else list(ext)
    win = np.asarray(x, dtype=np.float64)[off[0]:off[0] + ext[0], off[1]:off[1] + ext[1], off[2]:off[2] + ext[2]]
    pos = affine_positions(M, out_dims, ext)
    c, t = _corners(win, pos)
    w = [np.stack([1 - t[a], t[a]]) for a in range(3)]
    val = sum(c[a, b, k] * w[0][a] * w[1][b] * w[2][k] for a, b, k in itertools.product((0, 1), repeat=3))
    delta = 8 * EPS32 * np.maximum(np.abs(pos), 1.0)
    bound = np.zeros_like(val)
    for s in itertools.product((-1, 0, 1), repeat=3):
        cs, _ = _corners(win, pos + np.asarray(s, dtype=np.float64).reshape(3, 1, 1, 1) * delta)
        diffs = [np.abs(np.diff(cs, axis=a)).sum(axis=(0, 1, 2)) for a in range(3)]
        bound = np.maximum(bound, sum(delta[a] * diffs[a] for a in range(3)) + 8 * EPS32 * np.abs(cs).max(axis=(0, 1, 2)))
    return val, bound


def intensity(v, flags, gamma=1.0, shift=0.0, std=0.0, noise=None, dtype=np.float64):
    """the intensity stage on one sample v in ``dtype`` arithmetic (float64: the truth; float32: the yardstick); returns (out, min, max)"""
    v = np.asarray(v, dtype=dtype)
    mn, mx = v.min(), v.max()
    if flags & GAMMA:
        rng = dtype(mx - mn)
        v = np.power((v - mn) / dtype(rng + dtype(1e-7)), dtype(gamma)) * rng + mn
    if flags & SHIFT:
        v = v + dtype(shift)
    if flags & NOISE:
        v = v + dtype(std) * np.asarray(noise, dtype=dtype).reshape(v.shape)
    if flags & CLAMP:
        v = np.minimum(np.maximum(v, dtype(0)), dtype(1))
    return v.astype(dtype), mn, mx


def words4(seed, sample, q):
    """the four Philox words of every group index in the uint64 array q: [4, len(q)]"""
    q = np.asarray(q, dtype=np.uint64)
    zero = np.zeros_like(q)
    return np.stack(_philox(q & _LO, q >> np.uint64(32), zero + np.uint64(sample), zero, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def uniform32(w):
    """the kernel's uniform: (float32(w >> 8) + 0.5) * 2^-24 in float32"""
    return (((np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)).astype(np.float32)


def box_muller(w0, w1, dtype=np.float64):
    """two normals from two words; float64: exact uniforms ((w >> 8) + 0.5) 2^-24 and fp64 functions, float32: the kernel's operations in numpy float32"""
    if dtype == np.float32:
        u0, u1 = uniform32(w0), uniform32(w1)
        r, a = np.sqrt(np.float32(-2.0) * np.log(u0)), np.float32(6.2831853071795864769) * u1
        return (r * np.cos(a)).astype(np.float32), (r * np.sin(a)).astype(np.float32)
    u0 = ((np.asarray(w0, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    u1 = ((np.asarray(w1, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    r, a = np.sqrt(-2.0 * np.log(u0)), 2.0 * np.pi * u1
    return r * np.cos(a), r * np.sin(a)


def normals(seed, sample, start, n, dtype=np.float64):
    """n(e) for e = start .. start + n - 1 of one sample (start need not be a multiple of 4: the words of a voxel depend on e alone)"""
    e = np.arange(start, start + n, dtype=np.uint64)
    w = words4(seed, sample, e >> np.uint64(2))
    k = (e & np.uint64(3)).astype(np.int64)
    pair = k >> 1
    w0, w1 = np.where(pair == 0, w[0], w[2]), np.where(pair == 0, w[1], w[3])
    c, s = box_muller(w0, w1, dtype)
    return np.where((k & 1) == 0, c, s)
