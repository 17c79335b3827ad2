"""The ensemble anomaly map (csrc/anomaly.hip: sa_anomaly_map_ensemble) restated for the tests, on top of tests/anomaly_ref.py and
tests/anomaly_bounds.py.  numpy only.

The rule.  K members share the scan x, the residual mode and the taps; member k has a reconstruction r_k and an optional latent grid m_k.  With a_k the
number sa_anomaly_map computes for (x, r_k, m_k):  s = a_0;  s = s + a_k in fp32 for k = 1 .. K - 1, in member order;  a = s * inv_K with
inv_K = np.float32(1.0 / K).  ``compose_fp32`` is that sentence in numpy and carries no tolerance; ``ensemble_ref`` is the fp64 mean of the members'
fp64 references.

The element-wise bound of ``a`` against the fp64 mean (u = 2^-24, gamma_n = n u / (1 - n u), Higham lemma 3.1).  Write A_k for the kernel's fp32 member
map, a_k for its fp64 reference and b_k for the single-member bound of tests/anomaly_bounds.map_bound, |A_k - a_k| <= b_k.  Every A_k is >= 0 (a
residual that is >= 0 times a weight whose terms are all >= 0), so nothing cancels in the sum:

  K - 1 additions   s_j = (s_{j-1} + A_j)(1 + t_j), |t_j| <= u: every A_k ends up multiplied by at most K - 1 factors (1 + t); an fp32 sum of fp32
                    numbers loses nothing to underflow
  inv_K             (1 / K)(1 + d)(1 + h): 1 / K is rounded to a double (|d| <= 2^-53 <= u) and then to fp32 (|h| <= u): 2 factors
  s * inv_K         1 rounding, and at most one gradual-underflow step of 2^-149

  a = (1 / K) sum_k A_k (1 + T_k),  |T_k| <= gamma_{K+2}

  |a - (1 / K) sum_k a_k| <= (1 / K) sum_k |A_k - a_k| + gamma_{K+2} (1 / K) sum_k A_k + 2^-149
                          <= (1 / K) [ (1 + gamma_{K+2}) sum_k b_k + gamma_{K+2} sum_k a_k ] + 2^-149

No number in it is measured.  (Seen on the MI355X at K = 3 over the five cases, three residual modes and two volumes of
tests/test_anomaly_ensemble_gpu.py: worst |err| / bound 0.450 without a grid, 0.168 with one; the witnesses at least 2.9 x 10^5.)  The witnesses of the tests are this reference computed wrongly: the scale inv_K left out (sum_k a_k), and the members'
weights rotated by one (e_k paired with w_{k+1}); the bound is then taken for the wrong reference, as tests/test_anomaly_gpu.py does for its own."""
import functools
import math

import numpy as np

import anomaly_bounds
import anomaly_ref

# the five cases of tests/test_anomaly_gpu.py: volume, latent grid (None: no weight grid), sigma
CASES = {"wide": ((24, 40, 16), (3, 5, 2), 4.0), "ragged": ((18, 14, 22), (9, 7, 11), 1.5), "beyond": ((8, 12, 20), (2, 3, 5), 8.0),
         "mixed": ((16, 8, 24), (2, 4, 3), 2.0), "plain": ((18, 14, 22), None, 0.0)}
MODES = ("abs", "positive", "negative")
MAX_MEMBERS = 16


@functools.lru_cache(maxsize=None)
def inputs(case):
    """x [2, D, H, W], r [16, 2, D, H, W] in [0, 1), m [16, 2, d, h, w] (None without a grid; even members carry {0, 1} masks, odd ones NLL-like grids in
    nats) and labels [2, D, H, W] bytes, seeded by the case; an ensemble of K members takes the first K"""
    shape, latent, _ = CASES[case]
    rng = np.random.default_rng(100 + sorted(CASES).index(case))
    x = rng.random((2, *shape), dtype=np.float32)
    r = rng.random((MAX_MEMBERS, 2, *shape), dtype=np.float32)
    m = None
    if latent is not None:
        mask = (rng.random((MAX_MEMBERS, 2, *latent)) < 0.4).astype(np.float32)
        nll = (rng.exponential(1.5, (MAX_MEMBERS, 2, *latent)) * (rng.random((MAX_MEMBERS, 2, *latent)) < 0.8)).astype(np.float32)
        m = np.where((np.arange(MAX_MEMBERS) % 2 == 0).reshape(-1, 1, 1, 1, 1), mask, nll)
    labels = (rng.random((2, *shape)) < np.array([0.3, 0.1]).reshape(2, 1, 1, 1)).astype(np.uint8)
    for a in (x, r, m, labels):
        if a is not None:
            a.setflags(write=False)
    return x, r, m, labels


def taps_of(case):
    from synthanatomy_amd.metrics.anomaly import gaussian_taps
    return gaussian_taps(CASES[case][2])


@functools.lru_cache(maxsize=None)
def member_weights(case, K):
    """w_k in fp64 per member and volume, [K][2] arrays (ones without a grid); shared by the residual modes"""
    shape, latent, _ = CASES[case]
    _, _, m, _ = inputs(case)
    if latent is None:
        return [[np.ones(shape)] * 2 for _ in range(K)]
    taps = taps_of(case)
    return [[anomaly_ref.weight_ref(m[k, b], shape, taps) for b in range(2)] for k in range(K)]


def chain(case):
    shape, latent, sigma = CASES[case]
    return anomaly_bounds.chain_length(shape, latent, math.ceil(3 * sigma))


def compose_fp32(maps):
    """the rule on K fp32 member maps: the sequential fp32 sum in member order times np.float32(1.0 / K)"""
    maps = [np.asarray(a) for a in maps]
    assert maps and all(a.dtype == np.float32 and a.shape == maps[0].shape for a in maps)
    s = maps[0].copy()
    for a in maps[1:]:
        s = s + a
    return s * np.float32(1.0 / len(maps))


def ensemble_ref(x, rs, ws, mode, scale=True, rotate=0):
    """fp64, one volume: (the mean over k of residual(x, r_k) w_{k + rotate}, the members' references a_k, their weights as paired).  ``scale`` = False
    and ``rotate`` = 1 are the witnesses."""
    K = len(rs)
    paired = [ws[(k + rotate) % K] for k in range(K)]
    a = [anomaly_ref.residual(x, rs[k], mode) * paired[k] for k in range(K)]
    total = np.sum(a, axis=0)
    return (total / K if scale else total), a, paired


def ensemble_bound(x, rs, a_refs, w_refs, c, scaled=True):
    """the docstring's bound for one volume (``scaled`` = False: for the witness without inv_K, the same chain without the division)"""
    K = len(rs)
    g = (K + 2) * anomaly_bounds.U / (1.0 - (K + 2) * anomaly_bounds.U)
    b = sum(anomaly_bounds.map_bound(a_refs[k], w_refs[k], x, rs[k], c) for k in range(K))
    total = (1.0 + g) * b + g * np.sum(a_refs, axis=0)
    return (total / K if scaled else total) + 2.0 ** -149


def worst_ratios(got, case, K, mode):
    """worst |err| / bound of an ensemble map ``got`` [2, D, H, W] over both volumes: against the rule, against the reference without inv_K and against
    the one with rotated weights"""
    x, r, _, _ = inputs(case)
    ws = member_weights(case, K)
    c = chain(case)
    out = []
    for scale, rotate in ((True, 0), (False, 0), (True, 1)):
        worst = 0.0
        for b in range(2):
            rs = [r[k, b] for k in range(K)]
            ref, a, paired = ensemble_ref(x[b], rs, [ws[k][b] for k in range(K)], mode, scale, rotate)
            worst = max(worst, anomaly_bounds.worst_ratio(got[b], ref, ensemble_bound(x[b], rs, a, paired, c, scale)))
        out.append(worst)
    return tuple(out)


def model_fp32(case, K, mode):
    """an fp32 numpy model of the rule, [2, D, H, W]: per member fl(residual of fl(x - r_k)) * fl(w_k) -- three roundings where the kernel's chain allows
    c + 1 -- composed with ``compose_fp32``"""
    x, r, _, _ = inputs(case)
    ws = member_weights(case, K)
    vols = []
    for b in range(2):
        maps = []
        for k in range(K):
            d = x[b] - r[k, b]
            e = {"abs": np.abs(d), "positive": np.maximum(d, np.float32(0)), "negative": np.maximum(-d, np.float32(0))}[mode]
            maps.append(e * ws[k][b].astype(np.float32) if CASES[case][1] is not None else e)
        vols.append(compose_fp32(maps))
    return np.stack(vols)
