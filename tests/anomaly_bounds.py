"""Element-wise fp32 error bound of sa_anomaly_map's map against tests/anomaly_ref.py (fp64), derived from the summation chain of csrc/anomaly.hip as
built.  u = 2^-24 is the unit roundoff of fp32; the library is compiled with -ffp-contract=off, so every rounding below is one the source
spells out.

The reference uses the kernel's own fp32 taps, the inputs are fp32 numbers, and every term of the weight is >= 0 (taps, mask / NLL cells), so each rounded
operation multiplies what it touches by some (1 + delta), |delta| <= u, and nothing cancels:

  band tables   A_X[p][c] = the taps of p's window inside cell c, added one by one in ascending order: n_X = min(f_X, 2R + 1) taps, n_X - 1 roundings
  W, H, D pass  s = fmaf(A, value, s) over the cells of the tile's neighbourhood; an entry outside the band is exactly 0 and fmaf(0, v, s) = s, so only
                the K_X <= min(2 ceil(R / f_X) + 1, cells_X) band entries round: K_X roundings on the longest path (the first fmaf rounds its product)
  a = e * w     1 rounding

  c = 1 + sum over X in (D, H, W) of (n_X - 1 + K_X)           (0 without a weight grid: a = e is the correctly rounded subtraction)

The subtraction e = fl(x - r) is correctly rounded: |e - e_ref| <= u |x - r| <= u max(|x|, |r|) for operands of one sign (the tests draw both from
[0, 1)); abs / max(., 0) are exact.  Together, with gamma_c = c u / (1 - c u) (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1):

  |a - a_ref| <= gamma_c a_ref + (1 + gamma_c) u max(|x|, |r|) w_ref + 2^-149

(the last term: one gradual-underflow step, never reached by the tests' magnitudes).

Measured on the MI355X over every case of tests/test_anomaly_gpu.py (five shapes, three residual modes, two volumes): worst |err| / bound 0.218
(16 x 8 x 24, factors 8, 2, 8, sigma 2, c = 25); the witnesses -- the cell boundary (p + 1) // f, taps left unnormalised -- exceed the bound at least
2 x 10^5 times over in every case that has a weight grid."""
import math

import numpy as np

U = 2.0 ** -24


def chain_length(shape, latent, R):
    """c of the docstring for volume ``shape`` (D, H, W), latent grid ``latent`` (d, h, w; None: no weight grid) and filter radius R"""
    if latent is None:
        return 0
    c = 1
    for n, cells in zip(shape, latent):
        f = n // cells
        c += min(f, 2 * R + 1) - 1 + min(2 * math.ceil(R / f) + 1, cells)
    return c


def map_bound(a_ref, w_ref, x, r, c):
    """the element-wise bound (fp64 array) for fp64 references a_ref, w_ref and fp32 inputs x, r"""
    gamma = c * U / (1.0 - c * U)
    big = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(r, dtype=np.float64)))
    return gamma * np.asarray(a_ref, dtype=np.float64) + (1.0 + gamma) * U * big * np.asarray(w_ref, dtype=np.float64) + 2.0 ** -149


def worst_ratio(a, a_ref, bound):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - a_ref) / bound))
