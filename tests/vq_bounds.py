"""Element-wise fp64 error bounds for the EMA vector quantizer (csrc/vq.hip: sa_vq_assign, sa_vq_ema_update, sa_vq_perplexity, sa_vq_backward,
sa_vq_embed; csrc/deterministic.hip: sa_vq_stats_det), the planted-defect witnesses that an output must fail, and an fp32 model of the kernels'
arithmetic (tests/test_vq_bounds_cpu.py holds the model to the same gate; tests/test_vq_bounds_gpu.py holds the kernels to it).

The operands are drawn in fp32, so the fp64 reference sees exactly the kernel's values and the only legitimate error is the kernel's own fp32
arithmetic (the library is built with -ffp-contract=off: every product and every sum the source writes rounds on its own).  U = 2^-24.

Distances and admissible codes.  For row m and code k, d64 = |x|^2 - 2 x.w + |w|^2 in fp64.  The kernel takes xx and wn as sequential D-term
chains of __fadd_rn(s, __fmul_rn(v, v)) (at most D roundings on any term), the dot product as D / 4 exact-f32 MFMA steps (a k-ordered fmaf chain:
D roundings), then d = __fadd_rn(__fsub_rn(xx, 2 acc), wn): one rounding of xx - 2 x.w and one of d.  To first order, times 1 + 2 (D + 2) U,

    delta(m, k) = U [ D (|x|^2 + 2 sum_j |x_j w_j| + |w|^2) + |xx - 2 x.w| + |d64| ]
    A(m) = { k : d64(m, k) - delta(m, k) <= min_k' (d64(m, k') + delta(m, k')) }          the admissible codes

and the returned index (a) lies in A(m), so where A(m) has one element it is that code, (b) is never a code whose row is bitwise equal to a
lower-indexed code's row (bitwise equal operands give bitwise equal distances: the first must win), (c) on the lattice cases -- integer operands
in {-2 .. 2}, every fp32 intermediate an integer below 16 D <= 8064 < 2^24, hence exact -- equals the first index of the minimum of the integer
distance.  An all-NaN row never passes `nd > best`: its index only has to lie in [0, K).

Statistics, CONDITIONAL ON THE INDICES THE KERNEL RETURNED (once the index is admissible every other output is referenced in fp64 from it, so a
flipped near-tie cannot hide a wrong statistic):

    counts  = bincount(idx) exactly (integers below 2^24)
    dw[k,j] within (15 + b_k + 2) U sum |x_mj| over the rows of code k; b_k = the 16-row blocks holding a row of k (the leader row's in-block sum,
            then one atomic per block in any order)
    zq_st   within U (|q - x| + |q|) (1 + 2 U) of q = W[idx]                         (__fadd_rn(__fsub_rn(q, x), x))
    zq_lp   bitwise the round-to-nearest-even bf16 of the zq_st that was returned
    sqerr   within (ceil(16 D / 256) + 6 + 4 + nblk + 4) U sum (q - x)^2: one thread's terms, the wave butterfly, the four waves, the blocks' atomics,
            and the roundings of (q - x) (twice through the square) and of the square
    sa_vq_stats_det: counts exact; dw within (n_k + 2) U sum |x_mj| (n_k = the code's own row count, the chain of block k); sqerr within
            sum_k (n_k ceil(D / 256) + 8 + ceil(K / 1024) + 10 + 4) U E_k, E_k = the code's own error sum.  CORRECTION to the issue's chain length n_k:
            thread t of block k owns dimensions t and t + 256 and adds BOTH passes into one register (`for j0 ...: e += ...`), so at D > 256 its chain
            is 2 n_k long.
A NaN row makes sqerr and the dw row of the code it chose NaN by construction; those two are not held to a bound in the NaN case, everything else is.

sa_vq_ema_update (g = decay, both as fp32 values; 1.f - g is exact for g in [0.5, 1] by Sterbenz; eps the fp32 value):
    N'      within 3 U (|N g| + |c (1 - g)|) =: dN
    n       = sum N' carries dn = sum dN + (ceil(K / 1024) + 6 + 16) U sum N'.  CORRECTION: the issue's chain term alone leaves out that the sum is
            taken over the ROUNDED N' (the kernel reads back what it stored), so their 3 U errors add.
    avg'    within 3 U (|avg g| + |dw (1 - g)|) =: da
    wn      = ((N' + eps) / (n + K eps)) n has relative error rw = dn / n + dN / (N' + eps) + dn / (n + K eps) + 5 U.  CORRECTION: five roundings, not
            four -- __fadd_rn(N', eps), __fmul_rn(K, eps), __fadd_rn(n, .), __fdiv_rn, __fmul_rn(., n).
    codebook within da / wn + |a / wn| (rw + 2 U) (1 + 2 rw): relative to |a / wn| wherever a does not cancel, and still relative for codes with
            N = counts = 0, where wn ~ eps n / (n + K eps)

sa_vq_perplexity: t = sum p log(p + 1e-10), p = counts / M.  The kernel's p is counts * (1.f / (float) M): two roundings, p^ = p (1 + 2 U);
    4 U per term for logf, the product and the term's own slack; the (ceil(K / 1024) + 22) U chain -- all on S = sum |p log(p + 1e-10)|:
        dt = (4 + 2 + ceil(K / 1024) + 22) U S + 3 U sum p
    CORRECTION: the issue charges the fp32 rounding of p + 1e-10f (and has no term for 1 / M) against |p log p|.  A relative perturbation eta of the
    ARGUMENT moves the logarithm by eta ABSOLUTELY, so the term moves by p eta, which |p log p| does not cover as p -> 1: with one count holding all
    of M, p + 1e-10f rounds to 1, the term is 0 against the reference's 1e-10, and S is 1e-10 itself.  eta <= 2 U (p^) + U (the sum's rounding), hence
    the 3 U sum p.  The output exp(-t) has relative error dt + 4 U.

sa_vq_backward: dz = g + gl (x - q), gl = g_loss * (beta * 2 / n).  beta * 2 and (float) n are exact; the quotient, gl, x - q and the product round once
    each, and the sum once more (no contraction): U |g| + 5 U |t| to first order.  The bound is 4 U |g| + 5 U |t| (1 + 4 U), t = g_l beta 2 / n (x - q).
    CORRECTION: 5 U on t where the issue has 4 U, which counts the product and the sum as one fused operation.  + half a bf16 ulp of the result
    for a bf16 dz; a bf16 g_zq enters exactly; g_zq = NULL is g = 0; g_loss = NULL returns g itself, bit for bit (g + 0 (x - q)).
sa_vq_embed: fp32 output bit-exact W[clamp(idx)], bf16 output its round-to-nearest-even rounding; indices -3 and K + 5 read rows 0 and K - 1.

A witness is the fp32 model with one planted defect; WITNESSES names the case each must fail the gate on.

Worst max |err| / bound per output over every case (the acceptance threshold is the bound itself, ratio <= 1; MEASURED below; the atomic path's
figures move in the last digit from run to run with the order of the atomics):
                       dw      zq_st   sqerr   det_dw  det_sqerr  ema_N   ema_avg  ema_cb  ppl     dz (f32 / bf16)
    fp32 model (CPU):  0.109   0.955   0.060   0.254   0.053      0.590   0.637    0.171   0.029   0.429 / 1.00
    MI355X kernels:    0.124   0.955   0.047   0.254   0.053      0.590   0.637    0.171   0.053   0.429 / 1.00
Every index of every case was admissible, first among bitwise twins, and on the lattice the first exact minimum, on the model and on the MI355X.
zq_st sits at 0.955: its bound is nothing but the unit roundoffs of its own two roundings, U |q - x| + U |q|, and one rounding reaches U |v| when
v lies just above a power of two; over the 10^5 elements of the cases some element comes close on both at once.  A bf16 dz sits at 1.00: the
output's own rounding is up to the half ulp that makes up nearly all of its bound.  The deterministic path's figures and the EMA's are the same
on the model and the kernels because their operation order is fixed and the model follows it.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import conv_bounds as cb

U = cb.U32
F32 = np.float32
EPS32 = float(np.float32(1e-5))
BIG = 0x7FFFFFFF

# worst max |err| / bound measured on the MI355X per output, over every case of tests/test_vq_bounds_gpu.py
MEASURED = dict(dw=0.124, zq_st=0.955, sqerr=0.0469, det_dw=0.254, det_sqerr=0.0529, ema_N=0.59, ema_avg=0.637, ema_cb=0.171, ppl=0.053,
                dz_f32=0.429, dz_bf16=1.0)


# ------------------------------------------------------------------------------------------------------------------------------ dispatch
def nv_for(D: int) -> int:
    """float4 pieces per lane and tile: the template argument sa_vq_assign picks"""
    for lim, nv in ((16, 1), (32, 2), (64, 4), (128, 8), (256, 16)):
        if D <= lim:
            return nv
    return 32


def trips(K: int) -> int:
    """loop trips of one wave: 16-code tiles wave, wave + 4, ..."""
    return ((K + 15) // 16 + 3) // 4


def lds_bytes(D: int) -> int:
    return (5 * 16 * (D + 4) + 16 + 64 + 64 + 16 + 4) * 4


LDS_LIMIT = 160 * 1024

# (M, K, D, kind)
CASES = [
    (2, 1, 4, "near"),            # K = 1: one code, three idle waves and fifteen idle lanes' slots; M = K + 1
    (1, 3, 4, "near"),            # M = 1: fifteen zero-filled rows in the only block
    (4, 3, 16, "near"),           # K = 3, D = 16: the NV = 1 boundary
    (17, 16, 20, "near"),         # K = 16: one full tile; D = 20: one float4 past NV = 1 (a lane's last register piece is partly empty); M = 17: a one-row block
    (18, 17, 32, "near"),         # K = 17: a one-code tile for wave 1; D = 32: the NV = 2 boundary
    (65, 64, 36, "near"),         # K = 64: one full tile per wave; D = 36: one float4 past NV = 2
    (66, 65, 64, "near"),         # K = 65: a second trip for wave 0 only; D = 64: the NV = 4 boundary
    (130, 129, 68, "near"),       # K = 129: three trips (first refill of va); D = 68: one float4 past NV = 4
    (258, 257, 128, "near"),      # K = 257: five trips (both buffers refilled), ragged last tile; D = 128: the NV = 8 boundary
    (33, 65, 132, "near"),        # D = 132: one float4 past NV = 8; M = 33
    (16, 129, 256, "near"),       # D = 256: the NV = 16 boundary; M = 16: exactly one block
    (15, 257, 260, "near"),       # D = 260: one float4 past NV = 16; M = 15: one ragged block
    (66, 65, 504, "near"),        # D = 504: the widest row the LDS rule admits (163 216 of 163 840 bytes)
    (1, 17, 504, "near"),         # the widest row with a single row and a one-code tile
    (17, 257, 64, "near"),        # five trips at M = 17
    (33, 2048, 32, "near"),       # K = 2048: 32 trips, the production codebook
    (33, 17, 20, "randn"),        # unrelated rows and codes
    (15, 64, 16, "randn"),
    (66, 65, 4, "lattice"),       # integer operands: every operation exact, ties plentiful
    (258, 257, 4, "lattice"),
    (258, 257, 20, "lattice"),
    (66, 65, 504, "lattice"),
    (33, 257, 504, "lattice"),
    (130, 129, 32, "ladder"),     # best-two gap 0 (bitwise duplicates at k and k + 64) or 8 delta
    (258, 257, 132, "ladder"),
    (83, 64, 32, "collapsed"),    # three codes in use, whole blocks on one code, ragged last block of 3 rows
    (33, 17, 20, "nan"),          # one all-NaN row among normal rows
]
NAN_ROW = 7
LADDER_DUPS = (1, 5, 17, 33, 50, 63)           # W[k + 64] = W[k]
LADDER_PAIRS = ((2, 3), (9, 25), (20, 84), (0, 128))      # 1, 16, 64 and 128 apart: one lane group, the next wave, the next trip, the other buffer
COLLAPSED_CODES = (5, 37, 60)

# (K, D, decay)
EMA_CASES = [(5, 4, 0.5), (300, 36, 0.99), (2051, 4, 0.99), (2051, 36, 0.5)]
# (K, kind)
PPL_CASES = [(1, "all"), (64, "zeros"), (2051, "random"), (64, "one")]
# (M, K, D)
BWD_CASES = [(100, 17, 8), (33, 65, 36)]

# witness -> the case it must fail on
WITNESSES = {
    "ties_last": (66, 65, 4, "lattice"),
    "drop_last_tile": (18, 17, 32, "near"),
    "pad_rows_counted": (17, 16, 20, "near"),
    "wnorm_next": (33, 17, 20, "randn"),
    "dw_block_missing": (66, 65, 64, "near"),
}
EMA_WITNESSES = {"old_N": (300, 36, 0.99), "no_eps": (300, 36, 0.99)}
PPL_WITNESSES = {"no_eps": (64, "zeros")}


def case_id(c) -> str:
    return "-".join(str(v) for v in c)


# ------------------------------------------------------------------------------------------------------------------------------ operands
def _rng(*key):
    return np.random.default_rng([sum(map(ord, k)) if isinstance(k, str) else int(k) for k in key])


def _randn(g, *shape):
    return g.standard_normal(shape, dtype=np.float32)


def draw(M: int, K: int, D: int, kind: str):
    """(x [M, D], W [K, D]) in fp32"""
    g = _rng(M, K, D, kind)
    if kind == "lattice":
        # every code is one base row with one coordinate of a small pool moved by +-1 (every third code: two coordinates), every row the base plus
        # +-1 noise of a density that cycles over the rows: d = |n|^2 - 2 n.p + |p|^2 takes a handful of values, so each row's minimum is shared by
        # codes all over the codebook, bitwise twins and distinct rows alike
        P = min(D, 16)
        base = g.integers(-1, 2, D)
        pool = g.permutation(D)[:P]
        W = np.repeat(base[None], K, 0)
        j1 = g.integers(0, P, K)
        W[np.arange(K), pool[j1]] += g.choice([-1, 1], K)
        two = np.arange(K) % 3 == 2
        j2 = (j1 + 1 + g.integers(0, P - 1, K)) % P
        W[np.arange(K)[two], pool[j2[two]]] += g.choice([-1, 1], int(two.sum()))
        dens = np.array([0.05, 0.2, 0.6])[np.arange(M) % 3][:, None]
        noise = g.integers(-1, 2, (M, D)) * (g.random((M, D)) < dens)
        x = np.clip(base[None] + noise, -2, 2)
        return x.astype(F32), W.astype(F32)
    W = _randn(g, K, D)
    if kind == "randn":
        return _randn(g, M, D), W
    if kind in ("near", "nan"):
        x = W[np.arange(M) % K] + F32(0.3) * _randn(g, M, D)
        if kind == "nan":
            x[NAN_ROW] = np.nan
        return x.astype(F32), W
    if kind == "collapsed":
        W = W * F32(10.0)
        which = g.integers(0, 3, M)
        which[:32] = 0              # two whole blocks on one code
        which[32:48] = 1            # and a third on another
        x = W[np.array(COLLAPSED_CODES)[which]] + F32(0.01) * _randn(g, M, D)
        return x.astype(F32), W
    assert kind == "ladder"
    for k in LADDER_DUPS:
        W[k + 64] = W[k]
    for a, b in LADDER_PAIRS:                                     # two codes half a noise unit apart: the two nearest of any row between them
        W[b] = W[a] + F32(0.5) * _randn(g, D)
    x = np.empty((M, D), dtype=F32)
    W64 = W.astype(np.float64)
    for m in range(M):
        if m % 2 == 0:                                            # gap 0: next to a duplicated code
            k = LADDER_DUPS[(m // 2) % len(LADDER_DUPS)]
            x[m] = W[k] + F32(0.05) * _randn(g, D)
        else:                                                     # gap 8 delta: between two codes, the winner alternately the lower and the higher
            a, b = LADDER_PAIRS[(m // 2) % len(LADDER_PAIRS)]
            if (m // 2 // len(LADDER_PAIRS)) % 2:
                a, b = b, a
            u = W64[a] - W64[b]
            x0 = 0.5 * (W64[a] + W64[b]) + 0.05 * g.standard_normal(D)
            dl = _delta_terms(x0[None], W64[[a]], D)[1][0, 0]
            gap0 = ((x0 - W64[b]) ** 2).sum() - ((x0 - W64[a]) ** 2).sum()
            x[m] = (x0 + ((8.0 * dl - gap0) / (2 * (u @ u))) * u).astype(F32)      # d(b) - d(a) moves by 2 s |u|^2 to 8 delta
    return x, W


def draw_ema(K: int, D: int, decay: float):
    g = _rng(K, D, int(decay * 100), "ema")
    counts = g.integers(1, 40, K).astype(F32)
    N = (g.random(K, dtype=np.float32) * F32(30.0)).astype(F32)
    idle = np.arange(K) % 5 == 2                                  # a fifth of the codes drew no row this step ...
    counts[idle] = 0
    N[idle & (np.arange(K) % 10 == 2)] = 0                        # ... and half of those never have
    avg = (_randn(g, K, D) * N[:, None]).astype(F32)
    dw = (_randn(g, K, D) * counts[:, None]).astype(F32)
    return dict(N=N, avg=avg, counts=counts, dw=dw, decay=float(F32(decay)), eps=EPS32)


def draw_ppl(K: int, kind: str):
    g = _rng(K, kind, "ppl")
    if kind == "all":
        counts = np.array([1006], dtype=F32)
    elif kind == "one":
        counts = np.zeros(K, dtype=F32)
        counts[K // 3] = 1006
    else:
        counts = g.integers(0, 50, K).astype(F32)
        if kind == "zeros":
            counts[::3] = 0
    return counts, int(counts.sum())


# ------------------------------------------------------------------------------------------------------------------------------ reference
def _delta_terms(x, W, D):
    """(d64, delta) of fp64 rows x [M, D] against fp64 codes W [K, D]"""
    xx = (x * x).sum(1)[:, None]
    ww = (W * W).sum(1)[None, :]
    xw = x @ W.T
    d64 = ((x[:, None, :] - W[None, :, :]) ** 2).sum(2) if x.shape[0] * W.shape[0] * D <= 4_000_000 else xx - 2 * xw + ww     # (the same number)
    axw = np.abs(x) @ np.abs(W).T
    delta = U * (D * (xx + 2 * axw + ww) + np.abs(xx - 2 * xw) + np.abs(d64)) * (1 + 2 * (D + 2) * U)
    return d64, delta


class Ref:
    """what the fp64 reference says about one (x, W) before any output is seen"""

    def __init__(self, x, W, kind: str):
        self.x32, self.W32, self.kind = x, W, kind
        self.x, self.W = x.astype(np.float64), W.astype(np.float64)
        self.M, self.D = x.shape
        self.K = W.shape[0]
        self.nanrow = np.isnan(x).any(1)
        with np.errstate(invalid="ignore"):
            self.d64, self.delta = _delta_terms(self.x, self.W, self.D)
            self.adm = (self.d64 - self.delta) <= (self.d64 + self.delta).min(1, keepdims=True)           # [M, K]; all False on a NaN row
        _, first, inv = np.unique(np.ascontiguousarray(W).view(np.uint32), axis=0, return_index=True, return_inverse=True)
        self.canon = first[inv.reshape(-1)]                                                              # the first code with bitwise this row
        self.nadm = self.adm.sum(1)
        self.sole = np.where(self.nadm == 1, self.adm.argmax(1), -1)
        self.first_min = np.where(self.nanrow, 0, np.nan_to_num(self.d64, nan=np.inf).argmin(1))         # lattice: exact

    def lattice_exact(self) -> bool:
        ok = np.array_equal(self.x, np.rint(self.x)) and np.array_equal(self.W, np.rint(self.W))
        return ok and np.abs(self.x).max() <= 2 and np.abs(self.W).max() <= 2 and 16 * self.D < 2 ** 24

    def tie_offsets(self):
        """(k - k0, same 4-code lane group, same tile) over every row and every further minimiser k of the row's integer distance, k0 the first"""
        mn = self.d64.min(1, keepdims=True)
        m, k = np.nonzero(self.d64 == mn)
        k0 = self.first_min[m]
        keep = k > k0
        k, k0 = k[keep], k0[keep]
        return k - k0, (k // 4 == k0 // 4), (k // 16 == k0 // 16)


@functools.lru_cache(maxsize=None)
def case(c):
    """(x, W, Ref) of one row of CASES: drawn and referenced once, shared by every test, never written to"""
    x, W = draw(*c)
    x.setflags(write=False)
    W.setflags(write=False)
    return x, W, Ref(x, W, c[3])


def bf16_rne(a):
    """fp32 array rounded to nearest even bf16, held as fp32 (NaN stays NaN)"""
    return torch.tensor(np.asarray(a, dtype=F32)).to(torch.bfloat16).float().numpy()


def half_ulp_bf16(mag):
    return cb.half_ulp(torch.from_numpy(np.asarray(mag, dtype=np.float64)), "bf16").numpy()


def _ratio(err, bnd):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err <= bnd, err / np.maximum(bnd, 1e-300), np.inf)      # (NaN fails)
    return float(np.max(r)) if r.size else 0.0


def _note(ratios, key, r):
    if ratios is not None and np.isfinite(r):
        ratios[key] = max(ratios.get(key, 0.0), r)


def gate_index(ref: Ref, idx):
    """failures of the returned indices against the admissible sets (a list of strings; empty = passes)"""
    fails = []
    idx = np.asarray(idx).astype(np.int64)
    if idx.shape != (ref.M,) or idx.min() < 0 or idx.max() >= ref.K:
        return [f"idx out of [0, {ref.K}) or of shape {idx.shape}"]
    ok = ref.adm[np.arange(ref.M), idx] | ref.nanrow
    if not ok.all():
        m = int(np.nonzero(~ok)[0][0])
        fails.append(f"{int((~ok).sum())} rows with an inadmissible code; row {m}: got {idx[m]} (d64 {ref.d64[m, idx[m]]:.9g} +- {ref.delta[m, idx[m]]:.3g}), "
                     f"nearest {int(ref.d64[m].argmin())} (d64 {ref.d64[m].min():.9g})")
    dup = (ref.canon[idx] != idx) & ~ref.nanrow
    if dup.any():
        m = int(np.nonzero(dup)[0][0])
        fails.append(f"{int(dup.sum())} rows took a later bitwise duplicate; row {m}: got {idx[m]}, the same row of W stands at {ref.canon[idx[m]]}")
    if ref.kind == "lattice" and not np.array_equal(idx, ref.first_min):
        m = int(np.nonzero(idx != ref.first_min)[0][0])
        fails.append(f"lattice: {int((idx != ref.first_min).sum())} rows differ from the first index of the exact minimum; row {m}: got {idx[m]}, first {ref.first_min[m]}")
    return fails


def _blocks_per_code(idx, K):
    pairs = np.unique(np.stack([idx, np.arange(idx.size) // 16], 1), axis=0)
    return np.bincount(pairs[:, 0], minlength=K)


def gate_stats(ref: Ref, idx, counts, dw, sq, det: bool, ratios=None, pre="") -> list:
    """counts / dw / sqerr against the fp64 statistics of the RETURNED indices (atomic path: det = False; sa_vq_stats_det: det = True)"""
    fails = []
    idx = np.asarray(idx).astype(np.int64)
    M, K, D = ref.M, ref.K, ref.D
    n_k = np.bincount(idx, minlength=K)
    if not np.array_equal(np.asarray(counts, dtype=np.float64), n_k.astype(np.float64)):
        fails.append(f"{pre}counts differ from bincount(idx) (sum {float(np.sum(counts))} of {M} rows)")
    sdw, sab = np.zeros((K, D)), np.zeros((K, D))
    np.add.at(sdw, idx, ref.x)
    np.add.at(sab, idx, np.abs(ref.x))
    chain = n_k if det else 15 + _blocks_per_code(idx, K)
    bdw = (chain + 2)[:, None] * U * sab
    clean = np.ones(K, dtype=bool)
    clean[idx[ref.nanrow]] = False                       # the dw row of the code a NaN row chose is NaN by construction
    r = _ratio(np.abs(np.asarray(dw, dtype=np.float64) - sdw)[clean], bdw[clean])
    _note(ratios, pre + "dw", r)
    if not r <= 1.0:
        fails.append(f"{pre}dw: max |err| / bound = {r:.3g}")
    if not ref.nanrow.any():
        e_m = ((ref.W[idx] - ref.x) ** 2).sum(1)
        if det:
            E_k = np.bincount(idx, weights=e_m, minlength=K)
            bsq = float((((n_k * -(-D // 256)) + 8 + -(-K // 1024) + 10 + 4) * U * E_k).sum())
        else:
            bsq = (-(-16 * D // 256) + 6 + 4 + -(-M // 16) + 4) * U * float(e_m.sum())
        r = _ratio(np.abs(np.float64(sq) - e_m.sum()), np.float64(bsq))
        _note(ratios, pre + "sqerr", r)
        if not r <= 1.0:
            fails.append(f"{pre}sqerr: |err| / bound = {r:.3g} (got {float(sq):.9g}, fp64 {e_m.sum():.9g})")
    return fails


def gate_assign(ref: Ref, got: dict, ratios=None) -> list:
    """every output of one sa_vq_assign call: got = dict(idx, zq, zq_lp (fp32 values of the bf16 output, or None), counts, dw, sq)"""
    fails = gate_index(ref, got["idx"])
    if fails and fails[0].startswith("idx out of"):
        return fails
    idx = np.asarray(got["idx"]).astype(np.int64)
    fails += gate_stats(ref, idx, got["counts"], got["dw"], got["sq"], False, ratios)
    q = ref.W[idx]
    ok = ~ref.nanrow
    bzq = U * (np.abs(q - ref.x) + np.abs(q)) * (1 + 2 * U)
    zq = np.asarray(got["zq"])
    r = _ratio(np.abs(zq.astype(np.float64) - q)[ok], bzq[ok])
    _note(ratios, "zq_st", r)
    if not r <= 1.0:
        fails.append(f"zq_st: max |err| / bound = {r:.3g}")
    if not np.isnan(zq[~ok]).all():
        fails.append("zq_st of a NaN row is not NaN")
    if got.get("zq_lp") is not None:
        lp, want = np.asarray(got["zq_lp"], dtype=F32), bf16_rne(zq)
        same = (lp.view(np.uint32) == want.view(np.uint32)) | (np.isnan(lp) & np.isnan(want))
        if not same.all():
            fails.append(f"zq_lp: {int((~same).sum())} elements are not the round-to-nearest-even bf16 of zq_st")
    return fails


# ------------------------------------------------------------------------------------------------------------------------------ EMA, perplexity
def ema_ref(o, defect=None):
    """(N', avg', codebook) in fp64 with their bounds"""
    N, avg, c, dw = (o[k].astype(np.float64) for k in ("N", "avg", "counts", "dw"))
    g, eps = o["decay"], o["eps"]
    K, D = avg.shape
    N1 = N * g + c * (1 - g)
    dN = 3 * U * (np.abs(N * g) + np.abs(c * (1 - g)))
    n = N1.sum()
    dn = dN.sum() + (-(-K // 1024) + 6 + 16) * U * np.abs(N1).sum()
    a = avg * g + dw * (1 - g)
    da = 3 * U * (np.abs(avg * g) + np.abs(dw * (1 - g)))
    if defect == "no_eps":
        eps = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        wn = ((N if defect == "old_N" else N1) + eps) / (n + K * eps) * n
        rw = dn / n + dN / (N1 + eps) + dn / (n + K * eps) + 5 * U
        cbk = a / wn[:, None]
        bcb = da / wn[:, None] + np.abs(cbk) * ((rw + 2 * U) * (1 + 2 * rw))[:, None]
    return (N1, dN + 1e-300), (a, da + 1e-300), (cbk, bcb + 1e-300)


def gate_ema(o, got, ratios=None) -> list:
    fails = []
    for name, g, (r64, bnd) in zip(("ema_N", "ema_avg", "ema_cb"), got, ema_ref(o)):
        r = _ratio(np.abs(np.asarray(g, dtype=np.float64) - r64), bnd)
        _note(ratios, name, r)
        if not r <= 1.0:
            fails.append(f"{name}: max |err| / bound = {r:.3g}")
    return fails


def ppl_ref(counts, M):
    c = counts.astype(np.float64)
    K = c.size
    p = c / M
    term = p * np.log(p + 1e-10)
    S = np.abs(term).sum()
    dt = (4 + 2 + -(-K // 1024) + 22) * U * S + 3 * U * p.sum()
    ppl = np.exp(-term.sum())
    return ppl, ppl * (dt + 4 * U) * (1 + 2 * (dt + 4 * U))


def gate_ppl(counts, M, got, ratios=None) -> list:
    ppl, bnd = ppl_ref(counts, M)
    r = _ratio(np.abs(np.float64(got) - ppl), np.float64(bnd))
    _note(ratios, "ppl", r)
    return [] if r <= 1.0 else [f"perplexity: |err| / bound = {r:.3g} (got {float(got):.9g}, fp64 {ppl:.9g})"]


# ------------------------------------------------------------------------------------------------------------------------------ backward, embed
def draw_bwd(M, K, D, g_dt):
    """rows, codebook, idx, g (exact in g_dt), g_loss"""
    g = _rng(M, K, D, "bwd")
    x, W = _randn(g, M, D), _randn(g, K, D)
    idx = g.integers(0, K, M)
    gz = cb.rounded(torch.from_numpy(_randn(g, M, D)), g_dt).numpy()
    return dict(x=x, W=W, idx=idx, g=gz, gl=np.array([0.7], dtype=F32), beta=float(F32(0.25)))


def bwd_ref(o, use_g: bool, use_gl: bool, out_dt: str):
    x, W, g = o["x"].astype(np.float64), o["W"].astype(np.float64), o["g"].astype(np.float64)
    t = (float(o["gl"][0]) * o["beta"] * 2.0 / x.size) * (x - W[o["idx"]]) if use_gl else np.zeros_like(x)
    gg = g if use_g else np.zeros_like(x)
    ref = gg + t
    slack = 4 * U * np.abs(gg) + 5 * U * np.abs(t) * (1 + 4 * U)
    if out_dt == "bf16":
        slack = slack + half_ulp_bf16(np.abs(ref) + slack)
    return ref, slack + 1e-300


def gate_bwd(o, use_g, use_gl, out_dt, got, ratios=None) -> list:
    got = np.asarray(got, dtype=F32)
    if not use_gl:                          # g + 0 (x - q): g itself (rounded once to a bf16 output)
        want = o["g"] if use_g else np.zeros_like(o["x"])
        want = bf16_rne(want) if out_dt == "bf16" else want
        return [] if np.array_equal(got, want) else [f"dz without g_loss is not g bit for bit ({int((got != want).sum())} elements)"]
    ref, bnd = bwd_ref(o, use_g, use_gl, out_dt)
    r = _ratio(np.abs(got.astype(np.float64) - ref), bnd)
    _note(ratios, "dz_" + out_dt, r)
    return [] if r <= 1.0 else [f"dz ({out_dt}): max |err| / bound = {r:.3g}"]


def embed_ref(W, idx, out_dt):
    e = W[np.clip(idx, 0, W.shape[0] - 1)]
    return bf16_rne(e) if out_dt == "bf16" else e


# ------------------------------------------------------------------------------------------------------------------------------ fp32 model
def _chain_sq32(v):
    """sum_j v_j^2 as the kernels' __fadd_rn(s, __fmul_rn(v, v)) chain, per row"""
    s = np.zeros(v.shape[0], dtype=F32)
    for j in range(v.shape[1]):
        s = s + v[:, j] * v[:, j]
    return s


def _wave_sum32(v):
    """wave_sum over the last axis (64 lanes): the xor butterfly, every lane ends with the same tree"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def model_index(x, W, defect=None):
    """the indices of vq_assign_kernel for rows x padded to whole blocks with zeros: (idx of all 16 nblk rows, the padded rows)"""
    M, D = x.shape
    K = W.shape[0]
    Mp = -(-M // 16) * 16
    xp = np.zeros((Mp, D), dtype=F32)
    xp[:M] = x
    with np.errstate(invalid="ignore", over="ignore"):
        xx, wn = _chain_sq32(xp), _chain_sq32(W)
        if defect == "wnorm_next":
            wn = np.roll(wn, -1)
        acc = np.zeros((Mp, K), dtype=F32)
        for j in range(D):                 # the MFMA's k-ordered fmaf chain: the product is exact in fp64, one rounding per step (fp64-emulated fma)
            acc = (W[None, :, j].astype(np.float64) * xp[:, j:j + 1].astype(np.float64) + acc.astype(np.float64)).astype(F32)
        d = (xx[:, None] - F32(2.0) * acc) + wn[None, :]
        nd = -d
    it = trips(K)
    ndp = np.full((Mp, it * 64), -np.inf, dtype=F32)
    ndp[:, :K] = np.where(np.isnan(nd), -np.inf, nd)           # `nd > best` is false for a NaN
    if defect == "drop_last_tile" and K % 16:
        ndp[:, (K // 16) * 16:] = -np.inf
    # code = (it * 4 + wave) * 16 + fq * 4 + r: a (wave, lane group) slot meets its codes in (it, r) order and keeps the FIRST maximum (strict >)
    v = ndp.reshape(Mp, it, 4, 4, 4).transpose(0, 2, 3, 1, 4).reshape(Mp, 16, it * 4)
    code = np.arange(it * 64).reshape(it, 4, 4, 4).transpose(1, 2, 0, 3).reshape(16, it * 4)
    last = defect == "ties_last"
    pos = (it * 4 - 1 - v[..., ::-1].argmax(2)) if last else v.argmax(2)
    best = np.take_along_axis(v, pos[..., None], 2)[..., 0]
    bidx = np.where(best > -np.inf, code[np.arange(16)[None, :], pos], -1 if last else BIG)
    # the shuffle and LDS reductions: greater value, then lower index -- a total order, so the pairwise tree returns its maximum
    top = best.max(1, keepdims=True)
    idx = np.where(best == top, bidx, -1).max(1) if last else np.where(best == top, bidx, BIG).min(1)
    idx = np.where((idx < 0) | (idx >= K), 0, idx)
    return idx.astype(np.int64), xp


def model_assign(x, W, defect=None, lp: bool = True):
    """sa_vq_assign in fp32 numpy arithmetic, operation by operation"""
    M, D = x.shape
    K = W.shape[0]
    idxp, xp = model_index(x, W, defect)
    nblk = xp.shape[0] // 16
    counts, dw, sq = np.zeros(K, dtype=F32), np.zeros((K, D), dtype=F32), F32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        q = W[idxp[:M]]
        dqx = q - x
        zq = dqx + x
        for b in range(nblk):
            nv = min(16, M - b * 16)
            fin = idxp[b * 16:b * 16 + 16]
            nc = 16 if defect == "pad_rows_counted" else nv
            for r in range(nc):
                same = [r2 for r2 in range(nc) if fin[r2] == fin[r]]
                if same[0] == r:
                    counts[fin[r]] += F32(len(same))
            for r in range(nv):
                same = [r2 for r2 in range(nv) if fin[r2] == fin[r]]
                if same[0] == r and not (defect == "dw_block_missing" and b == nblk - 1):
                    acc = xp[b * 16 + r].copy()
                    for r2 in same[1:]:
                        acc = acc + xp[b * 16 + r2]
                    dw[fin[r]] = dw[fin[r]] + acc
            e = np.zeros(-(-16 * D // 256) * 256, dtype=F32)
            e[:nv * D] = (dqx[b * 16:b * 16 + nv] * dqx[b * 16:b * 16 + nv]).ravel()
            err = np.zeros(256, dtype=F32)
            for chunk in e.reshape(-1, 256):
                err = err + chunk
            w = _wave_sum32(err.reshape(4, 64))
            sq = sq + (((w[0] + w[1]) + w[2]) + w[3])
    return dict(idx=idxp[:M], zq=zq, zq_lp=bf16_rne(zq) if lp else None, counts=counts, dw=dw, sq=sq)


def _tree32(red):
    red = red.copy()
    o = red.size // 2
    while o:
        red[:o] = red[:o] + red[o:2 * o]
        o //= 2
    return red[0]


def model_stats_det(x, W, idx):
    """sa_vq_stats_det: block k walks the rows in order; thread t owns dimensions t, t + 256 and one error register; fixed trees"""
    M, D = x.shape
    K = W.shape[0]
    counts, dw, err = np.zeros(K, dtype=F32), np.zeros((K, D), dtype=F32), np.zeros(K, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            rows = np.nonzero(idx == k)[0]
            counts[k] = F32(rows.size)
            e = np.zeros(256, dtype=F32)
            for j0 in range(0, D, 256):
                j1 = min(D, j0 + 256)
                for i in rows:
                    dw[k, j0:j1] = dw[k, j0:j1] + x[i, j0:j1]
                    t = W[k, j0:j1] - x[i, j0:j1]
                    e[:j1 - j0] = e[:j1 - j0] + t * t
            err[k] = _tree32(e)
        pad = np.zeros(-(-K // 1024) * 1024, dtype=F32)
        pad[:K] = err
        s = np.zeros(1024, dtype=F32)
        for chunk in pad.reshape(-1, 1024):
            s = s + chunk
        sq = _tree32(s)
    return counts, dw, sq


def _block_sum32(v):
    """one 1024-thread block's sum of v: thread t adds v[t], v[t + 1024], ...; wave butterflies; thread 0 adds the 16 wave sums in order"""
    pad = np.zeros(-(-v.size // 1024) * 1024, dtype=F32)
    pad[:v.size] = v
    s = np.zeros(1024, dtype=F32)
    for chunk in pad.reshape(-1, 1024):
        s = s + chunk
    w = _wave_sum32(s.reshape(16, 64))
    t = F32(0.0)
    for i in range(16):
        t = t + w[i]
    return t


def model_ema(o, defect=None):
    """sa_vq_ema_update: (N', avg', codebook)"""
    N, avg, c, dw = o["N"], o["avg"], o["counts"], o["dw"]
    g, eps = F32(o["decay"]), F32(0.0 if defect == "no_eps" else o["eps"])
    K = N.size
    omd = F32(1.0) - g
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        N1 = N * g + c * omd
        n = _block_sum32(N1)
        denom = n + F32(K) * eps
        wn = (((N if defect == "old_N" else N1) + eps) / denom) * n
        a = avg * g + dw * omd
        return N1, a, a / wn[:, None]


def model_ppl(counts, M, defect=None):
    with np.errstate(divide="ignore", invalid="ignore"):
        p = counts * (F32(1.0) / F32(M))
        term = p * np.log(p + F32(0.0 if defect == "no_eps" else 1e-10))
        return np.exp(-_block_sum32(term.astype(F32)))


def model_bwd(o, use_g, use_gl, out_dt):
    x, W = o["x"], o["W"]
    coef = (F32(o["beta"]) * F32(2.0)) / F32(x.size)
    gl = o["gl"][0] * coef if use_gl else F32(0.0)
    v = (o["g"] if use_g else np.zeros_like(x)) + gl * (x - W[o["idx"]])
    return bf16_rne(v) if out_dt == "bf16" else v
