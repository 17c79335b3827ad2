"""Element-wise fp64 error bounds for the Performer's LayerNorm (csrc/performer.hip: sa_layernorm_fwd, sa_layernorm_bwd; csrc/deterministic.hip:
sa_layernorm_dwprod + sa_colsum_det) and cross-entropy (csrc/performer.hip: sa_cross_entropy; csrc/deterministic.hip: sa_cross_entropy_rows +
sa_sum_det), the planted-defect witnesses that an output must fail, and an fp32 model of the kernels' arithmetic (tests/test_head_bounds_cpu.py
holds the model to the same bounds; tests/test_head_bounds_gpu.py holds the kernels to them).  The checks are norm_bounds.check / assert_within.

The inputs are drawn in fp32 on the CPU, so the fp64 reference sees exactly the kernel's operands and the only legitimate error is the kernel's
own fp32 arithmetic (and the final rounding of a 16-bit output).  U = 2^-24 is one fp32 rounding; a sum carries G = L * U, where L is the longest
chain of fp32 additions it goes through, restated from the launch rules (wave_chain, ln_col_rule, ce_loss_rule below):

    a wave's row sum over n columns      L = ceil(n / 64) + 6                one lane's stride-64 columns, then the six butterfly levels of wave_sum
    ce_kernel's loss                     L = 8 + ceil(R / 8)                 the eight LDS terms of a block, then one atomic per block in ANY order
    sum_det_kernel over n values         L = ceil(n / 1024) + 10             one thread's stride-1024 values, then the ten levels of the fixed tree
    layernorm_bwd_rows_kernel dw / db    L = 8 + 2 + ceil(R / 32)            a wave's eight rows, the four waves in pairs, one atomic per block
    layernorm_bwd_kernel dw / db         L = R                               one atomic per row and column
    sa_colsum_det                        L = ceil(rpb / 4) + 2 + nblk        rpb = ceil(R / 256), nblk = ceil(R / rpb): a row lane, the four lanes, the blocks

expf, logf and rsqrtf are allowed E = 2 (a relative error of E * U = 2^-23: one ulp at the bottom of a binade, two at its top); the build has
-ffp-contract=off and no fast-math.  TINY = 2^-126 is the absolute floor of a result below the smallest normal (flushed or denormal).

LayerNorm forward, with a1 = mean |x| and mu, var, rstd the fp64 row statistics (the kernel is two-pass: a mean that is off by d shifts the
centred sum of squares by d^2 exactly, so there is no mu^2 / var widening -- the model confirms it at 30 sigma row means):

    dmu   = G a1 + 2 U |mu|
    dvar  = (G + 4 U) var + dmu^2
    drstd = rstd (dvar / (2 (var + eps)) + (E + 2) U)
    dy    = |w| (rstd dmu + |x - mu| drstd) + 4 U (|x - mu| rstd |w| + |b|)
    stats[2 r], stats[2 r + 1]: dmu, drstd.  y_lp: EQUAL to the kernel's own fp32 y rounded once to nearest even (no bound).

LayerNorm backward, from the fp32 stats the kernel is given (bounded in isolation from the forward), g = dy w, s1 = mean g, s2 = mean g xhat:

    ds1 = (G + U) mean |g|        ds2 = (G + 4 U) mean |g xhat|          (the roundings of g, xhat and their product inside the sums)
    dx  = rstd (ds1 + |xhat| ds2 + 6 U (|g| + |s1| + |xhat| |s2|))       norm_bounds.backward_bounds with M -> C, the row-sum G, w inside g
    dw  = (G_col + 4 U) sum |dy xhat| + 2 U (|dw0| + |sum dy xhat|) + A U |dw0|
    db  = G_col sum |dy| + 2 U (|db0| + |sum dy|) + A U |db0|

Cross-entropy, with m the row maximum, s = sum exp(l - m), p the softmax, t the target:

    ds / s = G + E U + U sum_c p_c |l_c - m| + V TINY
    dlse   = ds / s + E U |log s| + U |lse|
    dterm  = dlse + U |lse - l_t|
    dloss  = sum dterm + G_loss sum |term| + A U |loss0|
    dgrad  = gscale p_c (U |l_c - lse| + dlse + E U) + 2 U |grad_c| + TINY      (+ half an ulp of a 16-bit gradient)
    target -100: term 0, gradient row 0.  Any other target outside [0, V): term NaN, gradient row 0.  A logit of -inf: p = gradient = 0.  All exact.

Terms that differ from the derivation this work started from, and why:
  * dterm had a further U (|lse| + |l_t|).  lse - l[t] is ONE subtraction of the computed lse (whose own final rounding U |lse| is already in dlse)
    and an exact operand: its only new error is U |lse - l_t|.  Dropped; at the +100 offset this is most of what the row loss was allowed.
  * A U |acc0| (dw0, db0, loss0) is new: the atomic routes add their A block partials (A = ceil(R / 32), R, ceil(R / 8)) ONTO the accumulator, so
    its pre-existing content goes through A roundings, not the two of 2 U |dw0|.  (The fixed-order routes add once: A = 0.)
  * ds1 has G + U for the rounding of g = dy w inside the sum (BatchNorm's g is an operand).
  * V TINY and TINY: at the peaked case p underflows in fp32 (l_c - lse < -87) where the fp64 p is 1e-40 .. 1e-90: no relative bound can hold there.

A witness is asserted to fail wherever its planted defect leaves the bound of the truth on at least one element; where it does not, no output
could tell the two apart: printed, not asserted (decided from the two references alone).  WITNESSES lists them; tests/test_head_bounds_cpu.py
fails unless each is asserted in at least one case.

Worst max |err| / bound over every case (the acceptance threshold is the bound itself, ratio <= 1; MEASURED below; the atomic routes' figures move
in the last digit from run to run with the order of the atomics):
                        LayerNorm: mean   rstd    y       dx      dw      db        cross-entropy: row_loss  loss    grad    grad (bf16)
    fp32 model (CPU):              0.128  0.261   0.272   0.393   0.182   0.180                    0.495     0.115   0.601   0.999
    MI355X kernels:                0.128  0.231   0.230   0.393   0.167   0.218                    0.495     0.120   0.605   0.999
A bf16 gradient sits at 1.00 (0.999): the output's own rounding is up to the half ulp that makes up nearly all of its bound.  y_lp (bf16 and f16)
equals the kernel's y rounded once on every element of every case.
"""
from __future__ import annotations

import numpy as np
import torch

import conv_bounds as cb
import norm_bounds as nb

U = cb.U32
E = 2.0                                  # expf, logf, rsqrtf: relative error E * U
TINY = 2.0 ** -126
EPS32 = float(np.float32(1e-5))          # nn.LayerNorm's default, as the c_float the kernel gets

# worst max |err| / bound measured on the MI355X per output, over every case of tests/test_head_bounds_gpu.py
MEASURED = dict(ln=dict(mean=0.128, rstd=0.231, y=0.23, dx=0.393, dw=0.167, db=0.218), ce=dict(row_loss=0.495, loss=0.12, grad=0.605, grad_bf16=0.999))

# (R, C, row-mean offset in sigma, x scale): C < 64 and a ragged last forward block in which three waves have no row; three column strides, the last
# ragged; all eight register slots of the rows kernel at 30 sigma means; the first C of the per-element backward; var ~ 1e-4 so that eps shows;
# 129 row blocks of atomics and rpb = 17 in the fixed-order column sum
LN_CASES = [
    (37, 32, 0.3, 2.0),
    (70, 200, 0.0, 1.0),
    (33, 512, 30.0, 1.0),
    (9, 513, 0.0, 1.0),
    (70, 200, 0.0, 0.01),
    (4100, 64, 0.0, 1.0),
]
# (R, V, logit scale, offset): V < 64; exactly one stride; one column in the second stride (row 5 carries two -inf logits); the product's V, 33
# strides; the same with a peaked softmax; an offset at which an unshifted exp overflows and lse - l_t cancels; nine blocks of atomics.
# Every case plants one -100 target; (10, 7) also runs with the targets V and -1 planted.
CE_CASES = [
    (10, 7, 1.0, 0.0),
    (17, 64, 1.0, 0.0),
    (8, 65, 1.0, 0.0),
    (9, 2049, 1.0, 0.0),
    (9, 2049, 30.0, 0.0),
    (13, 130, 1.0, 100.0),
    (70, 130, 1.0, 0.0),
]
LN_IDS = [f"{R}x{C}-off{off:g}-x{sc:g}" for (R, C, off, sc) in LN_CASES]
CE_IDS = [f"{R}x{V}-x{sc:g}-off{off:g}" for (R, V, sc, off) in CE_CASES]
LN_ROUTES = ("atomic", "det")           # sa_layernorm_bwd's own dw / db; sa_layernorm_dwprod + sa_colsum_det
CE_ROUTES = ("atomic", "det")            # sa_cross_entropy; sa_cross_entropy_rows + sa_sum_det

WITNESSES = {
    "ln": ("no last column stride", "variance over C-1", "eps omitted", "stats of row r+1", "w of column c+1", "dx without the mean terms",
           "last row block dropped", "overwritten, not accumulated", "truncated store"),
    "ce": ("no last column stride", "no max shift", "one-hot at t+1", "target of row r+1", "gscale missing", "last row block dropped",
           "overwritten, not accumulated", "ignored row counted", "truncated store"),
}


# ------------------------------------------------------------------------------------------------------------------------------ launch rules
def wave_chain(n: int) -> int:
    """longest addition chain of a wave's sum over n columns: a lane's stride-64 columns, then wave_sum's six levels"""
    return -(-n // 64) + 6


def last_stride(n: int) -> int:
    """first column of the last stride-64 pass of a wave over n columns"""
    return 64 * ((n - 1) // 64)


def ln_col_rule(R: int, C: int, route: str):
    """(kernel, L, A, rows of the last row block) of the dw / db column sums: L the longest addition chain, A the additions onto the accumulator"""
    if route == "det":
        rpb = -(-R // 256)
        nblk = -(-R // rpb)
        return "colsum_det", -(-rpb // 4) + 2 + nblk, 0, R - (nblk - 1) * rpb
    if C <= 512:
        return "rows", 8 + 2 + -(-R // 32), -(-R // 32), R - 32 * ((R - 1) // 32)
    return "per-element", R, R, R - 4 * ((R - 1) // 4)


def ce_loss_rule(R: int, route: str):
    """(L, A, rows of the last row block) of the loss sum"""
    if route == "det":
        return -(-R // 1024) + 10, 0, R - 4 * ((R - 1) // 4)
    return 8 + -(-R // 8), -(-R // 8), R - 8 * ((R - 1) // 8)


def f32(v: float) -> float:
    """v as the c_float a kernel argument becomes"""
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------------------------------------ operands
def draw_ln(R: int, C: int, offset: float, scale: float, seed: int = 0):
    """the operands of one LayerNorm case, fp32 on the CPU; per-row scales in [0.5, 2] so that neighbouring rows differ; dw0 / db0 the pre-existing
    accumulator contents (the scale of a sum of R unit terms)"""
    gen = torch.Generator().manual_seed(seed + 7 * R + C + int(1000 * scale))
    rs = 0.5 + 1.5 * torch.rand(R, 1, generator=gen)
    x = (torch.randn(R, C, generator=gen) + offset) * (scale * rs)
    dy = torch.randn(R, C, generator=gen)
    w = 1.0 + 0.5 * torch.randn(C, generator=gen)
    b = 0.3 * torch.randn(C, generator=gen)
    dw0, db0 = R ** 0.5 * torch.randn(C, generator=gen), R ** 0.5 * torch.randn(C, generator=gen)
    return dict(x=x, dy=dy, w=w, b=b, dw0=dw0, db0=db0)


def draw_ce(R: int, V: int, scale: float, offset: float, seed: int = 0):
    """the operands of one cross-entropy case: logits, targets (row R // 2 is ignored), a non-zero loss accumulator; `bad`: the same targets with
    V in row 2 and -1 in row 3 (only (10, 7) runs it)"""
    gen = torch.Generator().manual_seed(seed + 7 * R + V + int(scale) + int(offset))
    l = torch.randn(R, V, generator=gen) * scale + offset
    tgt = torch.randint(0, V, (R,), generator=gen)
    if (R, V) == (8, 65):                          # two -inf logits at non-target classes of row 5, one of them in the second column stride
        t = int(tgt[5])
        c1 = (t + 1) % V
        c2 = 64 if 64 not in (t, c1) else (t + 3) % V
        l[5, c1] = l[5, c2] = float("-inf")
    tgt[R // 2] = -100
    bad = tgt.clone()
    bad[2], bad[3] = V, -1
    return dict(l=l, tgt=tgt, bad=bad, loss0=torch.tensor([f32(0.37 * R)], dtype=torch.float32))


def ce_variants(R: int, V: int):
    """(suffix of the tag, key of the targets in draw_ce's operands): (10, 7) runs a second time with the targets V and -1 planted"""
    return [("", "tgt")] + ([(" bad targets", "bad")] if (R, V) == (10, 7) else [])


# ------------------------------------------------------------------------------------------------------------------------------ LayerNorm forward
class RowStats:
    """per-row statistics (fp64, [R, 1]) and their bounds"""

    def __init__(self, x, eps: float = EPS32, drop_stride: bool = False, bessel: bool = False, no_eps: bool = False):
        C = x.shape[1]
        xs = x[:, : last_stride(C)] if drop_stride else x          # (witness: the sums miss the last column stride and are still divided by C)
        self.mu = xs.sum(1, keepdim=True) / C
        self.var = ((xs - self.mu) ** 2).sum(1, keepdim=True) / (C - 1 if bessel else C)
        G = wave_chain(C) * U
        self.dmu = G * x.abs().mean(1, keepdim=True) + 2 * U * self.mu.abs()
        self.dvar = (G + 4 * U) * self.var + self.dmu ** 2
        self.rstd = (self.var + (0.0 if no_eps else eps)).rsqrt()
        self.drstd = self.rstd * (self.dvar / (2 * (self.var + eps)) + (E + 2) * U)

    def rolled(self):
        """witness: row r carries the statistics of row r + 1"""
        S = object.__new__(RowStats)
        for k, v in vars(self).items():
            setattr(S, k, torch.roll(v, -1, 0))
        return S


def ln_apply(x, S: RowStats, w, b):
    return (x - S.mu) * S.rstd * w + b


def ln_apply_bound(x, S: RowStats, w, b):
    d = (x - S.mu).abs()
    return w.abs() * (S.rstd * S.dmu + d * S.drstd) + 4 * U * (d * S.rstd * w.abs() + b.abs()) + 1e-300


# ------------------------------------------------------------------------------------------------------------------------------ LayerNorm backward
def ln_backward_ref(x, dy, w, mean, rstd, dw0, db0, no_means=False, roll_rows=False, roll_w=False, drop_stride=False, drop_last=0):
    """(dx, dw, db) in fp64 from the mean / rstd [R, 1] the kernel gets.  The keyword arguments plant one defect each: dx without its two mean terms;
    row r normalised with the statistics of row r + 1; column c scaled by the weight of column c + 1; s1 / s2 without the last column stride; dw / db
    without the last `drop_last` rows."""
    R, C = x.shape
    if roll_rows:
        mean, rstd = torch.roll(mean, -1, 0), torch.roll(rstd, -1, 0)
    xh = (x - mean) * rstd
    g = dy * (torch.roll(w, -1, 0) if roll_w else w)
    n = last_stride(C) if drop_stride else C
    s1, s2 = g[:, :n].sum(1, keepdim=True) / C, (g * xh)[:, :n].sum(1, keepdim=True) / C
    dx = rstd * g if no_means else rstd * (g - s1 - xh * s2)
    return dx, dw0 + (dy * xh)[: R - drop_last].sum(0), db0 + dy[: R - drop_last].sum(0)


def ln_backward_bounds(x, dy, w, mean, rstd, dw0, db0, route: str):
    """bounds of (dx, dw, db)"""
    R, C = x.shape
    G = wave_chain(C) * U
    _, L, A, _ = ln_col_rule(R, C, route)
    xh = (x - mean) * rstd
    g = dy * w
    s1, s2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    ds1, ds2 = (G + U) * g.abs().mean(1, keepdim=True), (G + 4 * U) * (g * xh).abs().mean(1, keepdim=True)
    bdx = rstd * (ds1 + xh.abs() * ds2 + 6 * U * (g.abs() + s1.abs() + xh.abs() * s2.abs())) + 1e-300
    sw, sb = (dy * xh).sum(0), dy.sum(0)
    bdw = (L * U + 4 * U) * (dy * xh).abs().sum(0) + 2 * U * (dw0.abs() + sw.abs()) + A * U * dw0.abs() + 1e-300
    bdb = L * U * dy.abs().sum(0) + 2 * U * (db0.abs() + sb.abs()) + A * U * db0.abs() + 1e-300
    return bdx, bdw, bdb


# ------------------------------------------------------------------------------------------------------------------------------ cross-entropy
def ce_ref(l, tgt, gscale: float, drop_stride=False, no_shift=False, shift_onehot=False, roll_rows=False, count_ignored=False):
    """fp64 cross-entropy of logits l [R, V]: dict(m, s, lse, p, lt, term [R], grad [R, V], valid, ignored).  The keyword arguments plant one defect
    each: the sum of exponentials without the last column stride; no max shift (the exponentials and their sum overflow as fp32 ones would); the
    one-hot and the gathered logit at class t + 1; row r with the target of row r + 1; an ignored row counted as class 0."""
    R, V = l.shape
    if roll_rows:
        tgt = torch.roll(tgt, -1, 0)
    m = l.max(1, keepdim=True).values
    e = torch.exp(l - m)
    if drop_stride:
        e = e.clone()
        e[:, last_stride(V):] = 0.0
    s = e.sum(1, keepdim=True)
    lse = m + torch.log(s)
    if no_shift:
        lse = torch.log(torch.exp(l).float().double().sum(1, keepdim=True).float().double())
    p = torch.exp(l - lse)
    valid, ignored = (tgt >= 0) & (tgt < V), tgt == -100
    if count_ignored:
        tgt, valid = torch.where(ignored, torch.zeros_like(tgt), tgt), valid | ignored
    ti = ((tgt.clamp(0, V - 1) + (1 if shift_onehot else 0)) % V).view(R, 1)
    lt = l.gather(1, ti)
    nan = torch.full((R,), float("nan"), dtype=l.dtype)
    zero = torch.zeros(R, dtype=l.dtype)
    term = torch.where(valid, (lse - lt).view(R), torch.where(ignored, zero, nan))
    onehot = torch.zeros_like(l).scatter_(1, ti, 1.0)
    grad = torch.where(valid.view(R, 1), (p - onehot) * gscale, torch.zeros_like(l))
    return dict(m=m, s=s, lse=lse, p=p, lt=lt, term=term, grad=grad, valid=valid, ignored=ignored)


def ce_bounds(l, ref, gscale: float, out: str):
    """(dterm [R], dgrad [R, V]) of ce_ref's truth"""
    R, V = l.shape
    m, s, lse, p, lt, valid = ref["m"], ref["s"], ref["lse"], ref["p"], ref["lt"], ref["valid"]
    zero = torch.zeros_like(l)
    ds = wave_chain(V) * U + E * U + U * torch.where(p > 0, p * (l - m).abs(), zero).sum(1, keepdim=True) + V * TINY      # (a -inf logit: p = 0 exactly)
    dlse = ds + E * U * torch.log(s).abs() + U * lse.abs()
    dterm = torch.where(valid, (dlse + U * (lse - lt).abs()).view(R), torch.zeros(R, dtype=l.dtype)) + 1e-300
    slack = gscale * p * (U * torch.where(p > 0, (l - lse).abs(), zero) + dlse + E * U) + 2 * U * ref["grad"].abs() + TINY
    slack = torch.where(valid.view(R, 1) & (l > float("-inf")), slack, zero)
    return dterm, slack + cb.half_ulp(ref["grad"].abs() + slack, out) + 1e-300


def ce_loss_ref(term, loss0, drop_last: int = 0):
    """loss0 + the sum of the first R - drop_last terms, shape [1]"""
    return (loss0 + term[: term.shape[0] - drop_last].sum()).view(1)


def ce_loss_bound(term, dterm, loss0, route: str):
    L, A, _ = ce_loss_rule(term.shape[0], route)
    return (dterm.sum() + L * U * term.abs().sum() + A * U * abs(loss0)).view(1) + 1e-300


# ------------------------------------------------------------------------------------------------------------------------------ checks
def within(what: str, got, ref, bnd, witnesses, ratios=None, asserted=None):
    """norm_bounds.assert_within; the names of the witnesses it asserts (its rule: the planted defect leaves the bound of the truth somewhere, decided
    from the two references alone) are added to `asserted`"""
    if asserted is not None:
        for name, wit in witnesses.items():
            if not float(((wit - ref).abs() / bnd).max()) <= 1.0:
                asserted.add(name)
    nb.assert_within(what, got, ref, bnd, witnesses, ratios)


def assert_rounded_once(what: str, y32, y_lp, dt: str, asserted=None):
    """y_lp is the kernel's own fp32 y rounded once to nearest even -- equality; the witness (a truncating store) must differ"""
    y32, y_lp = y32.detach().cpu(), y_lp.detach().cpu()
    assert y_lp.dtype == cb.DT[dt] and y_lp.shape == y32.shape
    want = y32.to(cb.DT[dt])
    n = int((y_lp.float() != want.float()).sum())
    print(f"  {what}: {n} of {y32.numel()} elements differ from y rounded once to {dt}")
    assert n == 0, f"{what}: {n} of {y32.numel()} elements differ from y rounded once to {dt}"
    trunc = cb.truncated(y32.double(), dt).to(cb.DT[dt])
    nt = int((trunc.float() != want.float()).sum())
    if nt == 0:
        print("    witness truncated store: every y is exact in the 16-bit type -- not asserted")
        return
    print(f"    witness truncated store: differs on {nt} elements, fails as it must")
    if asserted is not None:
        asserted.add("truncated store")
    assert not torch.equal(y_lp.float(), trunc.float())


# ------------------------------------------------------------------------------------------------------------------------------ fp32 model
def _wave_sum32(v):
    """row sums of v [R, n] (fp32) in a wave's order: lane k adds columns k, k + 64, ... in order, then the six butterfly levels of wave_sum"""
    R, n = v.shape
    k = -(-n // 64)
    pad = torch.zeros(R, k * 64, dtype=torch.float32)
    pad[:, :n] = v
    pad = pad.view(R, k, 64)
    acc = torch.zeros(R, 64, dtype=torch.float32)
    for j in range(k):
        acc = acc + pad[:, j]
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ o]
    return acc[:, :1]


def _t(v: float):
    return torch.tensor(v, dtype=torch.float32)


def model_ln_forward(x, w, b, eps: float = EPS32):
    """layernorm_fwd_kernel in fp32 torch arithmetic, operation by operation: (y, stats [2 R])"""
    R, C = x.shape
    mean = _wave_sum32(x) / _t(float(C))
    d = x - mean
    rstd = (_wave_sum32(d * d) / _t(float(C)) + _t(eps)).rsqrt()
    y = (x - mean) * rstd * w + b
    return y, torch.cat([mean, rstd], 1).reshape(-1)


def _blocked_colsum32(v, acc0, rows: int, lanes: int):
    """acc0 + column sums of v [R, C] in the order of a kernel whose blocks own `rows` consecutive rows each: `lanes` = 4 partial sums per block and
    column, combined as (0 + 1) + (2 + 3); the blocks are added in order (one of the orders the atomics can take).  lanes > 0: lane k adds the rows
    k, k + 4, ... of the block (colsum_det_stage1_kernel); lanes < 0: lane k adds the block's k-th run of rows / 4 consecutive rows (the four waves
    of layernorm_bwd_rows_kernel).  Returns (the block sum added in order from 0, acc0 + each block in order)."""
    R, C = v.shape
    nblk = -(-R // rows)
    steps = -(-rows // 4)
    pad = torch.zeros(nblk, steps * 4, C, dtype=torch.float32)
    for bi in range(nblk):
        blk = v[bi * rows: (bi + 1) * rows]
        pad[bi, : blk.shape[0]] = blk
    pad = pad.view(nblk, steps, 4, C) if lanes > 0 else pad.view(nblk, 4, steps, C).transpose(1, 2)
    acc = torch.zeros(nblk, 4, C, dtype=torch.float32)
    for s in range(steps):
        acc = acc + pad[:, s]
    t = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
    seq, tot = torch.zeros(C, dtype=torch.float32), acc0.clone()
    for bi in range(nblk):
        seq, tot = seq + t[bi], tot + t[bi]
    return seq, tot


def model_ln_backward(x, dy, w, stats, dw0, db0, route: str):
    """sa_layernorm_bwd (route atomic: the rows kernel for C <= 512, the per-element kernel above) or sa_layernorm_dwprod + sa_colsum_det (route det)
    in fp32 torch arithmetic: (dx, dw, db)"""
    R, C = x.shape
    mean, rstd = stats.view(R, 2)[:, :1], stats.view(R, 2)[:, 1:]
    xh = (x - mean) * rstd
    g = dy * w
    s1, s2 = _wave_sum32(g) / _t(float(C)), _wave_sum32(g * xh) / _t(float(C))
    dx = (g - s1 - xh * s2) * rstd
    if route == "det":
        rpb = -(-R // 256)
        sw, _ = _blocked_colsum32(dy * (x - mean) * rstd, dw0, rpb, 4)
        sb, _ = _blocked_colsum32(dy, db0, rpb, 4)
        return dx, dw0 + sw, db0 + sb
    if C <= 512:
        return dx, _blocked_colsum32(dy * xh, dw0, 32, -4)[1], _blocked_colsum32(dy, db0, 32, -4)[1]
    dw, db = dw0.clone(), db0.clone()
    for r in range(R):
        dw, db = dw + (dy * xh)[r], db + dy[r]
    return dx, dw, db


def model_ce(l, tgt, loss0, gscale: float, route: str, out: str):
    """ce_kernel (route atomic: returns loss0 + the sum) or ce_rows_kernel + sum_det_kernel (route det: the sum alone, as sa_sum_det's accumulate = 0
    writes it) in fp32 torch arithmetic: (loss [1], row_loss [R], grad [R, V] in the output type)"""
    R, V = l.shape
    mx = l.max(1, keepdim=True).values
    lse = mx + torch.log(_wave_sum32(torch.exp(l - mx)))
    valid, ignored = (tgt >= 0) & (tgt < V), tgt == -100
    ti = tgt.clamp(0, V - 1).view(R, 1)
    nan, zero = torch.full((R,), float("nan"), dtype=torch.float32), torch.zeros(R, dtype=torch.float32)
    term = torch.where(valid, (lse - l.gather(1, ti)).view(R), torch.where(ignored, zero, nan))
    onehot = torch.zeros_like(l).scatter_(1, ti, 1.0)
    grad = torch.where(valid.view(R, 1), (torch.exp(l - lse) - onehot) * _t(gscale), torch.zeros_like(l)).to(cb.DT[out])
    if route == "det":                              # thread e holds term e (R <= 1024), then the fixed tree
        red = torch.zeros(1024, dtype=torch.float32)
        red[:R] = term
        o = 512
        while o > 0:
            red = torch.cat([red[:o] + red[o: 2 * o], red[o:]])
            o //= 2
        return red[:1].clone(), term, grad
    pad = torch.zeros(-(-R // 8) * 8, dtype=torch.float32)
    pad[:R] = term
    tot = loss0.clone()
    for blk in pad.view(-1, 8):
        t = _t(0.0)
        for i in range(8):
            t = t + blk[i]
        tot = tot + t
    return tot, term, grad


# ------------------------------------------------------------------------------------------------------------------------------ one case, every output
def fp64(ops):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in ops.items()}


def ln_backward_stats(ops, eps: float = EPS32):
    """the fp32 stats [2 R] a backward call is given: the fp64 row statistics rounded once"""
    S = RowStats(ops["x"].double(), eps)
    return torch.cat([S.mu, S.rstd], 1).float().reshape(-1)


def verify_ln_forward(tag: str, ops, got, ratios=None, asserted=None, eps: float = EPS32):
    """got = (y, stats, {16-bit type: y_lp}) of forward calls on ops"""
    o = fp64(ops)
    x, w, b = o["x"], o["w"], o["b"]
    R, C = x.shape
    y, stats, lps = got
    stats = stats.detach().cpu().view(R, 2)
    S = RowStats(x, eps)
    alt = {"no last column stride": RowStats(x, eps, drop_stride=True), "variance over C-1": RowStats(x, eps, bessel=True),
           "eps omitted": RowStats(x, eps, no_eps=True), "stats of row r+1": S.rolled()}
    within(f"{tag} mean", stats[:, :1], S.mu, S.dmu + 1e-300, {k: v.mu for k, v in alt.items() if k in ("no last column stride", "stats of row r+1")},
           ratios, asserted)
    within(f"{tag} rstd", stats[:, 1:], S.rstd, S.drstd, {k: v.rstd for k, v in alt.items()}, ratios, asserted)
    wit = {k: ln_apply(x, v, w, b) for k, v in alt.items()}
    wit["w of column c+1"] = ln_apply(x, S, torch.roll(w, -1, 0), b)
    within(f"{tag} y", y, ln_apply(x, S, w, b), ln_apply_bound(x, S, w, b), wit, ratios, asserted)
    for dt, y_lp in lps.items():
        assert_rounded_once(f"{tag} y_lp[{dt}]", y, y_lp, dt, asserted)


def verify_ln_backward(tag: str, ops, route: str, stats32, got, ratios=None, asserted=None):
    """got = (dx, dw, db) of one backward call that was given stats32 and accumulated into dw0 / db0; dx None: the route has none (det)"""
    o = fp64(ops)
    R, C = o["x"].shape
    st = stats32.double().cpu().view(R, 2)
    a = (o["x"], o["dy"], o["w"], st[:, :1], st[:, 1:], o["dw0"], o["db0"])
    rdx, rdw, rdb = ln_backward_ref(*a)
    bdx, bdw, bdb = ln_backward_bounds(*a, route)
    last = ln_col_rule(R, C, route)[3]
    _, ddw, ddb = ln_backward_ref(*a, drop_last=last)
    rolled = ln_backward_ref(*a, roll_rows=True)
    dx, dw, db = got
    if dx is not None:
        wit = {"dx without the mean terms": ln_backward_ref(*a, no_means=True)[0], "stats of row r+1": rolled[0],
               "w of column c+1": ln_backward_ref(*a, roll_w=True)[0], "no last column stride": ln_backward_ref(*a, drop_stride=True)[0]}
        within(f"{tag} dx", dx, rdx, bdx, wit, ratios, asserted)
    within(f"{tag} dw", dw, rdw, bdw, {"last row block dropped": ddw, "overwritten, not accumulated": rdw - o["dw0"], "stats of row r+1": rolled[1]},
           ratios, asserted)
    within(f"{tag} db", db, rdb, bdb, {"last row block dropped": ddb, "overwritten, not accumulated": rdb - o["db0"]}, ratios, asserted)


def verify_ce(tag: str, ops, tgt, gscale: float, route: str, out: str, got, ratios=None, asserted=None):
    """got = (loss [1], row_loss [R] or None, grad [R, V] or None) of one call with targets tgt: route atomic accumulated the loss onto loss0,
    route det wrote the sum of row_loss"""
    l = ops["l"].double()
    R, V = l.shape
    loss0 = float(ops["loss0"]) if route == "atomic" else 0.0
    ref = ce_ref(l, tgt, gscale)
    dterm, dgrad = ce_bounds(l, ref, gscale, out)
    wits = {"no last column stride": ce_ref(l, tgt, gscale, drop_stride=True), "no max shift": ce_ref(l, tgt, gscale, no_shift=True),
            "one-hot at t+1": ce_ref(l, tgt, gscale, shift_onehot=True), "target of row r+1": ce_ref(l, tgt, gscale, roll_rows=True)}
    loss, row_loss, grad = got
    valid, ignored, ok = ref["valid"], ref["ignored"], ref["valid"] | ref["ignored"]
    if row_loss is not None:
        row_loss = row_loss.detach().cpu()
        assert bool(torch.isnan(row_loss[~ok]).all()), f"{tag}: a target outside [0, V) other than -100 must give a NaN term"
        assert bool((row_loss[ignored] == 0).all()), f"{tag}: an ignored row must give the term 0"
        wrow = {k: v["term"][ok] for k, v in wits.items()}
        wrow["ignored row counted"] = ce_ref(l, tgt, gscale, count_ignored=True)["term"][ok]
        within(f"{tag} row_loss", row_loss[ok], ref["term"][ok], dterm[ok], wrow, ratios, asserted)
    loss = loss.detach().cpu().view(1)
    if not bool(ok.all()):
        print(f"  {tag} loss: {float(loss)} (targets outside [0, V) planted: NaN expected)")
        assert bool(torch.isnan(loss).all()), f"{tag}: a target outside [0, V) other than -100 must poison the loss, got {float(loss)}"
    else:
        last = ce_loss_rule(R, route)[2]
        wl = {k: ce_loss_ref(v["term"], loss0) for k, v in wits.items()}
        wl["last row block dropped"] = ce_loss_ref(ref["term"], loss0, drop_last=last)
        wl["ignored row counted"] = ce_loss_ref(ce_ref(l, tgt, gscale, count_ignored=True)["term"], loss0)
        if route == "atomic":
            wl["overwritten, not accumulated"] = ce_loss_ref(ref["term"], 0.0)
        within(f"{tag} loss", loss, ce_loss_ref(ref["term"], loss0), ce_loss_bound(ref["term"], dterm, loss0, route), wl, ratios, asserted)
    if grad is not None:
        g = grad.detach().cpu()
        assert g.dtype == cb.DT[out]
        assert bool((g[~valid] == 0).all()), f"{tag}: the gradient of a row whose target is ignored or out of range must be 0"
        assert bool((g[ops["l"] == float("-inf")] == 0).all()), f"{tag}: the gradient at a -inf logit must be 0"
        wg = {k: v["grad"] for k, v in wits.items()}
        wg["gscale missing"] = ce_ref(l, tgt, 1.0)["grad"]
        if out != "f32":
            wg["truncated store"] = cb.truncated(ref["grad"], out)
        within(f"{tag} grad" if out == "f32" else f"{tag} grad_{out}", g, ref["grad"], dgrad, wg, ratios, asserted)
