"""Element-wise fp64 error bounds for the discriminator's BatchNorm (+ LeakyReLU) kernels (csrc/norm.hip: sa_bn_forward, sa_bn_backward), the
planted-defect witnesses that an output must fail, and an fp32 model of the kernels' arithmetic (tests/test_norm_bounds_cpu.py holds the model
to the same bounds; tests/test_norm_bounds_gpu.py holds the kernels to them).

The inputs are drawn in fp32 and rounded to the operand type (conv_bounds.rounded), so the fp64 reference sees exactly the kernel's values and
the only legitimate error is the kernel's own fp32 arithmetic (and the final rounding of a 16-bit output).  With U = 2^-24 one fp32 rounding,
the column sums carry G = L * U, where L is the longest chain of additions a column sum goes through, restated from the launch rule:

    rpb  = max(64, ceil(M / 1024))       rows per block        (deterministic mode: max(64, ceil(M / 64)))
    nblk = ceil(M / rpb)                 row blocks
    L    = ceil(rpb / 8) + 8 + nblk      one lane's rows, the eight lanes of a column, the blocks (in ANY order: atomics or the fixed order)

First-order bounds, with a1 = mean |x|, a2 = mean x^2 and mu, var, rstd the fp64 statistics:

    dmu   = G a1 + 2 U |mu|
    dvar  = G a2 + 2 |mu| dmu + 4 U (a2 + mu^2)                     the kernel's one-pass E[x^2] - mu^2: widens with mu^2 / var
    drstd = rstd (dvar / (2 (var + eps)) + 4 U)
    dy    = |w| (rstd dmu + |x - mu| drstd) + 4 U (|x - mu| rstd |w| + |b|)          (+ half an ulp of a 16-bit y; LeakyReLU has Lipschitz constant 1)
    running_mean, running_var: momentum x the bounds above + 2 U of the result
    db    = G sum|g| + 2 U (|db0| + |sum g|)
    dw    = (G + 4 U) sum|g xhat| + 2 U (|dw0| + |sum g xhat|)
    dx    = |w| rstd (ds1 / M + |xhat| ds2 / M + 6 U (|g| + |s1| / M + |xhat| |s2| / M))   (+ half an ulp; ds1, ds2 the G terms of db and dw;
            eval mode: the same with s1 = s2 = ds1 = ds2 = 0)

The backward takes the mean and rstd the kernel gets (fp32 values), so it is bounded in isolation from the forward.  In eval mode the forward's
statistics are the running buffers: dmu = dvar = 0.

A witness is asserted to fail wherever its planted defect leaves the bound of the truth on at least one element; where it does not (the biased
running variance at 30 sigma means and at M = 70001, where dvar exceeds var / (M - 1)) no output could tell the two apart: printed, not asserted.

Worst max |err| / bound over every case and mode, fp32 / bf16 operands (the acceptance threshold is the bound itself, ratio <= 1; MEASURED below;
the atomic mode's figures move in the last digit from run to run with the order of the atomics):
                        mean           rstd           y             running_mean   running_var    dx            dw             db
    fp32 model (CPU):   0.079 / 0.031  0.365 / 0.365  0.456 / 1.00  0.319 / 0.327  0.211 / 0.124  0.328 / 1.00  0.013 / 0.029  0.022 / 0.016
    MI355X kernels:     0.097 / 0.031  0.376 / 0.376  0.511 / 1.00  0.319 / 0.327  0.211 / 0.113  0.328 / 1.00  0.013 / 0.029  0.022 / 0.016
A bf16 y or dx sits at 1.00 (0.9998): the output's own rounding is up to the half ulp that makes up nearly all of its bound.
"""
from __future__ import annotations

import numpy as np
import torch

import conv_bounds as cb

U = cb.U32
SLOPE32 = float(np.float32(0.2))
EPS32 = float(np.float32(1e-5))
MOMENTUM32 = float(np.float32(0.1))

# worst max |err| / bound measured on the MI355X per output, over every case of tests/test_norm_bounds_gpu.py
MEASURED = dict(f32=dict(mean=0.0967, rstd=0.376, y=0.511, running_mean=0.319, running_var=0.211, dx=0.328, dw=0.0134, db=0.0224),
                bf16=dict(mean=0.0309, rstd=0.376, y=1.0, running_mean=0.327, running_var=0.113, dx=1.0, dw=0.0285, db=0.0164))

# (M, C, channel-mean offset in sigma, modes): the ragged last row block in both modes (4 rows of 64 / 5 rows of 65) with a second column block
# only 8 channels wide; C no multiple of 32 with means up to 30 sigma; a second block of one row; rpb = 69 > 64 in 1015 blocks (default mode only)
CASES = [
    (4100, 40, 0.0, (False, True)),
    (1000, 33, 30.0, (False, True)),
    (65, 8, 0.5, (False, True)),
    (70001, 8, 0.0, (False,)),
]


def launch_rule(M: int, deterministic: bool):
    """(rows per block, row blocks, longest addition chain) of bn_colstats_kernel's launch"""
    rpb = max(64, -(-M // (64 if deterministic else 1024)))
    nblk = -(-M // rpb)
    return rpb, nblk, -(-rpb // 8) + 8 + nblk


def last_block_rows(M: int, deterministic: bool) -> int:
    rpb, nblk, _ = launch_rule(M, deterministic)
    return M - (nblk - 1) * rpb


def gamma(M: int, deterministic: bool) -> float:
    return launch_rule(M, deterministic)[2] * U


def draw(M: int, C: int, offset: float, dt: str, seed: int = 0):
    """the operands of one case, fp32 on the CPU: x and g exact in `dt`; per-channel scales in [0.5, 2] so that neighbouring channels differ"""
    gen = torch.Generator().manual_seed(seed + 7 * M + C)
    scale = 0.5 + 1.5 * torch.rand(C, generator=gen)
    x = cb.rounded((torch.randn(M, C, generator=gen) + offset) * scale, dt)
    g = cb.rounded(torch.randn(M, C, generator=gen), dt)
    w = 1.0 + 0.5 * torch.randn(C, generator=gen)
    b = 0.3 * torch.randn(C, generator=gen)
    rm0 = 0.8 * offset * scale + 0.3 * torch.randn(C, generator=gen)
    rv0 = 0.5 + torch.rand(C, generator=gen)
    dw0, db0 = M ** 0.5 * torch.randn(C, generator=gen), M ** 0.5 * torch.randn(C, generator=gen)      # (the scale of a sum of M unit terms)
    return dict(x=x, g=g, w=w, b=b, rm0=rm0, rv0=rv0, dw0=dw0, db0=db0)


# ------------------------------------------------------------------------------------------------------------------------------ forward
class Stats:
    """per-channel statistics (fp64) and their bounds"""

    def __init__(self, mu, var, dmu, dvar, M, eps=EPS32):
        self.mu, self.var, self.dmu, self.dvar, self.M, self.eps = mu, var, dmu, dvar, M, eps
        self.rstd = (var + eps).rsqrt()
        self.drstd = self.rstd * (dvar / (2 * (var + eps)) + 4 * U)

    def rolled(self):
        """witness: channel c carries the statistics of channel c + 1"""
        r = lambda t: torch.roll(t, -1, 0)
        return Stats(r(self.mu), r(self.var), r(self.dmu), r(self.dvar), self.M, self.eps)


def train_stats(x, G: float, drop_last: int = 0) -> Stats:
    """batch statistics of x [M, C] (fp64).  drop_last: the witness of a lost row block -- the sums miss the last `drop_last` rows and are still
    divided by M, as a kernel would that never added that block's partial."""
    M = x.shape[0]
    xs = x[: M - drop_last] if drop_last else x
    mu = xs.sum(0) / M
    a1 = xs.abs().sum(0) / M
    a2 = (xs * xs).sum(0) / M
    var = a2 - mu * mu if drop_last else ((x - mu) ** 2).mean(0)     # (the same number; the centred form has no cancellation)
    dmu = G * a1 + 2 * U * mu.abs()
    dvar = G * a2 + 2 * mu.abs() * dmu + 4 * U * (a2 + mu * mu)
    return Stats(mu, var.clamp_min(0.0), dmu, dvar, M)


def eval_stats(rm, rv) -> Stats:
    z = torch.zeros_like(rm)
    return Stats(rm, rv, z, z.clone(), 0)


def apply_ref(x, S: Stats, w, b, slope: float = SLOPE32):
    z = (x - S.mu) * S.rstd * w + b
    return torch.where(z > 0, z, z * slope)


def apply_bound(x, S: Stats, w, b, out: str):
    d = (x - S.mu).abs()
    slack = w.abs() * (S.rstd * S.dmu + d * S.drstd) + 4 * U * (d * S.rstd * w.abs() + b.abs())
    y = apply_ref(x, S, w, b)
    return slack + cb.half_ulp(y.abs() + slack, out) + 1e-300


def running_ref(S: Stats, rm0, rv0, momentum: float = MOMENTUM32, biased: bool = False, wrong_side: bool = False):
    unb = S.var if biased or S.M <= 1 else S.var * (S.M / (S.M - 1))
    a, c = (momentum, 1.0 - momentum) if wrong_side else (1.0 - momentum, momentum)
    return a * rm0 + c * S.mu, a * rv0 + c * unb


def running_bound(S: Stats, rm0, rv0, momentum: float = MOMENTUM32):
    rm, rv = running_ref(S, rm0, rv0, momentum)
    f = S.M / (S.M - 1) if S.M > 1 else 1.0
    return momentum * S.dmu + 2 * U * rm.abs() + 1e-300, momentum * f * S.dvar + 2 * U * rv.abs() + 1e-300


# ------------------------------------------------------------------------------------------------------------------------------ backward
def backward_ref(x, g, w, mean, rstd, dw0, db0, training: bool, drop_last: int = 0, dx_training=None, roll: bool = False):
    """(dx, dw, db) in fp64 from the mean / rstd the kernel gets.  drop_last: the sums miss the last rows (witness); dx_training: the dx formula of
    that mode instead of `training`'s (witness); roll: channel c normalised with the statistics of channel c + 1 (witness)."""
    if roll:
        mean, rstd = torch.roll(mean, -1, 0), torch.roll(rstd, -1, 0)
    M = x.shape[0]
    xh = (x - mean) * rstd
    n = M - drop_last
    s1, s2 = g[:n].sum(0), (g[:n] * xh[:n]).sum(0)
    if training if dx_training is None else dx_training:
        dx = w * rstd * (g - s1 / M - xh * s2 / M)
    else:
        dx = w * rstd * g
    return dx, dw0 + s2, db0 + s1


def backward_bounds(x, g, w, mean, rstd, dw0, db0, training: bool, G: float, out: str):
    """bounds of (dx, dw, db)"""
    M = x.shape[0]
    xh = (x - mean) * rstd
    s1, s2 = g.sum(0), (g * xh).sum(0)
    A1, A2 = g.abs().sum(0), (g * xh).abs().sum(0)
    ds1, ds2 = G * A1, (G + 4 * U) * A2
    bdb = ds1 + 2 * U * (db0.abs() + s1.abs()) + 1e-300
    bdw = ds2 + 2 * U * (dw0.abs() + s2.abs()) + 1e-300
    if training:
        slack = w.abs() * rstd * (ds1 / M + xh.abs() * ds2 / M + 6 * U * (g.abs() + s1.abs() / M + xh.abs() * s2.abs() / M))
    else:
        slack = w.abs() * rstd * 6 * U * g.abs()
    dx = backward_ref(x, g, w, mean, rstd, dw0, db0, training)[0]
    return slack + cb.half_ulp(dx.abs() + slack, out) + 1e-300, bdw, bdb


# ------------------------------------------------------------------------------------------------------------------------------ checks
def check(got, ref, bnd):
    """(passes, max |got - ref| / bound)"""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= bnd)                          # (NaN fails)
    return not bool(bad.any()), float((err / bnd).max())


def assert_within(what: str, got, ref, bnd, witnesses, ratios=None, log=print):
    """got within bnd of ref, and NOT within bnd of any witness (name -> the reference with one planted defect)."""
    ok, ratio = check(got, ref, bnd)
    log(f"  {what}: max |err| / bound = {ratio:.3g}")
    if ratios is not None:
        key = what.split()[-1]
        ratios[key] = max(ratios.get(key, 0.0), ratio)
    assert ok, f"{what}: max |err| / bound = {ratio:.3g}"
    for name, wit in witnesses.items():
        wok, wratio = check(got, wit, bnd)
        defect = float(((wit - ref).abs() / bnd).max())
        if defect <= 1.0:
            # a defect inside the bound of the truth on every element is below what the bound resolves at this shape: the exact result itself would
            # pass as the witness (decided from the two references alone, never from the output)
            log(f"    witness {name}: the planted defect is {defect:.3g} x the bound at this shape, below what it resolves -- not asserted "
                f"(max |err| / bound = {wratio:.3g})")
            continue
        log(f"    witness {name}: max |err| / bound = {wratio:.3g}, {'PASSES -- the bound does not discriminate' if wok else 'fails as it must'}")
        assert not wok, f"{what}: the planted defect '{name}' is not detected at this shape (max |err| / bound = {wratio:.3g})"


# ------------------------------------------------------------------------------------------------------------------------------ fp32 model
def _colsum32(v, rpb: int, nblk: int):
    """column sums of v [M, C] (fp32) in the kernel's order: each of a block's eight lanes adds its rows r0 + lane, + 8, ...; the eight lanes are
    added in order; the blocks are added in order (one of the orders the atomics can take, and the deterministic mode's)."""
    M, C = v.shape
    steps = -(-rpb // 8)
    pad = torch.zeros(nblk * steps * 8, C, dtype=torch.float32)
    idx = torch.arange(nblk * steps * 8)
    blk, step, lane = idx // (steps * 8), (idx // 8) % steps, idx % 8
    inb = step * 8 + lane
    row = blk * rpb + inb
    ok = (inb < rpb) & (row < M)
    pad[ok] = v[row[ok]]
    pad = pad.view(nblk, steps, 8, C)
    acc = torch.zeros(nblk, 8, C, dtype=torch.float32)
    for s in range(steps):
        acc = acc + pad[:, s]
    t = torch.zeros(nblk, C, dtype=torch.float32)
    for k in range(8):
        t = t + acc[:, k]
    tot = torch.zeros(C, dtype=torch.float32)
    for bi in range(nblk):
        tot = tot + t[bi]
    return tot


def model_forward(x, w, b, rm0, rv0, training: bool, deterministic: bool, out: str, eps=EPS32, momentum=MOMENTUM32, slope=SLOPE32):
    """sa_bn_forward in fp32 torch arithmetic, operation by operation: (y, mean, rstd, running_mean, running_var)"""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    x = x.float()
    M = x.shape[0]
    rm = rv = None
    if training:
        rpb, nblk, _ = launch_rule(M, deterministic)
        s1, s2 = _colsum32(x, rpb, nblk), _colsum32(x * x, rpb, nblk)
        mu = s1 / f(float(M))
        var = (s2 / f(float(M)) - mu * mu).clamp_min(0.0)
        mean, rstd = mu, (var + f(eps)).rsqrt()
        if rm0 is not None:
            unb = var * (f(float(M)) / f(float(M - 1))) if M > 1 else var
            rm = (f(1.0) - f(momentum)) * rm0 + f(momentum) * mu
            rv = (f(1.0) - f(momentum)) * rv0 + f(momentum) * unb
    else:
        mean, rstd = rm0.clone(), (rv0 + f(eps)).rsqrt()
    v = (x - mean) * rstd * w + b
    y = torch.where(v > 0, v, v * f(slope))
    return y.to(cb.DT[out]), mean, rstd, rm, rv


def model_backward(x, g, w, mean, rstd, dw0, db0, training: bool, deterministic: bool, out: str):
    """sa_bn_backward in fp32 torch arithmetic: (dx, dw, db)"""
    x, g = x.float(), g.float()
    M = x.shape[0]
    rpb, nblk, _ = launch_rule(M, deterministic)
    s1, s2 = _colsum32(g, rpb, nblk), _colsum32(g * (x - mean) * rstd, rpb, nblk)
    v = g
    if training:
        invM = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(M), dtype=torch.float32)
        xh = (x - mean) * rstd
        v = g - s1 * invM - xh * s2 * invM
    return (v * w * rstd).to(cb.DT[out]), dw0 + s2, db0 + s1


# ------------------------------------------------------------------------------------------------------------------------------ one case, every output
def fp64(ops):
    return {k: v.double() for k, v in ops.items()}


def backward_stats(ops, training: bool):
    """the fp32 (mean, rstd) a backward call is given: the batch statistics (training) or the running buffers' (eval), rounded once"""
    o = fp64(ops)
    S = train_stats(o["x"], 0.0) if training else eval_stats(o["rm0"], o["rv0"])
    return S.mu.float(), S.rstd.float()


def verify_forward(tag: str, ops, dt: str, deterministic: bool, mode: str, got, ratios=None):
    """got = (y, mean, rstd, running_mean, running_var) of one forward call; mode: train (running buffers updated) / train_norun / eval"""
    o = fp64(ops)
    x, w, b = o["x"], o["w"], o["b"]
    M = x.shape[0]
    y, mean, rstd, rm, rv = got
    if mode == "eval":
        S = eval_stats(o["rm0"], o["rv0"])
        assert_within(f"{tag} mean", mean, S.mu, S.dmu + 1e-300, {}, ratios)
        assert_within(f"{tag} rstd", rstd, S.rstd, S.drstd, {"stats of c+1": S.rolled().rstd}, ratios)
        wit = {"stats of c+1": apply_ref(x, S.rolled(), w, b)}
    else:
        S = train_stats(x, gamma(M, deterministic))
        D = train_stats(x, gamma(M, deterministic), drop_last=last_block_rows(M, deterministic))
        assert_within(f"{tag} mean", mean, S.mu, S.dmu, {"last row block dropped": D.mu}, ratios)
        assert_within(f"{tag} rstd", rstd, S.rstd, S.drstd, {"last row block dropped": D.rstd}, ratios)
        wit = {"last row block dropped": apply_ref(x, D, w, b), "stats of c+1": apply_ref(x, S.rolled(), w, b)}
    ref = apply_ref(x, S, w, b)
    wit["slope 0"] = torch.relu(ref)
    if dt != "f32":
        wit["truncated store"] = cb.truncated(ref, dt)
    assert_within(f"{tag} y", y, ref, apply_bound(x, S, w, b, dt), wit, ratios)
    if mode == "train":
        rrm, rrv = running_ref(S, o["rm0"], o["rv0"])
        brm, brv = running_bound(S, o["rm0"], o["rv0"])
        wrm, wrv = running_ref(S, o["rm0"], o["rv0"], wrong_side=True)
        drm, drv = running_ref(D, o["rm0"], o["rv0"])
        assert_within(f"{tag} running_mean", rm, rrm, brm, {"last row block dropped": drm, "momentum on the wrong side": wrm}, ratios)
        assert_within(f"{tag} running_var", rv, rrv, brv, {"last row block dropped": drv, "momentum on the wrong side": wrv,
                                                           "biased variance": running_ref(S, o["rm0"], o["rv0"], biased=True)[1]}, ratios)
    else:           # the buffers are not touched
        assert rm is None or torch.equal(rm.cpu(), ops["rm0"]), f"{tag}: running_mean changed"
        assert rv is None or torch.equal(rv.cpu(), ops["rv0"]), f"{tag}: running_var changed"


def verify_backward(tag: str, ops, dt: str, deterministic: bool, training: bool, mean32, rstd32, got, ratios=None):
    """got = (dx, dw, db) of one backward call that was given (mean32, rstd32) and accumulated into dw0 / db0"""
    o = fp64(ops)
    M = o["x"].shape[0]
    a = (o["x"], o["g"], o["w"], mean32.double().cpu(), rstd32.double().cpu(), o["dw0"], o["db0"])
    rdx, rdw, rdb = backward_ref(*a, training)
    bdx, bdw, bdb = backward_bounds(*a, training, gamma(M, deterministic), dt)
    ddx, ddw, ddb = backward_ref(*a, training, drop_last=last_block_rows(M, deterministic))
    wit = {"the other mode's formula": backward_ref(*a, training, dx_training=not training)[0], "stats of c+1": backward_ref(*a, training, roll=True)[0]}
    if training:
        wit["last row block dropped"] = ddx
    if dt != "f32":
        wit["truncated store"] = cb.truncated(rdx, dt)
    dx, dw, db = got
    assert_within(f"{tag} dx", dx, rdx, bdx, wit, ratios)
    assert_within(f"{tag} dw", dw, rdw, bdw, {"last row block dropped": ddw, "overwritten, not accumulated": rdw - o["dw0"]}, ratios)
    assert_within(f"{tag} db", db, rdb, bdb, {"last row block dropped": ddb, "overwritten, not accumulated": rdb - o["db0"]}, ratios)
