"""GPU: the discriminator's BatchNorm + LeakyReLU kernels (csrc/norm.hip: sa_bn_forward, sa_bn_backward, sa_lrelu_mask), called through _ffi the
way networks/discriminator/baseline.py calls them, against the fp64 reference under the element-wise bounds of tests/norm_bounds.py -- every
output, in fp32 and bf16, with atomics and in deterministic mode, training (with and without running buffers) and eval mode -- with the
planted-defect witnesses that the same output must fail.  Run with -s to read every max |err| / bound and witness."""
import pytest
import torch

import conv_bounds as cb
import norm_bounds as nb

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(16, torch.get_num_threads()))
DEV = "cuda"
PARAMS = [(M, C, off, dt, det) for (M, C, off, modes) in nb.CASES for dt in ("f32", "bf16") for det in modes]
IDS = [f"{M}x{C}-{dt}-{'det' if det else 'atomic'}" for (M, C, off, dt, det) in PARAMS]
RATIOS = {}          # operand type -> output -> worst max |err| / bound so far (printed, never asserted)


def _ws(C):
    """the scratch the library asks for under the CURRENT flags, poisoned: the launch must not rely on its contents"""
    from synthanatomy_amd import _ffi
    return torch.full((int(_ffi.lib().sa_bn_sums_ws_floats(C)),), float("nan"), dtype=torch.float32, device=DEV)


def _forward(ops, dt, det, training, running):
    from synthanatomy_amd import _ffi, debug
    lib = _ffi.lib()
    x = ops["x"].to(DEV).to(cb.DT[dt])
    M, C = x.shape
    w, b = ops["w"].to(DEV), ops["b"].to(DEV)
    rm = ops["rm0"].to(DEV) if running else None
    rv = ops["rv0"].to(DEV) if running else None
    y = torch.empty_like(x)
    mean = torch.full((C,), float("nan"), dtype=torch.float32, device=DEV)
    rstd = mean.clone()
    with debug.override(deterministic=det):
        ws = _ws(C)
        assert ws.numel() == (65 if det else 1) * 2 * C
        _ffi.check(lib.sa_bn_forward(_ffi.ptr(x), _ffi.dtype_id(x.dtype), M, C, _ffi.ptr(w), _ffi.ptr(b), _ffi.ptr(rm), _ffi.ptr(rv), nb.MOMENTUM32, nb.EPS32,
                                     int(training), nb.SLOPE32, _ffi.ptr(y), _ffi.ptr(mean), _ffi.ptr(rstd), _ffi.ptr(ws), _ffi.stream()), "sa_bn_forward")
        torch.cuda.synchronize()
    return y, mean, rstd, rm, rv


def _backward(ops, dt, det, training, mean32, rstd32):
    from synthanatomy_amd import _ffi, debug
    lib = _ffi.lib()
    x, g = ops["x"].to(DEV).to(cb.DT[dt]), ops["g"].to(DEV).to(cb.DT[dt])
    M, C = x.shape
    w, dw, db = ops["w"].to(DEV), ops["dw0"].to(DEV), ops["db0"].to(DEV)
    dx = torch.empty_like(x)
    md, rd = mean32.to(DEV), rstd32.to(DEV)
    with debug.override(deterministic=det):
        ws = _ws(C)
        _ffi.check(lib.sa_bn_backward(_ffi.ptr(x), _ffi.ptr(g), _ffi.dtype_id(x.dtype), M, C, _ffi.ptr(w), _ffi.ptr(md), _ffi.ptr(rd),
                                      int(training), _ffi.ptr(dx), _ffi.ptr(dw), _ffi.ptr(db), _ffi.ptr(ws), _ffi.stream()), "sa_bn_backward")
        torch.cuda.synchronize()
    return dx, dw, db


def _bit_equal(tag, a, b):
    for i, (u, v) in enumerate(zip(a, b)):
        assert (u is None and v is None) or torch.equal(u, v), f"{tag}: output {i} differs between two deterministic calls"


@pytest.mark.parametrize("M,C,off,dt,det", PARAMS, ids=IDS)
def test_bn_forward_within_fp64_bound(M, C, off, dt, det):
    ops = nb.draw(M, C, off, dt)
    tag = f"[{M}x{C} {dt} {'det' if det else 'atomic'}]"
    for mode in ("train", "train_norun", "eval"):
        got = _forward(ops, dt, det, mode != "eval", mode != "train_norun")
        if det:
            _bit_equal(f"{tag} fwd {mode}", got, _forward(ops, dt, det, mode != "eval", mode != "train_norun"))
        nb.verify_forward(f"{tag} fwd {mode}", ops, dt, det, mode, got, RATIOS.setdefault(dt, {}))
    print("worst max |err| / bound so far:", {d: {k: float(f"{v:.3g}") for k, v in r.items()} for d, r in RATIOS.items()})


@pytest.mark.parametrize("M,C,off,dt,det", PARAMS, ids=IDS)
def test_bn_backward_within_fp64_bound(M, C, off, dt, det):
    ops = nb.draw(M, C, off, dt)
    tag = f"[{M}x{C} {dt} {'det' if det else 'atomic'}]"
    for training in (True, False):
        mean32, rstd32 = nb.backward_stats(ops, training)
        got = _backward(ops, dt, det, training, mean32, rstd32)
        if det:
            _bit_equal(f"{tag} bwd", got, _backward(ops, dt, det, training, mean32, rstd32))
        nb.verify_backward(f"{tag} bwd {'train' if training else 'eval'}", ops, dt, det, training, mean32, rstd32, got, RATIOS.setdefault(dt, {}))
    print("worst max |err| / bound so far:", {d: {k: float(f"{v:.3g}") for k, v in r.items()} for d, r in RATIOS.items()})


def test_bn_rejects_missing_running_buffers_in_eval_mode():
    """eval mode without running buffers is an argument error, not a launch"""
    from synthanatomy_amd import _ffi
    ops = nb.draw(65, 8, 0.5, "f32")
    x = ops["x"].to(DEV)
    y, mean, rstd = torch.empty_like(x), torch.empty(8, device=DEV), torch.empty(8, device=DEV)
    rc = _ffi.lib().sa_bn_forward(_ffi.ptr(x), _ffi.SA_F32, 65, 8, _ffi.ptr(ops["w"].to(DEV)), _ffi.ptr(ops["b"].to(DEV)), None, None, nb.MOMENTUM32, nb.EPS32, 0,
                                  nb.SLOPE32, _ffi.ptr(y), _ffi.ptr(mean), _ffi.ptr(rstd), _ffi.ptr(_ws(8)), _ffi.stream())
    assert rc == _ffi.SA_EINVAL


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_lrelu_mask_is_exact(dt):
    """sa_lrelu_mask (exported; the product fuses the same mask into the data-gradient epilogues): g = dy where y > 0, else dy * slope, one fp32
    product rounded once to the output type -- exact equality, with +0.0 and -0.0 planted in y (both take the slope) and a ragged last block"""
    from synthanatomy_amd import _ffi
    n = 8192 * 256 + 77 * 256 + 13         # past the 8192-block grid cap: a second, partial grid-stride pass with a ragged last block
    gen = torch.Generator().manual_seed(11)
    dy = cb.rounded(torch.randn(n, generator=gen), dt)
    y = cb.rounded(torch.randn(n, generator=gen), dt)
    y[5], y[6], y[n - 1], y[n - 2] = 0.0, -0.0, 0.0, -0.0
    assert dy[5] != 0 and dy[6] != 0
    T = cb.DT[dt]
    dyd, yd = dy.to(DEV).to(T), y.to(DEV).to(T)
    g = torch.empty_like(dyd)
    _ffi.check(_ffi.lib().sa_lrelu_mask(_ffi.ptr(dyd), _ffi.ptr(yd), _ffi.dtype_id(T), _ffi.ptr(g), n, nb.SLOPE32, _ffi.stream()), "sa_lrelu_mask")
    torch.cuda.synchronize()
    want = torch.where(y > 0, dy, dy * torch.tensor(nb.SLOPE32, dtype=torch.float32)).to(T)       # fp32 product, then one rounding
    assert torch.equal(g.cpu(), want), f"{int((g.cpu() != want).sum())} of {n} elements differ"
    assert g[5].item() == want[5].item() != dy[5].item() and g[6].item() == want[6].item() != dy[6].item()
