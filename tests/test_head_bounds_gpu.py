"""GPU: the Performer's LayerNorm and cross-entropy kernels (csrc/performer.hip: sa_layernorm_fwd, sa_layernorm_bwd, sa_cross_entropy;
csrc/deterministic.hip: sa_layernorm_dwprod + sa_colsum_det, sa_cross_entropy_rows + sa_sum_det), called through _ffi the way
networks/transformers/performer.py and losses/transformer.py call them, against the fp64 reference under the element-wise bounds of
tests/head_bounds.py -- every output, both reduction routes, the 16-bit copies and gradients -- with the planted-defect witnesses that the same
output must fail.  Every output buffer that is not an accumulator starts as NaN.  Run with -s to read every max |err| / bound and witness."""
import pytest
import torch

import conv_bounds as cb
import head_bounds as hb

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(16, torch.get_num_threads()))
DEV = "cuda"
RATIOS = {"ln": {}, "ce": {}}        # output -> worst max |err| / bound so far (printed; the checks themselves assert <= 1 element-wise)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _bit_equal(tag, a, b):
    for i, (u, v) in enumerate(zip(a, b)):
        assert (u is None and v is None) or torch.equal(u.view(torch.int32 if u.dtype == torch.float32 else torch.int16),
                                                        v.view(torch.int32 if v.dtype == torch.float32 else torch.int16)), f"{tag}: output {i} differs between two calls"


def _report(fam):
    print("worst max |err| / bound so far:", {k: float(f"{v:.3g}") for k, v in RATIOS[fam].items()})


# ------------------------------------------------------------------------------------------------------------------------------ LayerNorm
def _ln_forward(ops, lp):
    """one sa_layernorm_fwd call; lp: None (as the network calls it) or the 16-bit type of the y_lp copy"""
    from synthanatomy_amd import _ffi
    x, w, b = ops["x"].to(DEV), ops["w"].to(DEV), ops["b"].to(DEV)
    R, C = x.shape
    y, stats = _nan(R, C), _nan(2 * R)
    y_lp = None if lp is None else _nan(R, C, dtype=cb.DT[lp])
    with _ffi.kernel_log() as names:
        _ffi.check(_ffi.lib().sa_layernorm_fwd(_ffi.ptr(x), _ffi.ptr(w), _ffi.ptr(b), _ffi.ptr(y), _ffi.ptr(y_lp), 0 if lp is None else _ffi.dtype_id(cb.DT[lp]),
                                               _ffi.ptr(stats), R, C, hb.EPS32, _ffi.stream()), "sa_layernorm_fwd")
        torch.cuda.synchronize()
    assert sorted(names) == ["layernorm_fwd_kernel"], names
    return y, stats, y_lp


def _ln_backward(ops, stats32):
    """sa_layernorm_bwd accumulating onto dw0 / db0: (dx, dw, db)"""
    from synthanatomy_amd import _ffi
    x, dy, w, st = ops["x"].to(DEV), ops["dy"].to(DEV), ops["w"].to(DEV), stats32.to(DEV)
    R, C = x.shape
    dx, dw, db = _nan(R, C), ops["dw0"].to(DEV), ops["db0"].to(DEV)
    with _ffi.kernel_log() as names:
        _ffi.check(_ffi.lib().sa_layernorm_bwd(_ffi.ptr(dy), _ffi.ptr(x), _ffi.ptr(w), _ffi.ptr(st), _ffi.ptr(dx), _ffi.ptr(dw), _ffi.ptr(db), R, C, _ffi.stream()),
                   "sa_layernorm_bwd")
        torch.cuda.synchronize()
    assert sorted(names) == ["layernorm_bwd_rows_kernel" if C <= 512 else "layernorm_bwd_kernel"], names        # the route head_bounds.ln_col_rule restates
    return dx, dw, db


def _ln_backward_det(ops, stats32):
    """the deterministic route of dw / db: sa_layernorm_dwprod, then engine.colsum_det (sa_colsum_det) of the products and of dy, onto dw0 / db0"""
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.engine import colsum_det
    x, dy, st = ops["x"].to(DEV), ops["dy"].to(DEV), stats32.to(DEV)
    R, C = x.shape
    prod, dw, db = _nan(R, C), ops["dw0"].to(DEV), ops["db0"].to(DEV)
    _ffi.check(_ffi.lib().sa_layernorm_dwprod(_ffi.ptr(dy), _ffi.ptr(x), _ffi.ptr(st), _ffi.ptr(prod), R, C, _ffi.stream()), "sa_layernorm_dwprod")
    colsum_det(prod, C, dw)
    colsum_det(dy, C, db)
    torch.cuda.synchronize()
    return None, dw, db


@pytest.mark.parametrize("R,C,off,sc", hb.LN_CASES, ids=hb.LN_IDS)
def test_layernorm_forward_within_fp64_bound(R, C, off, sc):
    ops = hb.draw_ln(R, C, off, sc)
    tag = f"[LN {R}x{C} off {off:g} x {sc:g}]"
    y, stats, _ = _ln_forward(ops, None)
    lps = {}
    for dt in ("bf16", "f16"):
        y2, stats2, lps[dt] = _ln_forward(ops, dt)
        _bit_equal(f"{tag} fwd with a {dt} copy", (y, stats), (y2, stats2))        # (the copy changes nothing else; each wave's order is fixed)
    hb.verify_ln_forward(f"{tag} fwd", ops, (y, stats, lps), RATIOS["ln"])
    _report("ln")


@pytest.mark.parametrize("R,C,off,sc", hb.LN_CASES, ids=hb.LN_IDS)
def test_layernorm_backward_within_fp64_bound(R, C, off, sc):
    ops = hb.draw_ln(R, C, off, sc)
    tag = f"[LN {R}x{C} off {off:g} x {sc:g}]"
    stats32 = hb.ln_backward_stats(ops)
    hb.verify_ln_backward(f"{tag} bwd atomic", ops, "atomic", stats32, _ln_backward(ops, stats32), RATIOS["ln"])
    got = _ln_backward_det(ops, stats32)
    _bit_equal(f"{tag} bwd det", got, _ln_backward_det(ops, stats32))
    hb.verify_ln_backward(f"{tag} bwd det", ops, "det", stats32, got, RATIOS["ln"])
    _report("ln")


# ------------------------------------------------------------------------------------------------------------------------------ cross-entropy
def _ce(ops, tgt, gscale, route, out):
    """route atomic: sa_cross_entropy accumulating onto loss0; route det: sa_cross_entropy_rows, then sa_sum_det (accumulate = 0) into a NaN-filled
    scalar, as losses/transformer.py does.  out None: dlogits = NULL.  Returns (loss [1], row_loss or None, grad or None)."""
    from synthanatomy_amd import _ffi
    lib = _ffi.lib()
    l, t = ops["l"].to(DEV), tgt.to(DEV)
    R, V = l.shape
    d = None if out is None else _nan(R, V, dtype=cb.DT[out])
    did = _ffi.SA_F32 if out is None else _ffi.dtype_id(cb.DT[out])
    with _ffi.kernel_log() as names:
        if route == "det":
            row_loss, acc = _nan(R), _nan(1)
            _ffi.check(lib.sa_cross_entropy_rows(_ffi.ptr(l), _ffi.ptr(t), R, V, _ffi.ptr(row_loss), _ffi.ptr(d), did, gscale, _ffi.stream()), "sa_cross_entropy_rows")
            _ffi.check(lib.sa_sum_det(_ffi.ptr(row_loss), R, _ffi.ptr(acc), 0, _ffi.stream()), "sa_sum_det")
        else:
            row_loss, acc = None, ops["loss0"].to(DEV)
            _ffi.check(lib.sa_cross_entropy(_ffi.ptr(l), _ffi.ptr(t), R, V, _ffi.ptr(acc), _ffi.ptr(d), did, gscale, _ffi.stream()), "sa_cross_entropy")
        torch.cuda.synchronize()
    assert sorted(names) == (["ce_rows_kernel", "sum_det_kernel"] if route == "det" else ["ce_kernel"]), names
    return acc, row_loss, d


@pytest.mark.parametrize("route", hb.CE_ROUTES)
@pytest.mark.parametrize("R,V,sc,off", hb.CE_CASES, ids=hb.CE_IDS)
def test_cross_entropy_within_fp64_bound(R, V, sc, off, route):
    ops = hb.draw_ce(R, V, sc, off)
    for name, key in hb.ce_variants(R, V):
        first = None
        for gscale in (1.0, hb.f32(1.0 / R)):
            for out in ("f32", "bf16"):
                tag = f"[CE {R}x{V} x {sc:g} off {off:g}{name} {route} gscale {gscale:.3g} {out}]"
                got = _ce(ops, ops[key], gscale, route, out)
                if route == "det":
                    _bit_equal(tag, got, _ce(ops, ops[key], gscale, route, out))
                    first = first or got
                    _bit_equal(f"{tag}: the loss does not depend on the gradient's type or scale", got[:2], first[:2])
                hb.verify_ce(tag, ops, ops[key], gscale, route, out, got, RATIOS["ce"])
        # dlogits = NULL (a forward without a gradient): the same loss
        tag = f"[CE {R}x{V} x {sc:g} off {off:g}{name} {route} no gradient]"
        got = _ce(ops, ops[key], 1.0, route, None)
        if route == "det":
            _bit_equal(f"{tag}: the loss does not depend on dlogits", got[:2], first[:2])
        hb.verify_ce(tag, ops, ops[key], 1.0, route, "f32", got, RATIOS["ce"])
    _report("ce")


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_celoss_module_within_fp64_bound(reduction, det):
    """losses.CELoss on logits [B, V, N] = [2, 130, 9]: the loss and logits.grad within the kernels' bounds.  The module multiplies the summed loss
    by its fp32 scale (1 / R for "mean"): 2 U |loss| on top (the rounding of the scale and of the product); the gradient is multiplied by the
    incoming gradient 1, exactly."""
    from synthanatomy_amd import debug
    from synthanatomy_amd.losses.transformer import CELoss
    B, V, N = 2, 130, 9
    R = B * N
    gen = torch.Generator().manual_seed(5)
    logits = torch.randn(B, V, N, generator=gen)
    target = torch.randint(0, V, (B, N), generator=gen)
    route = "det" if det else "atomic"
    scale = hb.f32(1.0 / R) if reduction == "mean" else 1.0
    ld = logits.to(DEV).requires_grad_(True)
    with debug.override(deterministic=det):
        loss = CELoss(reduction=reduction)(ld, target.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
    l, tgt = logits.transpose(1, 2).reshape(R, V).double(), target.reshape(R)
    ref = hb.ce_ref(l, tgt, scale)
    dterm, dgrad = hb.ce_bounds(l, ref, scale, "f32")
    rl = hb.ce_loss_ref(ref["term"], 0.0) * scale
    bl = hb.ce_loss_bound(ref["term"], dterm, 0.0, route) * scale + 2 * hb.U * rl.abs()
    tag = f"[CELoss {reduction} {route}]"
    wl = {"one-hot at t+1": hb.ce_loss_ref(hb.ce_ref(l, tgt, scale, shift_onehot=True)["term"], 0.0) * scale,
          "last row block dropped": hb.ce_loss_ref(ref["term"], 0.0, drop_last=hb.ce_loss_rule(R, route)[2]) * scale,
          "the other reduction": hb.ce_loss_ref(ref["term"], 0.0) * (1.0 if reduction == "mean" else 1.0 / R)}
    hb.within(f"{tag} loss", loss.detach().view(1), rl, bl, wl, RATIOS["ce"])
    wg = {"one-hot at t+1": hb.ce_ref(l, tgt, scale, shift_onehot=True)["grad"], "target of row r+1": hb.ce_ref(l, tgt, scale, roll_rows=True)["grad"],
          "the other reduction": hb.ce_ref(l, tgt, 1.0 if reduction == "mean" else 1.0 / R)["grad"],
          "not transposed back": ref["grad"].view(B, N, V).reshape(B, V, N).transpose(1, 2).reshape(R, V)}
    hb.within(f"{tag} grad", ld.grad.transpose(1, 2).reshape(R, V), ref["grad"], dgrad, wg, RATIOS["ce"])
    _report("ce")
