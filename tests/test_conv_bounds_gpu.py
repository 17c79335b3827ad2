"""GPU: every dispatchable variant of the implicit-GEMM convolution family (and the one-channel first / last layers), selected by name, against
an fp64 CPU reference under the element-wise bound of tests/conv_bounds.py -- with a planted-defect witness per case that the same output
must fail.  Run with -s to read each row's kernel names, max |err| / A and witness."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_bounds as cb
from grad_stand_in import Grads

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(16, torch.get_num_threads()))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _ncdhw(t):            # channels-last [N, D, H, W, C] -> [N, C, D, H, W], float64 on the CPU
    return t.detach().double().cpu().permute(0, 4, 1, 2, 3)


def _cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _operand(shape, dt, gen, scale=1.0, relu=False):
    t = torch.randn(shape, generator=gen) * scale
    if relu:
        t = torch.relu(t)
    return cb.rounded(t, dt)


def _both16(t):
    """values exact in bf16 AND f16 (the f16 forward chain's first layer: f16 taps forward, bf16 taps in the weight gradient)"""
    t = torch.where(t.abs() < 2.0 ** -10, torch.zeros_like(t), t)
    return cb.rounded(t, "bf16")


def _kernels(names, case):
    got = sorted(names)
    print(f"[{case['id']}] kernels: {', '.join(got)}")
    for want in case["kernels"]:
        assert any(n.startswith(want) for n in got), f"{case['id']}: expected a launch of {want!r}, the log holds {got}"


def _epilogue(z, case, add=None, mask=None, slope=cb.SLOPE32, mask_ge=False):
    """the reference epilogue on the fp64 pre-activation z (bias included); returns (out, lip, extra).  slope / mask_ge: the LeakyReLU witnesses
    (slope 0: what ReLU or the sign mask would give; mask_ge: the mask tested with >= 0, which lets +0.0 and -0.0 through)"""
    epi = case["epi"]
    if epi == "lrelu":
        return torch.where(z > 0, z, slope * z), 1.0, None
    if epi == "mask_lrelu":
        keep = (mask >= 0) if mask_ge else (mask > 0)
        return z * torch.where(keep, 1.0, slope), 1.0, None
    if epi in ("none", "bias"):
        return z, 1.0, None
    if epi == "relu":
        return torch.relu(z), 1.0, None
    if epi == "gelu":
        return F.gelu(z), cb.GELU_LIP, 4 * cb.U32 * z.abs()          # (+ a few ulps of erff)
    if epi == "add_relu":
        return torch.relu(z + add), 1.0, None
    if epi == "mask":
        return (z + add) * (mask > 0), 1.0, None
    raise KeyError(epi)


def _ffi_consts():
    from synthanatomy_amd import _ffi
    return dict(none=_ffi.ACT_NONE, bias=_ffi.ACT_NONE, relu=_ffi.ACT_RELU, gelu=_ffi.ACT_GELU, add_relu=_ffi.ACT_RELU, mask=_ffi.ACT_NONE,
                lrelu=_ffi.ACT_LRELU, mask_lrelu=_ffi.ACT_NONE)


def _padded(t, width):
    """channels-last t zero-padded to `width` channels (engine.cast_pad's layout: a cin = 1 input, a cout = 1 gradient)"""
    return t if t.shape[-1] == width else F.pad(t, (0, width - t.shape[-1]))


def _plant_zeros(mask, z):
    """+0.0 and -0.0 in the channels-last mask at the eight voxels where |z| (fp64, NCDHW) is largest, alternating"""
    flat = mask.view(-1)
    top = torch.topk(_cl(z).reshape(-1).abs(), 8).indices
    flat[top[0::2]] = 0.0
    flat[top[1::2]] = -0.0


def _lrelu_witnesses(what, got, z, case, A, out, mask64=None):
    """a LeakyReLU row must also fail the reference with slope 0 and, for the data-gradient mask, the one that tests mask >= 0 -- on every 61st
    element and the planted zeros (failing on a part is failing; the whole of a cells256 volume would cost half its row again)"""
    if case["epi"] not in ("lrelu", "mask_lrelu"):
        return
    sel = torch.arange(0, z.numel(), 61)
    if mask64 is not None:
        sel = torch.cat([sel, (mask64.reshape(-1) == 0).nonzero().flatten()])
    got, z, A, mask64 = (None if t is None else t.reshape(-1)[sel] for t in (got, z, A, mask64))
    cb.assert_witness_fails(what + " [slope 0]", got, _epilogue(z, case, None, mask64, slope=0.0)[0], A, out)
    if case["epi"] == "mask_lrelu":
        cb.assert_witness_fails(what + " [mask >= 0]", got, _epilogue(z, case, None, mask64, mask_ge=True)[0], A, out)


def _check16(what, got, ref, A, wit, out, lip=1.0, extra=None):
    cb.assert_bounded(what, got, ref, A, wit, out, lip, extra)
    if out != "f32":   # a truncating store must not pass either
        cb.assert_bounded(what + " [truncation witness]", got, ref, A, cb.truncated(ref, out), out, lip, extra)


# ---------------------------------------------------------------------------------------------------------------------------- ConvOp cases
def _weights(case, gen):
    kind, cin, cout, k = case["kind"], case["cin"], case["cout"], case["k"]
    wshape = (cout, cin, k, k, k) if kind == "conv" else (cin, cout, k, k, k)
    fan = cin * k ** 3
    w = _operand(wshape, case["fwd"] if case["op"] == "fprop" else case["dt"], gen, fan ** -0.5)
    b = torch.randn(cout, generator=gen) * 0.1
    return w, b


def _fprop(case, gen):
    from synthanatomy_amd import _ffi, debug, engine
    kind, s, p, N, dims = case["kind"], case["s"], case["p"], case["N"], case["dims"]
    fdt, out = case["fwd"], case["out"]
    w, b = _weights(case, gen)
    x = _operand((N, *dims, case["cin"]), fdt, gen, relu=case["epi"] == "mask")
    op = engine.ConvOp(kind, case["cin"], case["cout"], case["k"], s, p, w.to(DEV), b.to(DEV), cb.DT[case["dt"]], fwd_dtype=cb.DT[fdt])
    od = op.out_dims(dims)
    add = mask = None
    if case["epi"] in ("add_relu", "mask"):
        add = _operand((N, *od, case["cout"]), fdt, gen)
    if case["epi"] == "mask":
        mask = _operand((N, *od, case["cout"]), case["dt"], gen)
    use_bias = case["epi"] != "none"
    with debug.override(**case["flags"]), _ffi.kernel_log() as names:
        y = op.fprop(_padded(x, op.cs_in()).to(DEV).to(cb.DT[fdt]), act=_ffi_consts()[case["epi"]], addend=None if add is None else add.to(DEV).to(cb.DT[fdt]),
                     add_before_act=case["epi"] == "add_relu", mask=None if mask is None else mask.to(DEV).to(cb.DT[case["dt"]]),
                     mask_mode=_ffi.MASK_POS if mask is not None else _ffi.MASK_NONE, out_dtype=cb.DT[out], use_bias=use_bias,
                     out_channels_stride=case["out_stride"], slope=cb.SLOPE32)
        torch.cuda.synchronize()
    _kernels(names, case)
    x64, w64 = _ncdhw(x), w.double()
    b64 = b.double() if use_bias else None
    z = cb.conv_ref(kind, x64, w64, b64, s, p)
    A = cb.conv_ref(kind, x64.abs(), w64.abs(), None if b64 is None else b64.abs(), s, p)
    if kind == "conv":   # witness: the last input channel dropped
        dz = F.conv3d(x64[:, -1:], w64[:, -1:], stride=s, padding=p)
    else:
        dz = F.conv_transpose3d(x64[:, -1:], w64[-1:], stride=s, padding=p)
    add64 = None if add is None else _ncdhw(add)
    mask64 = None if mask is None else _ncdhw(mask)
    if add64 is not None:
        A = A + add64.abs()
    ref, lip, extra = _epilogue(z, case, add64, mask64)
    wit, _, _ = _epilogue(z - dz, case, add64, mask64)
    _check16(f"[{case['id']}] y", _ncdhw(y), ref, A, wit, out, lip, extra)
    _lrelu_witnesses(f"[{case['id']}] y", _ncdhw(y), z, case, A, out)


def _dgrad(case, gen):
    from synthanatomy_amd import _ffi, debug, engine
    kind, s, p, N, dims, k = case["kind"], case["s"], case["p"], case["N"], case["dims"], case["k"]
    dt, out = case["dt"], case["out"]
    w, b = _weights(case, gen)
    op = engine.ConvOp(kind, case["cin"], case["cout"], k, s, p, w.to(DEV), b.to(DEV), cb.DT[dt])
    od = op.out_dims(dims)
    g = _operand((N, *od, case["cout"]), dt, gen)
    add = mask = None
    if case["epi"] == "mask":           # the residual block's data gradient: + the incoming gradient, masked by the layer input's sign
        add = _operand((N, *dims, case["cin"]), dt, gen)
        mask = _operand((N, *dims, case["cin"]), dt, gen)
    g64, w64 = _ncdhw(g), w.double()
    z = cb.dgrad_ref(kind, g64, w64, s, p, dims)
    mode = _ffi.MASK_POS if mask is not None else _ffi.MASK_NONE
    if case["epi"] == "mask_lrelu":     # the discriminator's data gradient: LeakyReLU'(the layer input), both signs and both zeros in the mask
        mask = _operand((N, *dims, case["cin"]), dt, gen)
        _plant_zeros(mask, z)
        mode = _ffi.MASK_LRELU
    with debug.override(**case["flags"]), _ffi.kernel_log() as names:
        # (a gradient whose channel count is no multiple of the vector arrives zero-padded to one, as engine.cast_pad leaves it)
        dx = op.dgrad(_padded(g, -(-case["cout"] // op.vec) * op.vec).to(DEV).to(cb.DT[dt]), dims, addend=None if add is None else add.to(DEV).to(cb.DT[dt]),
                      mask=None if mask is None else mask.to(DEV).to(cb.DT[dt]), mask_mode=mode, out_dtype=cb.DT[out], slope=cb.SLOPE32)
        torch.cuda.synchronize()
    _kernels(names, case)
    A = cb.dgrad_ref(kind, g64.abs(), w64.abs(), s, p, dims)
    if kind == "conv":   # witness: the last channel of the incoming gradient dropped
        dz = cb.dgrad_ref(kind, g64[:, -1:], w64[-1:], s, p, dims)
    else:
        dz = cb.dgrad_ref(kind, g64[:, -1:], w64[:, -1:], s, p, dims)
    add64 = None if add is None else _ncdhw(add)
    if add64 is not None:
        A = A + add64.abs()
    mask64 = None if mask is None else _ncdhw(mask)
    ref, lip, extra = _epilogue(z, case, add64, mask64)
    wit, _, _ = _epilogue(z - dz, case, add64, mask64)
    _check16(f"[{case['id']}] dx", _ncdhw(dx), ref, A, wit, out, lip, extra)
    _lrelu_witnesses(f"[{case['id']}] dx", _ncdhw(dx), z, case, A, out, mask64)


def _wgrad_inputs(case, gen):
    kind, N, dims, dt = case["kind"], case["N"], case["dims"], case["dt"]
    w, b = _weights(case, gen)
    from synthanatomy_amd import engine
    od = engine.ConvOp(kind, case["cin"], case["cout"], case["k"], case["s"], case["p"], w, b, cb.DT[dt]).out_dims(dims)
    x = _operand((N, *dims, case["cin"]), dt, gen, relu=case["op"] == "bwd1x1")
    g = _operand((N, *od, case["cout"]), dt, gen)
    dw0 = torch.randn(w.shape, generator=gen) * 0.5 if case["acc"] else torch.zeros(w.shape)
    db0 = torch.randn(case["cout"], generator=gen) if case["acc"] else torch.zeros(case["cout"])
    return w, b, x, g, dw0, db0


def _wgrad_refs(case, w, x, g, dw0, db0):
    kind, s, p, k = case["kind"], case["s"], case["p"], case["k"]
    x64, g64 = _ncdhw(x), _ncdhw(g)
    dw = cb.wgrad_ref(kind, x64, g64, w.shape, s, p) + dw0.double()
    A = cb.wgrad_ref(kind, x64.abs(), g64.abs(), w.shape, s, p) + dw0.double().abs()
    wit = dw - cb.wgrad_last_plane(kind, x64, g64, w.shape, s, p, k)   # witness: the last depth plane of the last image left out of the reduction
    db = g64.sum(dim=(0, 2, 3, 4)) + db0.double()
    Ab = g64.abs().sum(dim=(0, 2, 3, 4)) + db0.double().abs()
    return dw, A, wit, db, Ab, g64[-1:, :, -1].sum(dim=(0, 2, 3))


def _check_wgrad(tag, dw, db, refs, is_convT):
    rdw, A, wit, rdb, Ab, last = refs
    cb.assert_bounded(f"{tag} dw", dw, rdw, A, wit)
    plane = last if not is_convT else None
    if plane is not None:      # bias gradient: the rows of the last output plane of the last image
        cb.assert_bounded(f"{tag} db", db, rdb, Ab, rdb - plane)
    else:
        ok, ratio, worst = cb.check(db, rdb, Ab)
        assert ok, f"{tag} db: max|err|/A = {ratio:.2e} at {worst}"
        print(f"  {tag} db: max|err|/A = {ratio:.2e}")


def _wgrad_helpers(op, x, g, names, with_db):
    """The reduce and column-sum kernels that sa_conv_wgrad launches after the weight-gradient kernel.  They leave no kernel-log entry, so which
    ones run is restated from conv_wgrad_impl (csrc/conv_wgrad.hip): the wide reduce for <= 8 tiles and >= 128 splits (the split count from the
    workspace the library asks for); a stand-alone column sum when the bias gradient is not fused -- over the dense output, or over the rows of
    a strided geometry.  Call under the same debug flags as the launch."""
    import ctypes
    from synthanatomy_amd import _ffi, debug
    lib = _ffi.lib()
    did = _ffi.dtype_id(op.dtype)
    T = "float" if op.dtype == torch.float32 else "bf16_t"
    no_fused_db = bool(lib.sa_get_debug_flags() & debug.LIB_FLAGS["no_fused_db"])
    unfused_kernel = any(n.startswith("conv_wgrad_kernel") for n in names)     # (the global-load kernel never sums the bias gradient)
    out = set()
    for pl in op._get_plans(x.shape[0], tuple(x.shape[1:4]), op.cout, g.shape[-1])["wgrad"]:
        gm = pl.geom
        ntiles = -(-(pl.ntaps * gm.Cin) // 128) * -(-gm.cout_valid // 128)
        splits = lib.sa_conv_wgrad_workspace_bytes(ctypes.byref(gm), did) // (ntiles * 128 * 128 * 4)
        out.add("wgrad_reduce_wide_kernel" if ntiles <= 8 and splits >= 128 else "wgrad_reduce_kernel")
        if with_db and not debug.deterministic() and (op.dtype != torch.bfloat16 or no_fused_db or unfused_kernel):
            dense = all(gm.out_mult[d] == 1 and gm.out_off[d] == 0 for d in range(3)) and (gm.Dm, gm.Hm, gm.Wm) == (gm.Do, gm.Ho, gm.Wo)
            out.add(f"colsum_kernel<{T}>" if dense else f"colsum_geom_kernel<{T}>")
    return out


def _wgrad(case, gen):
    from synthanatomy_amd import _ffi, debug, engine
    dt = cb.DT[case["dt"]]
    w, b, x, g, dw0, db0 = _wgrad_inputs(case, gen)
    op = engine.ConvOp(case["kind"], case["cin"], case["cout"], case["k"], case["s"], case["p"], w.to(DEV), b.to(DEV), dt)
    dw, db = dw0.to(DEV), db0.to(DEV)
    dx = None
    with debug.override(**case["flags"]):
        with _ffi.kernel_log() as names:
            if case["op"] == "bwd1x1":
                dx = engine.conv1x1_backward(op, x.to(DEV).to(dt), g.to(DEV).to(dt), dw, db)
                assert dx is not None
            else:
                gp = _padded(g, -(-case["cout"] // op.vec) * op.vec)      # (a cout = 1 gradient arrives 8 wide with one valid channel)
                op.wgrad(_padded(x, op.cs_in()).to(DEV).to(dt), gp.to(DEV).to(dt), dw, db)
            torch.cuda.synchronize()
        helpers = _wgrad_helpers(op, x, gp if case["op"] != "bwd1x1" else g, names, True)      # (the log is read when its block closes)
    print(f"[{case['id']}] reduce / column-sum kernels by rule: {', '.join(sorted(helpers))}")
    _kernels(list(names) + sorted(helpers), case)
    refs = _wgrad_refs(case, w, x, g, dw0, db0)
    if case["kind"] == "convT":
        # the convT weight gradient's rows are input voxels: the bias gradient's witness would need the output planes -- checked without one
        _check_wgrad(f"[{case['id']}]", dw, db, refs, True)
    else:
        _check_wgrad(f"[{case['id']}]", dw, db, refs, False)
    if dx is not None:   # the fused ReLU-masked data gradient of the 1x1x1 layer
        g64, w64, x64 = _ncdhw(g), w.double(), _ncdhw(x)
        m = (x64 > 0).double()
        z = F.conv_transpose3d(g64, w64) * m
        A = F.conv_transpose3d(g64.abs(), w64.abs()) * m
        wit = z - F.conv_transpose3d(g64[:, -1:], w64[-1:]) * m
        _check16(f"[{case['id']}] dx", _ncdhw(dx), z, A, wit, "bf16")


# ---------------------------------------------------------------------------------------------------------------------------- residual block
def _resblock(case, gen):
    from synthanatomy_amd import _ffi, debug
    from synthanatomy_amd.networks.vqvae.baseline import ResidualLayer, _Act, _ResStage
    fdt, N, dims = case["fwd"], case["N"], case["dims"]
    mod = ResidualLayer(128, 128, 0.0)
    w3 = _operand((128, 128, 3, 3, 3), fdt, gen, (128 * 27) ** -0.5)
    w1 = _operand((128, 128, 1, 1, 1), fdt, gen, 128 ** -0.5)
    b1, b2 = torch.randn(128, generator=gen) * 0.1, torch.randn(128, generator=gen) * 0.1
    with torch.no_grad():
        mod[0].weight.copy_(w3), mod[0].bias.copy_(b1), mod[3].weight.copy_(w1), mod[3].bias.copy_(b2)
    st = _ResStage(mod.to(DEV).eval(), in_act=True, dtype=torch.bfloat16, fwd_dtype=cb.DT[fdt] if fdt != "bf16" else None)
    x = _operand((N, *dims, 128), fdt, gen, relu=True)
    tape = []
    with debug.override(**case["flags"]), _ffi.kernel_log() as names:
        y = st.fwd(x.to(DEV).to(cb.DT[fdt]), tape)
        torch.cuda.synchronize()
    _kernels(names, case)
    ys = None
    if isinstance(y, _Act):
        y, ys = y.f, y.s
    h = tape[0][1]
    x64 = _ncdhw(x)
    w3d, w1d = w3.double(), w1.double()
    z1 = F.conv3d(x64, w3d, b1.double(), padding=1)
    A1 = F.conv3d(x64.abs(), w3d.abs(), b1.double().abs(), padding=1)
    h_ref = torch.relu(z1)
    h_wit = torch.relu(z1 - F.conv3d(x64[:, -1:], w3d[:, -1:], padding=1))
    # f16 chain: the stored bf16 h (and the bf16 copy of y) is rounded from the f16 value the 1x1x1 consumed -- two roundings, so half an f16 ulp
    # more than one rounding to bf16 (a tie at the f16 value goes to even in bf16: seen 0.517735 -> 0.517578 -> 0.515625)
    dbl = (lambda r: cb.half_ulp(r, "f16")) if fdt == "f16" else (lambda r: None)
    _check16(f"[{case['id']}] h", _ncdhw(h), h_ref, A1, h_wit, "bf16", 1.0, dbl(h_ref))
    # the 1x1x1 operand is h rounded to the forward operand type: its error propagates through |w1|
    slack = cb.GAMMA * A1 + 2 * cb.U32 * h_ref
    dh = slack + cb.half_ulp(h_ref + slack, fdt)
    z2 = F.conv3d(h_ref, w1d, b2.double()) + x64
    A2 = F.conv3d(h_ref, w1d.abs(), b2.double().abs()) + x64.abs()
    extra = F.conv3d(dh, w1d.abs())
    y_ref = torch.relu(z2)
    y_wit = torch.relu(z2 - F.conv3d(h_ref[:, -1:], w1d[:, -1:]))        # witness: the last hidden channel dropped
    # (no truncation witness for y: the propagated rounding of h is of the order of y's own half ulp)
    cb.assert_bounded(f"[{case['id']}] y", _ncdhw(y), y_ref, A2, y_wit, fdt, 1.0, extra)
    if ys is not None:
        cb.assert_bounded(f"[{case['id']}] y (bf16 copy)", _ncdhw(ys), y_ref, A2, y_wit, "bf16", 1.0, extra + cb.half_ulp(y_ref, "f16"))


# ---------------------------------------------------------------------------------------------------------------------------- one-channel layers
def _Grads(params, gen, acc):
    return Grads(params, [torch.randn(p.shape, generator=gen) * 0.5 for p in params] if acc else None)


def _corner_tap(w):
    t = torch.zeros_like(w)
    t[..., 0, 0, 0] = w[..., 0, 0, 0]
    return t


def _conv1(case, gen):
    from synthanatomy_amd import _ffi, debug
    from synthanatomy_amd.networks.vqvae.baseline import _Act, _Conv1Stage
    fdt, dt, N, dims, cout = case["fwd"], case["dt"], case["N"], case["dims"], case["cout"]
    mod = nn.Conv3d(1, cout, 4, 2, 1)
    w = _both16(torch.randn(cout, 1, 4, 4, 4, generator=gen) * 0.125) if dt != "f32" else torch.randn(cout, 1, 4, 4, 4, generator=gen) * 0.125
    b = torch.randn(cout, generator=gen) * 0.1
    with torch.no_grad():
        mod.weight.copy_(w), mod.bias.copy_(b)
    mod = mod.to(DEV)
    st = _Conv1Stage(mod, _ffi.ACT_RELU, cb.DT[dt], fwd_dtype=cb.DT[fdt] if fdt != dt else None)
    x = torch.randn(N, *dims, generator=gen)
    x = _both16(x) if dt != "f32" else x
    od = tuple(d // 2 for d in dims)
    G = _operand((N, *od, cout), dt, gen)
    gr = _Grads([mod.weight, mod.bias], gen, case["acc"])
    tape = []
    with debug.override(**case["flags"]), _ffi.kernel_log() as names:
        y = st.fwd(x.to(DEV), tape)
        st.bwd(G.to(DEV).to(cb.DT[dt]), tape[0], gr)
        torch.cuda.synchronize()
    _kernels(names, case)
    ys = None
    if isinstance(y, _Act):
        y, ys = y.f, y.s
    x64, w64 = x.double()[:, None], w.double()
    z = F.conv3d(x64, w64, b.double(), stride=2, padding=1)
    A = F.conv3d(x64.abs(), w64.abs(), b.double().abs(), stride=2, padding=1)
    wit = torch.relu(z - F.conv3d(x64, _corner_tap(w64), stride=2, padding=1))     # witness: one corner tap dropped
    _check16(f"[{case['id']}] y", _ncdhw(y), torch.relu(z), A, wit, fdt)
    if ys is not None:
        _check16(f"[{case['id']}] y (bf16 copy)", _ncdhw(ys), torch.relu(z), A, wit, "bf16")
    dw0, db0 = gr.init[id(mod.weight)], gr.init[id(mod.bias)]
    refs = _wgrad_refs(dict(case, cin=1), w, _cl(x[:, None]), G, dw0, db0)
    _check_wgrad(f"[{case['id']}]", gr.buf(mod.weight), gr.buf(mod.bias), refs, False)


def _convt1(case, gen):
    from synthanatomy_amd import _ffi, debug
    from synthanatomy_amd.networks.vqvae.baseline import _ConvT1Stage
    dt, N, dims = case["dt"], case["N"], case["dims"]
    mod = nn.ConvTranspose3d(128, 1, 4, 2, 1)
    w = _operand((128, 1, 4, 4, 4), dt, gen, 0.05)
    b = torch.randn(1, generator=gen) * 0.1
    with torch.no_grad():
        mod.weight.copy_(w), mod.bias.copy_(b)
    mod = mod.to(DEV)
    st = _ConvT1Stage(mod, in_act=True, dtype=cb.DT[dt])
    x = _operand((N, *dims, 128), dt, gen, relu=True)
    od = tuple(2 * d for d in dims)
    G = _operand((N, *od, 1), dt, gen)          # (the GEMM routes gather the gradient taps in the compute dtype)
    gr = _Grads([mod.weight, mod.bias], gen, case["acc"])
    tape = []
    with debug.override(**case["flags"]), _ffi.kernel_log() as names:
        y = st.fwd(x.to(DEV).to(cb.DT[dt]), tape)
        dx = st.bwd(G.to(DEV), tape[0], gr)
        torch.cuda.synchronize()
    _kernels(names, case)
    x64, w64, G64 = _ncdhw(x), w.double(), _ncdhw(G)
    z = F.conv_transpose3d(x64, w64, b.double(), stride=2, padding=1)
    A = F.conv_transpose3d(x64.abs(), w64.abs(), b.double().abs(), stride=2, padding=1)
    wit = z - F.conv_transpose3d(x64[:, -1:], w64[-1:], stride=2, padding=1)       # witness: the last input channel dropped
    _check16(f"[{case['id']}] y", _ncdhw(y), z, A, wit, "f32")
    m = (x64 > 0).double()
    zx = F.conv3d(G64, w64, stride=2, padding=1) * m
    Ax = F.conv3d(G64.abs(), w64.abs(), stride=2, padding=1) * m
    witx = zx - F.conv3d(G64, _corner_tap(w64), stride=2, padding=1) * m          # witness: one corner tap dropped
    _check16(f"[{case['id']}] dx", _ncdhw(dx), zx, Ax, witx, dt)
    dw0, db0 = gr.init[id(mod.weight)], gr.init[id(mod.bias)]
    refs = _wgrad_refs(case, w, x, G, dw0, db0)
    _check_wgrad(f"[{case['id']}]", gr.buf(mod.weight), gr.buf(mod.bias), refs, True)


_RUN = dict(fprop=_fprop, dgrad=_dgrad, wgrad=_wgrad, bwd1x1=_wgrad, resblock=_resblock, conv1=_conv1, convt1=_convt1)


@pytest.mark.parametrize("case", cb.CASES, ids=[c["id"] for c in cb.CASES])
def test_conv_variant_within_fp64_bound(case):
    gen = torch.Generator().manual_seed(sum(map(ord, case["id"])))
    _RUN[case["op"]](case, gen)


# ---------------------------------------------------------------------------------------------------------------------------- split counts
_CHILD = r"""
import json, sys, torch
sys.path.insert(0, sys.argv[1])
from synthanatomy_amd import _ffi, debug, engine
d = torch.load(sys.argv[2])
out = {}
for name, flags in (("halo", {}), ("dma", {"no_halo": True})):
    op = engine.ConvOp("conv", 128, 128, 3, 1, 1, d["w"].cuda(), d["b"].cuda(), torch.bfloat16)
    dw, db = d["dw0"].cuda(), d["db0"].cuda()
    with debug.override(**flags), _ffi.kernel_log() as names:
        op.wgrad(d["x"].cuda().to(torch.bfloat16), d["g"].cuda().to(torch.bfloat16), dw, db)
        torch.cuda.synchronize()
    out[name] = (dw.cpu(), db.cpu(), sorted(names))
torch.save(out, sys.argv[3])
"""


def test_wgrad_split_counts_in_fresh_processes(tmp_path):
    """The split-count tunables (SA_WGRAD_HALO_SPLITS, SA_WGRAD_ROWS / SA_WGRAD_MIN_BLOCKS, SA_PP_DBG bit 16384 = halo9<16>) are read once per process:
    the same saved operands through the halo and the LDS-DMA weight gradient in one fresh child per setting, each result under the same bound."""
    case = dict(next(c for c in cb.CASES if c["id"] == "wgrad_halo9_cout256_acc"), cout=128)
    gen = torch.Generator().manual_seed(7)
    w, b, x, g, dw0, db0 = _wgrad_inputs(case, gen)
    src = tmp_path / "operands.pt"
    torch.save(dict(w=w, b=b, x=x, g=g, dw0=dw0, db0=db0), src)
    refs = _wgrad_refs(case, w, x, g, dw0, db0)
    for tag, env, kernel in cb.SPLIT_ENVS:
        dst = tmp_path / f"{tag}.pt"
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(src), str(dst)], env={**os.environ, **env}, cwd=ROOT, timeout=300,
                           capture_output=True, text=True)
        assert r.returncode == 0, f"{tag} ({env}): child exited with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        res = torch.load(dst)
        for name, (dw, db, names) in res.items():
            print(f"[split {tag} {json.dumps(env)} / {name}] kernels: {', '.join(names)}")
            if name == "halo":
                assert kernel in names, (tag, names)
            else:
                assert any(n.startswith("conv_wgrad_dma_kernel") for n in names), (tag, names)
            _check_wgrad(f"[split {tag} / {name}]", dw, db, refs, False)
