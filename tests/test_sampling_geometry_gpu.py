"""GPU: ConvOp and the one-channel stages on sampling geometries beyond k4 s2 p1 / even extents -- odd extents, kernels 2 and 3, dilation, output_padding --
against fp64 torch on the CPU under the element-wise bound of tests/conv_bounds.py, each with a planted-defect witness (a dropped channel) that must fail.
Run with -s to read max |err| / A per row."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_bounds as cb
from grad_stand_in import Grads

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(16, torch.get_num_threads()))
DEV = "cuda"
N = 2

# (id, kind, (k, s, p, op, d), extents, cin, cout, operand types)
ROWS = [
    ("conv_k4s2p1_odd", "conv", (4, 2, 1, 0, 1), (9, 11, 7), 16, 24, ("f32", "bf16")),
    ("conv_k3s2p1", "conv", (3, 2, 1, 0, 1), (7, 10, 9), 16, 24, ("f32", "bf16")),
    ("conv_k2s2p0_unread_plane", "conv", (2, 2, 0, 0, 1), (7, 8, 9), 16, 24, ("f32", "bf16")),
    ("conv_k3s1p2d2", "conv", (3, 1, 2, 0, 2), (6, 7, 9), 16, 24, ("f32", "bf16")),
    ("conv_k4s2p1_odd_c128", "conv", (4, 2, 1, 0, 1), (31, 33, 65), 128, 64, ("bf16",)),
    ("convT_k4s2p1op1", "convT", (4, 2, 1, 1, 1), (4, 5, 6), 16, 24, ("f32", "bf16")),
    ("convT_k3s2p1op1", "convT", (3, 2, 1, 1, 1), (4, 5, 6), 16, 24, ("f32", "bf16")),
    ("convT_k2s2p0", "convT", (2, 2, 0, 0, 1), (4, 5, 6), 16, 24, ("f32", "bf16")),
    ("convT_k3s1p2d2", "convT", (3, 1, 2, 0, 2), (5, 6, 7), 16, 24, ("f32", "bf16")),
]
CASES = [(r, dt, what) for r in ROWS for dt in r[6] for what in ("fprop", "dgrad", "wgrad")]


def _ncdhw(t):
    return t.detach().double().cpu().permute(0, 4, 1, 2, 3)


def _operand(shape, dt, gen, scale=1.0, relu=False):
    t = torch.randn(shape, generator=gen) * scale
    return cb.rounded(torch.relu(t) if relu else t, dt)


def fwd_ref(kind, x, w, b, tup):
    k, s, p, op, d = tup
    if kind == "conv":
        return F.conv3d(x, w, b, stride=s, padding=p, dilation=d)
    return F.conv_transpose3d(x, w, b, stride=s, padding=p, output_padding=op, dilation=d)


def dgrad_ref(kind, g, w, tup, idims):
    k, s, p, op, d = tup
    if kind == "conv":
        opad = tuple(idims[a] - ((g.shape[2 + a] - 1) * s - 2 * p + d * (k - 1) + 1) for a in range(3))
        return F.conv_transpose3d(g, w, stride=s, padding=p, output_padding=opad, dilation=d)
    return F.conv3d(g, w, stride=s, padding=p, dilation=d)[:, :, :idims[0], :idims[1], :idims[2]]


def wgrad_ref(kind, x, g, wshape, tup):
    k, s, p, op, d = tup
    if kind == "conv":
        return torch.nn.grad.conv3d_weight(x, wshape, g, stride=s, padding=p, dilation=d)
    return torch.nn.grad.conv3d_weight(g, wshape, x, stride=s, padding=p, dilation=d)      # convT: x = conv3d(g, w) is its adjoint


def _check16(what, got, ref, A, wit, out):
    cb.assert_bounded(what, got, ref, A, wit, out)
    if out != "f32":
        cb.assert_bounded(what + " [truncation witness]", got, ref, A, cb.truncated(ref, out), out)


def test_references_agree_with_autograd():
    """the closed-form references above against torch's own autograd, at one dilated and one output-padded tuple (fp64, CPU)"""
    gen = torch.Generator().manual_seed(3)
    for kind, tup, idims in (("conv", (3, 2, 1, 0, 1), (7, 10, 9)), ("conv", (2, 2, 0, 0, 1), (7, 8, 9)), ("convT", (3, 2, 1, 1, 1), (4, 5, 6)), ("convT", (3, 1, 2, 0, 2), (5, 6, 7))):
        k = tup[0]
        x = torch.randn(2, 3, *idims, generator=gen, dtype=torch.float64, requires_grad=True)
        w = torch.randn((5, 3, k, k, k) if kind == "conv" else (3, 5, k, k, k), generator=gen, dtype=torch.float64, requires_grad=True)
        y = fwd_ref(kind, x, w, None, tup)
        g = torch.randn(y.shape, generator=gen, dtype=torch.float64)
        gx, gw = torch.autograd.grad(y, (x, w), g)
        assert torch.allclose(dgrad_ref(kind, g, w.detach(), tup, idims), gx, atol=1e-10)
        assert torch.allclose(wgrad_ref(kind, x.detach(), g, w.shape, tup), gw, atol=1e-10)


@pytest.mark.parametrize("row,dt,what", CASES, ids=[f"{r[0]}-{dt}-{what}" for r, dt, what in CASES])
def test_convop_geometry_within_fp64_bound(row, dt, what):
    from synthanatomy_amd import _ffi, engine
    rid, kind, tup, idims, cin, cout, _ = row
    k, s, p, op_, d = tup
    gen = torch.Generator().manual_seed(sum(map(ord, rid + dt)))
    wshape = (cout, cin, k, k, k) if kind == "conv" else (cin, cout, k, k, k)
    w = _operand(wshape, dt, gen, (cin * k ** 3) ** -0.5)
    b = torch.randn(cout, generator=gen) * 0.1
    tdt = cb.DT[dt]
    op = engine.ConvOp(kind, cin, cout, k, s, p, w.to(DEV), b.to(DEV), tdt, output_pad=op_, dilation=d)
    od = op.out_dims(idims)
    assert od == tuple(fwd_ref(kind, torch.zeros(1, cin, *idims), w, None, tup).shape[2:])
    w64 = w.double()
    tag = f"[{rid} {dt}]"
    in_ch = (lambda t: t[:, -1:]) if kind == "conv" else (lambda t: t[-1:])        # the weight slice of the last input channel
    out_ch = (lambda t: t[-1:]) if kind == "conv" else (lambda t: t[:, -1:])       # ... of the last output channel
    if what == "fprop":        # bias + ReLU
        x = _operand((N, *idims, cin), dt, gen)
        y = op.fprop(x.to(DEV).to(tdt), act=_ffi.ACT_RELU)
        torch.cuda.synchronize()
        x64 = _ncdhw(x)
        z = fwd_ref(kind, x64, w64, b.double(), tup)
        A = fwd_ref(kind, x64.abs(), w64.abs(), b.double().abs(), tup)
        wit = torch.relu(z - fwd_ref(kind, x64[:, -1:], in_ch(w64), None, tup))      # witness: the last input channel dropped
        _check16(f"{tag} y", _ncdhw(y), torch.relu(z), A, wit, dt)
    elif what == "dgrad":      # with the sign mask of the layer's input
        g = _operand((N, *od, cout), dt, gen)
        mask = _operand((N, *idims, cin), dt, gen)
        dx = op.dgrad(g.to(DEV).to(tdt), idims, mask=mask.to(DEV).to(tdt), mask_mode=_ffi.MASK_POS)
        torch.cuda.synchronize()
        g64, m = _ncdhw(g), (_ncdhw(mask) > 0).double()
        z = dgrad_ref(kind, g64, w64, tup, idims) * m
        A = dgrad_ref(kind, g64.abs(), w64.abs(), tup, idims) * m
        wit = z - dgrad_ref(kind, g64[:, -1:], out_ch(w64), tup, idims) * m          # witness: the last gradient channel dropped
        _check16(f"{tag} dx", _ncdhw(dx), z, A, wit, dt)
        if rid == "conv_k2s2p0_unread_plane":     # no window reads the last depth plane (7 = 2 * 3 + 1): its gradient is exactly zero
            assert float(dx[:, -1].abs().max()) == 0.0 and float(z[:, :, -1].abs().max()) == 0.0
    else:                      # + db, accumulating into non-zero buffers
        x = _operand((N, *idims, cin), dt, gen)
        g = _operand((N, *od, cout), dt, gen)
        dw0, db0 = torch.randn(wshape, generator=gen) * 0.5, torch.randn(cout, generator=gen)
        dw, db = dw0.to(DEV), db0.to(DEV)
        op.wgrad(x.to(DEV).to(tdt), g.to(DEV).to(tdt), dw, db)
        torch.cuda.synchronize()
        x64, g64 = _ncdhw(x), _ncdhw(g)
        rdw = wgrad_ref(kind, x64, g64, wshape, tup) + dw0.double()
        A = wgrad_ref(kind, x64.abs(), g64.abs(), wshape, tup) + dw0.double().abs()
        x0 = x64.clone()
        x0[:, -1] = 0                                                                   # witness: the last input channel dropped
        cb.assert_bounded(f"{tag} dw", dw, rdw, A, wgrad_ref(kind, x0, g64, wshape, tup) + dw0.double())
        rdb = g64.sum(dim=(0, 2, 3, 4)) + db0.double()
        Ab = g64.abs().sum(dim=(0, 2, 3, 4)) + db0.double().abs()
        cb.assert_bounded(f"{tag} db", db, rdb, Ab, rdb - g64[-1, :, -1].sum(dim=(1, 2)))     # witness: the last output plane of the last image left out


# ---------------------------------------------------------------------------------------------------------------------------- one-channel stages
def _both16(t):
    t = torch.where(t.abs() < 2.0 ** -10, torch.zeros_like(t), t)
    return cb.rounded(t, "bf16")


def _corner_tap(w):
    t = torch.zeros_like(w)
    t[..., 0, 0, 0] = w[..., 0, 0, 0]
    return t


@pytest.mark.parametrize("cout,dt", [(128, "bf16"), (64, "f32")], ids=str)
@pytest.mark.parametrize("tup", [(3, 2, 1, 0, 1), (2, 2, 0, 0, 1)], ids=str)
def test_conv1_stage_taps_route(tup, cout, dt):
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.networks.vqvae.baseline import _Conv1Stage
    k, s, p, _, d = tup
    dims = (21, 27, 35)
    gen = torch.Generator().manual_seed(k * 1000 + cout)
    mod = nn.Conv3d(1, cout, k, s, p, dilation=d)
    w = torch.randn(cout, 1, k, k, k, generator=gen) * k ** -1.5
    x = torch.randn(N, *dims, generator=gen)
    if dt != "f32":
        w, x = _both16(w), _both16(x)
    b = torch.randn(cout, generator=gen) * 0.1
    with torch.no_grad():
        mod.weight.copy_(w), mod.bias.copy_(b)
    mod = mod.to(DEV)
    assert _Conv1Stage.applicable(mod)
    st = _Conv1Stage(mod, _ffi.ACT_RELU, cb.DT[dt])
    x64, w64 = x.double()[:, None], w.double()
    z = fwd_ref("conv", x64, w64, b.double(), tup)
    G = _operand((N, *z.shape[2:], cout), dt, gen)
    gr = Grads([mod.weight, mod.bias])
    tape = []
    with _ffi.kernel_log() as names:
        y = st.fwd(x.to(DEV), tape)
        st.bwd(G.to(DEV).to(cb.DT[dt]), tape[0], gr)
        torch.cuda.synchronize()
    print(sorted(names))
    assert any(n.startswith("taps_unfold_kernel") for n in names), names
    A = fwd_ref("conv", x64.abs(), w64.abs(), b.double().abs(), tup)
    wit = torch.relu(z - fwd_ref("conv", x64, _corner_tap(w64), None, tup))             # witness: one corner tap dropped
    _check16(f"[conv1 {tup} {dt}] y", _ncdhw(y), torch.relu(z), A, wit, dt)
    G64 = _ncdhw(G)
    rdw, Aw = wgrad_ref("conv", x64, G64, w.shape, tup), wgrad_ref("conv", x64.abs(), G64.abs(), w.shape, tup)
    x0 = x64.clone()
    x0[-1, :, 0] = 0                                          # witness: the first depth plane of the last image dropped (k2 s2 p0 never reads the last of 21)
    cb.assert_bounded(f"[conv1 {tup} {dt}] dw", gr.buf(mod.weight), rdw, Aw, wgrad_ref("conv", x0, G64, w.shape, tup))
    rdb, Ab = G64.sum(dim=(0, 2, 3, 4)), G64.abs().sum(dim=(0, 2, 3, 4))
    cb.assert_bounded(f"[conv1 {tup} {dt}] db", gr.buf(mod.bias), rdb, Ab, rdb - G64[-1, :, -1].sum(dim=(1, 2)))


@pytest.mark.parametrize("C,dt", [(128, "bf16"), (64, "f32")], ids=str)
@pytest.mark.parametrize("tup", [(4, 2, 1, 1, 1), (3, 2, 1, 1, 1), (2, 2, 0, 0, 1)], ids=str)
def test_convt1_stage_taps_route(tup, C, dt):
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.networks.vqvae.baseline import _ConvT1Stage
    k, s, p, op, d = tup
    dims = (7, 18, 17)          # 4 284 cells in two images >= GEMM_MIN_CELLS
    gen = torch.Generator().manual_seed(k * 1000 + C)
    mod = nn.ConvTranspose3d(C, 1, k, s, p, output_padding=op, dilation=d)
    w = _operand((C, 1, k, k, k), dt, gen, 0.05)
    b = torch.randn(1, generator=gen) * 0.1
    with torch.no_grad():
        mod.weight.copy_(w), mod.bias.copy_(b)
    mod = mod.to(DEV)
    assert _ConvT1Stage.applicable(mod)
    st = _ConvT1Stage(mod, in_act=True, dtype=cb.DT[dt])
    x = _operand((N, *dims, C), dt, gen, relu=True)
    x64, w64 = _ncdhw(x), w.double()
    z = fwd_ref("convT", x64, w64, b.double(), tup)
    G = _operand((N, *z.shape[2:], 1), dt, gen)
    gr = Grads([mod.weight, mod.bias])
    tape = []
    with _ffi.kernel_log() as names:
        y = st.fwd(x.to(DEV).to(cb.DT[dt]), tape)
        dx = st.bwd(G.to(DEV), tape[0], gr)
        torch.cuda.synchronize()
        gr2 = Grads([mod.weight, mod.bias])
        assert st.bwd(G.to(DEV), tape[0], gr2, wgrad_only=True) is None                 # (BaselineVQVAE.last_layer_grad)
        torch.cuda.synchronize()
    print(sorted(names))
    assert any(n.startswith("taps_fold_kernel") for n in names) and any(n.startswith("taps_unfold_kernel") for n in names), names
    assert tuple(y.shape) == (N, *z.shape[2:], 1)
    A = fwd_ref("convT", x64.abs(), w64.abs(), b.double().abs(), tup)
    wit = z - fwd_ref("convT", x64[:, -1:], w64[-1:], None, tup)                         # witness: the last input channel dropped
    _check16(f"[convt1 {tup} {dt}] y", _ncdhw(y), z, A, wit, "f32")
    G64, m = _ncdhw(G), (x64 > 0).double()
    zx = dgrad_ref("convT", G64, w64, tup, dims) * m
    Ax = dgrad_ref("convT", G64.abs(), w64.abs(), tup, dims) * m
    witx = zx - dgrad_ref("convT", G64, _corner_tap(w64), tup, dims) * m                 # witness: one corner tap dropped
    _check16(f"[convt1 {tup} {dt}] dx", _ncdhw(dx), zx, Ax, witx, dt)
    rdw, Aw = wgrad_ref("convT", x64, G64, w.shape, tup), wgrad_ref("convT", x64.abs(), G64.abs(), w.shape, tup)
    x0 = x64.clone()
    x0[-1, :, -1] = 0                                                                       # witness: the last depth plane of the last image dropped
    witw = wgrad_ref("convT", x0, G64, w.shape, tup)
    cb.assert_bounded(f"[convt1 {tup} {dt}] dw", gr.buf(mod.weight), rdw, Aw, witw)
    cb.assert_bounded(f"[convt1 {tup} {dt}] dw (wgrad_only)", gr2.buf(mod.weight), rdw, Aw, witw)
    rdb, Ab = G64.sum().reshape(1), G64.abs().sum().reshape(1)
    cb.assert_bounded(f"[convt1 {tup} {dt}] db", gr.buf(mod.bias), rdb, Ab, rdb - G64[-1, :, -1].sum().reshape(1))
