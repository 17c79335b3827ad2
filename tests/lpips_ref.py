"""Plain-torch fp64 restatement, on the CPU, of the 2.5D LPIPS-alex perceptual term and of the three loss classes around it:
the reference for tests/test_perceptual_losses_cpu.py / _gpu.py and the ``lpips.LPIPS`` stand-in of tests/golden/make_goldens_perceptual.py.

It restates ``lpips.LPIPS(net='alex', version='0.1', lpips=True, spatial=False)`` in eval mode from its published description -- UNPINNED against upstream
(the package is not installed anywhere this project is built).  It holds its own copies of the seeded weight draw and of the slice draw, and

* ``rounded=True``: the "bf16 model" -- weights and every layer's input rounded to bf16 (straight-through for the gradient), everything else fp64;
* four planted defects for the witnesses (``defect=``): ``"pad_shift"`` the scaling layer's shift leaked into conv1's padding, ``"ceil_pool"`` ceil
  instead of floor extents in the pools, ``"no_projection"`` the projection term of the normalisation's gradient dropped everywhere,
  ``"swap_hw"`` H and W swapped in the slices of the second view.

One deliberate difference from upstream's autograd: where a feature vector is all zero the square root's gradient is taken as 0 (upstream: NaN).
"""
import numpy as np
import torch
import torch.nn.functional as F

ALEX = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
CONV_KEYS = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")
LIN_KEYS = tuple(f"lin{i}.model.1.weight" for i in range(5))
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
PERMUTES = ((0, 2, 1, 3, 4), (0, 3, 1, 2, 4), (0, 4, 1, 2, 3))
DEFECTS = ("pad_shift", "ceil_pool", "no_projection", "swap_hw")


def draw_weights(seed):
    """the package's seeded stand-in weights (losses/lpips.py: random_state_dict), restated"""
    gen = torch.Generator().manual_seed(int(seed))
    sd = {}
    for key, (ci, co, k, _, _) in zip(CONV_KEYS, ALEX):
        sd[key + ".weight"] = (torch.randn(co, ci, k, k, generator=gen, dtype=torch.float64) * (2.0 / (ci * k * k)) ** 0.5).float()
        sd[key + ".bias"] = (torch.randn(co, generator=gen, dtype=torch.float64) * 0.1).float()
    for key, (_, co, _, _, _) in zip(LIN_KEYS, ALEX):
        sd[key] = torch.rand(1, co, 1, 1, generator=gen, dtype=torch.float64).float()
    return sd


def draw_slices(seed, step, view, n_slices, n_keep):
    """the package's slice draw (losses/lpips.py: draw_slices), restated"""
    if n_keep >= n_slices:
        return np.arange(n_slices, dtype=np.int32)
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF, int(view)])))
    return np.sort(rng.permutation(n_slices)[:n_keep]).astype(np.int32)


def _bf16(t):
    return t.float().bfloat16().double()


def _rnd(t, rounded):          # straight-through rounding of a layer's input
    return t + (_bf16(t.detach()) - t.detach()) if rounded else t


def _unit(f, defect):
    s = (f * f).sum(1, keepdim=True)
    pos = s > 0
    r = torch.where(pos, s, torch.ones_like(s)).sqrt() * pos          # sqrt with the subgradient 0 at 0
    if defect == "no_projection":
        r = r.detach()
    return f / (r + 1e-10)


def features(x, sd, normalize=True, rounded=False, defect=None):
    """the five ReLU taps of slices x [S, 1, h, w] (float64)"""
    w = [sd[k + ".weight"].double() for k in CONV_KEYS]
    b = [sd[k + ".bias"].double() for k in CONV_KEYS]
    if rounded:
        w = [_bf16(t) for t in w]
    shift = torch.tensor(SHIFT, dtype=torch.float64).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float64).view(1, 3, 1, 1)
    u = 2 * x - 1 if normalize else x
    if defect == "pad_shift":        # pad u with zeros BEFORE scaling: padded taps become -shift / scale
        s = (F.pad(u, (2, 2, 2, 2)) - shift) / scale
        f = torch.relu(F.conv2d(_rnd(s, rounded), w[0], b[0], stride=4))
    else:
        f = torch.relu(F.conv2d(_rnd((u - shift) / scale, rounded), w[0], b[0], stride=4, padding=2))
    ceil = defect == "ceil_pool"
    taps = [_rnd(f, rounded)]
    f = torch.relu(F.conv2d(F.max_pool2d(taps[-1], 3, 2, ceil_mode=ceil), w[1], b[1], padding=2))
    taps.append(_rnd(f, rounded))
    f = torch.relu(F.conv2d(F.max_pool2d(taps[-1], 3, 2, ceil_mode=ceil), w[2], b[2], padding=1))
    taps.append(_rnd(f, rounded))
    f = torch.relu(F.conv2d(taps[-1], w[3], b[3], padding=1))
    taps.append(_rnd(f, rounded))
    f = torch.relu(F.conv2d(taps[-1], w[4], b[4], padding=1))
    taps.append(_rnd(f, rounded))
    return taps


def distance(x0, x1, sd, normalize=True, rounded=False, defect=None):
    """LPIPS per slice: [S]"""
    f0 = features(x0, sd, normalize, rounded, defect)
    f1 = features(x1, sd, normalize, rounded, defect)
    d = 0
    for a, b, key in zip(f0, f1, LIN_KEYS):
        lin = sd[key].double().view(1, -1, 1, 1)
        d = d + (lin * (_unit(a, defect) - _unit(b, defect)) ** 2).sum(1).mean((1, 2))
    return d


class LPIPS(torch.nn.Module):
    """stand-in for ``lpips.LPIPS`` with the call signature the reference's loss classes use: ``forward(in0, in1, normalize=...)`` -> [S, 1, 1, 1]"""
    seed = 0

    def __init__(self, **kwargs):
        super().__init__()
        assert kwargs.get("net", "alex") == "alex" and not kwargs.get("spatial", False)
        self.sd = draw_weights(type(self).seed)

    def forward(self, in0, in1, normalize=False):
        return distance(in0.double(), in1.double(), self.sd, normalize).view(-1, 1, 1, 1)


def slices(vol, view, defect=None):
    """[B, 1, D, H, W] -> the reference's batchified view [B n, 1, h, w]"""
    s = vol.permute(*PERMUTES[view]).contiguous()
    s = s.view(-1, *s.shape[2:])
    if defect == "swap_hw" and view == 1:
        s = s.transpose(-1, -2)
    return s


def perceptual_terms(pred, y, sd, ids=None, views=(0, 1, 2), factor=0.001, normalize=True, rounded=False, defect=None, chunk=64):
    """[perceptual_factor * mean over the kept slices of LPIPS] per view (float64, differentiable to pred); ids[i] = the kept slice ids of views[i]
    (None: all).  Slices go through in chunks (memory); ``defect`` as in the module docstring."""
    out = []
    for i, v in enumerate(views):
        ys, ps = slices(y.double(), v, defect), slices(pred.double(), v, defect)
        keep = torch.arange(ys.shape[0]) if ids is None or ids[i] is None else torch.as_tensor(np.asarray(ids[i]), dtype=torch.long)
        tot = 0
        for lo in range(0, keep.numel(), chunk):
            k = keep[lo:lo + chunk]
            tot = tot + distance(ys[k], ps[k], sd, normalize, rounded, defect).sum()
        out.append(tot / keep.numel() * factor)
    return out


def loss(kind, pred, y, q, sd, ids=None, factor=0.001, spectral_factor=1.0, rounded=False, defect=None):
    """The three classes with their defaults: kind = perceptual | jukebox_perceptual | hartley_perceptual.  Returns (loss, summaries) in float64,
    differentiable to pred; summaries under the reference's keys (quantization entries left out)."""
    import fourier_ref
    pred64, y64 = pred.double(), y.double()
    summ = {}
    total = 0
    if kind == "jukebox_perceptual":
        amp = lambda t: torch.fft.fftn(t, dim=(1, 2, 3, 4), norm="ortho").abs()      # noqa: E731
        total = F.mse_loss(amp(pred64), amp(y64)) * spectral_factor
        summ["Loss-Spectral-Reconstruction"] = total
    elif kind == "hartley_perceptual":
        # (fourier_ref returns value and gradient; the autograd form of the same term: 0.5 mse of the weighted Hartley transforms)
        Yp, Yy = (torch.fft.fftn(t, dim=(1, 2, 3, 4), norm="ortho") for t in (pred64, y64))
        D, H, W = pred.shape[2:]
        wh = fourier_ref.hartley_weight(D, H, W)       # half spectrum along W; mirror it to the full one
        full = torch.cat([wh, wh[..., 1:(W + 1) // 2].flip(-1)], -1) if W > 1 else wh
        hp, hy = (Yp.real - Yp.imag) * full, (Yy.real - Yy.imag) * full
        total = 0.5 * F.mse_loss(hp, hy) * spectral_factor
        summ["Loss-Hartley-Reconstruction"] = total
    else:
        assert kind == "perceptual", kind
    for i, t in enumerate(perceptual_terms(pred, y, sd, ids, factor=factor, rounded=rounded, defect=defect)):
        summ[f"Loss-Perceptual_{i}-Reconstruction"] = t
        total = total + t
    l2 = F.mse_loss(pred64, y64)
    summ["Loss-MSE-Reconstruction"] = l2
    total = total + l2
    for ql in q:
        total = total + float(ql)
    return total, summ
