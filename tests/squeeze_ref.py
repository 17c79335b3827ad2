"""Plain-torch fp64 restatement, on the CPU, of the 2.5D LPIPS-squeeze perceptual term and of ``BaselineLoss`` around it: the
reference for tests/test_baseline_loss_cpu.py / _gpu.py and the ``lpips.LPIPS`` stand-in of tests/golden/make_goldens_baseline.py.

It restates ``lpips.LPIPS(net='squeeze', version='0.1', lpips=True, spatial=False)`` in eval mode over torchvision's SqueezeNet-1.1 ``features`` from
their published sources with plain ``F.conv2d``, ``F.max_pool2d(ceil_mode=True)`` and ``torch.cat`` -- RESTATED, UNPINNED against upstream (neither
package is installed anywhere this project is built).  It holds its own copy of the seeded weight draw, and

* ``rounded=True``: the "bf16 model" -- weights and every layer's input rounded to bf16 (straight-through for the gradient), everything else fp64;
* four planted defects for the witnesses (``defect=``): ``"floor_pool"`` floor instead of ceil extents in the pools, ``"swap_expand"`` the two expand
  halves concatenated in the wrong order, ``"pad_conv1"`` padding 1 on the first layer, ``"swap_axial_coronal"`` the axial and coronal permutes exchanged.

As in tests/lpips_ref.py, the square root's gradient is taken as 0 where a feature vector is all zero (upstream: NaN).
"""
import numpy as np
import torch
import torch.nn.functional as F

from lpips_ref import PERMUTES, SCALE, SHIFT, _bf16, _rnd, _unit, draw_slices  # noqa: F401  (shared with the alex restatement)

# (state-dict prefix, cin, squeeze, expand1x1, expand3x3); a ceil-mode pool sits in front of features 3, 6 and 9; taps after features 0, 4, 7, 9, 10, 11, 12
FIRES = (("net.slice2.3", 64, 16, 64, 64), ("net.slice2.4", 128, 16, 64, 64), ("net.slice3.6", 128, 32, 128, 128), ("net.slice3.7", 256, 32, 128, 128),
         ("net.slice4.9", 256, 48, 192, 192), ("net.slice5.10", 384, 48, 192, 192), ("net.slice6.11", 384, 64, 256, 256), ("net.slice7.12", 512, 64, 256, 256))
POOL_BEFORE = (0, 2, 4)
TAP_AFTER = (1, 3, 4, 5, 6, 7)
TAP_CHANNELS = (64, 128, 256, 384, 384, 512, 512)
LIN_KEYS = tuple(f"lin{i}.model.1.weight" for i in range(7))
DEFECTS = ("floor_pool", "swap_expand", "pad_conv1", "swap_axial_coronal")
BASELINE_VIEWS = (0, 2, 1)      # sagittal, axial, coronal: upstream's order
SUMMARY_VIEW_KEYS = ("Loss-Perceptual_Sagittal-Reconstruction", "Loss-Perceptual_Axial-Reconstruction", "Loss-Perceptual_Coronal-Reconstruction")


def shapes():
    out = {"net.slice1.0.weight": (64, 3, 3, 3), "net.slice1.0.bias": (64,)}
    for key, ci, s, e1, e3 in FIRES:
        out[f"{key}.squeeze.weight"], out[f"{key}.squeeze.bias"] = (s, ci, 1, 1), (s,)
        out[f"{key}.expand1x1.weight"], out[f"{key}.expand1x1.bias"] = (e1, s, 1, 1), (e1,)
        out[f"{key}.expand3x3.weight"], out[f"{key}.expand3x3.bias"] = (e3, s, 3, 3), (e3,)
    for key, c in zip(LIN_KEYS, TAP_CHANNELS):
        out[key] = (1, c, 1, 1)
    return out


def draw_weights(seed):
    """the package's seeded stand-in squeeze weights (losses/lpips_squeeze.py: random_state_dict), restated"""
    gen = torch.Generator().manual_seed(int(seed))
    sd = {}
    for key, shape in shapes().items():
        if key in LIN_KEYS:
            sd[key] = torch.rand(shape, generator=gen, dtype=torch.float64).float()
        elif key.endswith(".weight"):
            sd[key] = (torch.randn(shape, generator=gen, dtype=torch.float64) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5).float()
        else:
            sd[key] = (torch.randn(shape, generator=gen, dtype=torch.float64) * 0.1).float()
    return sd


def features(x, sd, normalize=False, rounded=False, defect=None):
    """the seven ReLU taps of slices x [S, 1, h, w] (float64)"""
    def wb(key):
        w = sd[key + ".weight"].double()
        return (_bf16(w) if rounded else w), sd[key + ".bias"].double()

    shift = torch.tensor(SHIFT, dtype=torch.float64).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float64).view(1, 3, 1, 1)
    u = 2 * x - 1 if normalize else x
    w, b = wb("net.slice1.0")
    f = torch.relu(F.conv2d(_rnd((u - shift) / scale, rounded), w, b, stride=2, padding=1 if defect == "pad_conv1" else 0))
    f = _rnd(f, rounded)
    taps = [f]
    ceil = defect != "floor_pool"
    for i, (key, *_rest) in enumerate(FIRES):
        if i in POOL_BEFORE:
            f = F.max_pool2d(f, 3, 2, ceil_mode=ceil)
        w, b = wb(key + ".squeeze")
        z = _rnd(torch.relu(F.conv2d(f, w, b)), rounded)
        w1, b1 = wb(key + ".expand1x1")
        w3, b3 = wb(key + ".expand3x3")
        halves = [torch.relu(F.conv2d(z, w1, b1)), torch.relu(F.conv2d(z, w3, b3, padding=1))]
        f = _rnd(torch.cat(halves[::-1] if defect == "swap_expand" else halves, 1), rounded)
        if i in TAP_AFTER:
            taps.append(f)
    return taps


def distance(x0, x1, sd, normalize=False, rounded=False, defect=None):
    """LPIPS per slice: [S]"""
    f0 = features(x0, sd, normalize, rounded, defect)
    f1 = features(x1, sd, normalize, rounded, defect)
    d = 0
    for a, b, key in zip(f0, f1, LIN_KEYS):
        lin = sd[key].double().view(1, -1, 1, 1)
        d = d + (lin * (_unit(a, defect) - _unit(b, defect)) ** 2).sum(1).mean((1, 2))
    return d


class LPIPS(torch.nn.Module):
    """stand-in for ``lpips.LPIPS(net="squeeze")`` with the call signature the reference's BaselineLoss uses: ``forward(in0, in1)`` -> [S, 1, 1, 1]"""
    seed = 0

    def __init__(self, **kwargs):
        super().__init__()
        assert kwargs.get("net") == "squeeze" and not kwargs.get("spatial", False)
        self.sd = draw_weights(type(self).seed)

    def forward(self, in0, in1, normalize=False):
        return distance(in0.double(), in1.double(), self.sd, normalize).view(-1, 1, 1, 1)


def slices(vol, view, defect=None):
    """[B, 1, D, H, W] -> the reference's batchified view [B n, 1, h, w]"""
    if defect == "swap_axial_coronal":
        view = {0: 0, 1: 2, 2: 1}[view]
    s = vol.permute(*PERMUTES[view]).contiguous()
    return s.view(-1, *s.shape[2:])


def perceptual_means(pred, y, sd, ids=None, views=BASELINE_VIEWS, normalize=False, rounded=False, defect=None, chunk=64):
    """[mean over the kept slices of LPIPS] per view (float64, differentiable to pred); ids[i] = the kept slice ids of views[i] (None: all)"""
    out = []
    for i, v in enumerate(views):
        ys, ps = slices(y.double(), v, defect), slices(pred.double(), v, defect)
        keep = torch.arange(ys.shape[0]) if ids is None or ids[i] is None else torch.as_tensor(np.asarray(ids[i]), dtype=torch.long)
        tot = 0
        for lo in range(0, keep.numel(), chunk):
            k = keep[lo:lo + chunk]
            tot = tot + distance(ys[k], ps[k], sd, normalize, rounded, defect).sum()
        out.append(tot / keep.numel())
    return out


def baseline_ids(shape, seed, step, n_slices=512):
    """the kept slice ids of BaselineLoss' three views, in BASELINE_VIEWS order"""
    B, _, D, H, W = shape
    return [draw_slices(seed, step, v, B * (D, H, W)[v], min(n_slices, B * (D, H, W)[v])) for v in BASELINE_VIEWS]


def baseline_loss(pred, y, q, sd, ids=None, pixel_factor=1.0, perceptual_factor=0.002, fft_factor=1.0, rounded=False, defect=None):
    """BaselineLoss with its defaults: (loss, summaries) in float64, differentiable to pred; summaries under the reference's keys (commitment left out)"""
    pred64, y64 = pred.double(), y.double()
    summ = {}
    l1 = F.l1_loss(pred64, y64) * pixel_factor
    summ["Loss-MAE-Reconstruction"] = l1
    amp = lambda t: torch.fft.fftn((t + 1.0) / 2.0, norm="ortho").abs()      # noqa: E731  (no dim: all five axes)
    fl = F.mse_loss(amp(y64), amp(pred64)) * fft_factor
    summ["Loss-Jukebox-Reconstruction"] = fl
    means = perceptual_means(pred, y, sd, ids, rounded=rounded, defect=defect)
    for k, m in zip(SUMMARY_VIEW_KEYS, means):
        summ[k] = m
    pl = (means[0] + means[1] + means[2]) * perceptual_factor
    summ["Loss-Perceptual-Reconstruction"] = pl
    total = l1 + fl + pl
    for ql in q:
        total = total + float(ql)
    return total, summ
