"""float64 NumPy restatement of ``pytorch_msssim.ms_ssim`` 0.2.1 for [B, C, D, H, W] volumes -- the contract of DESIGN §7.3 that the HIP metric
(``synthanatomy_amd.metrics.ms_ssim``, csrc/metrics.hip) is held to.  The package is not installed on the build machines, so this is a restatement,
not a pinned oracle.  ``odd_padding`` and the window's sigma exist so that tests can build witnesses with a planted mistake."""
import numpy as np

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window(win_size, win_sigma=1.5):
    """The package's 1-D Gaussian (``_fspecial_gauss_1d``), built with torch's fp32 CPU ops as it is, then widened.  The exact fp32 taps matter:
    their sum is 1 only to within an ulp, and at w = 11 an ulp of difference in the taps moves a level's mean cs by ~1e-5 (sigma^2 is a small
    difference of two filtered values)."""
    import torch
    coords = torch.arange(win_size, dtype=torch.float32)
    coords -= win_size // 2
    g = torch.exp(-(coords ** 2) / (2 * win_sigma ** 2))
    g /= g.sum()
    return g.numpy().astype(np.float64)


def gaussian_filter(v, g):
    """Valid-mode separable filter along D, then H, then W of [B, C, D, H, W]."""
    w = len(g)
    for ax in (2, 3, 4):
        n = v.shape[ax] - w + 1
        out = np.zeros(v.shape[:ax] + (n,) + v.shape[ax + 1:])
        for t in range(w):
            out += g[t] * np.take(v, np.arange(t, t + n), axis=ax)
        v = out
    return v


def avg_pool(v, odd_padding=True):
    """avg_pool3d(kernel 2, stride 2, padding = side % 2, count_include_pad=True): an odd side gets one zero on both ends."""
    for ax in (2, 3, 4):
        s = v.shape[ax]
        if s % 2 and odd_padding:
            pad = [(0, 0)] * 5
            pad[ax] = (1, 1)
            v = np.pad(v, pad)
            s += 2
        n = (s - 2) // 2 + 1
        a = np.take(v, np.arange(0, 2 * n, 2), axis=ax)
        b = np.take(v, np.arange(1, 2 * n, 2), axis=ax)
        v = a + b
    return v / 8.0


def ssim_cs(x, y, g, data_range=1.0, K=(0.01, 0.03)):
    """Per-(b, c) means of the ssim and cs maps of one level, each [B, C]."""
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    mx, my = gaussian_filter(x, g), gaussian_filter(y, g)
    sxx = gaussian_filter(x * x, g) - mx * mx
    syy = gaussian_filter(y * y, g) - my * my
    sxy = gaussian_filter(x * y, g) - mx * my
    cs = (2 * sxy + C2) / (sxx + syy + C2)
    ssim = (2 * mx * my + C1) / (mx * mx + my * my + C1) * cs
    return ssim.reshape(ssim.shape[:2] + (-1,)).mean(-1), cs.reshape(cs.shape[:2] + (-1,)).mean(-1)


def ms_ssim(X, Y, data_range=1.0, win_size=11, win_sigma=1.5, weights=WEIGHTS, K=(0.01, 0.03), odd_padding=True, levels_out=None):
    """Per-batch-element MS-SSIM ([B], the mean over channels: ``size_average=False``).  ``levels_out`` (a list) receives the per-level
    [B, C, 2] (ssim, cs) means."""
    x = np.asarray(X, dtype=np.float64)
    y = np.asarray(Y, dtype=np.float64)
    if x.shape != y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {x.shape} and {y.shape}.")
    if win_size % 2 != 1:
        raise ValueError("Window size should be odd.")
    assert min(x.shape[-2:]) > (win_size - 1) * 2 ** 4
    g = window(win_size, win_sigma)
    L = len(weights)
    vals = []
    for lv in range(L):
        ssim, cs = ssim_cs(x, y, g, data_range, K)
        if levels_out is not None:
            levels_out.append(np.stack([ssim, cs], -1))
        if lv < L - 1:
            vals.append(np.maximum(cs, 0.0))
            x, y = avg_pool(x, odd_padding), avg_pool(y, odd_padding)
    vals.append(np.maximum(ssim, 0.0))
    w = np.asarray(weights, dtype=np.float32).astype(np.float64)
    out = np.prod(np.stack(vals, 0) ** w[:, None, None], axis=0)
    return out.mean(1)


def torch_ms_ssim(X, Y, data_range=1.0, win_size=11, win_sigma=1.5, weights=WEIGHTS, K=(0.01, 0.03), levels_out=None):
    """The package's algorithm written with torch ops in the input's dtype and on its device: conv3d with the 1-D window along each axis
    (groups=C), avg_pool3d with padding = side % 2.  The yardstick for what fp32 arithmetic in the package's order costs."""
    import torch
    import torch.nn.functional as F
    C = X.shape[1]
    g = torch.from_numpy(window(win_size, win_sigma).astype(np.float32)).to(X.device, X.dtype)
    win = g.reshape(1, 1, 1, 1, -1).repeat(C, 1, 1, 1, 1)
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2

    def filt(v):
        for i in range(3):
            v = F.conv3d(v, win.transpose(2 + i, -1), groups=C)
        return v

    mcs = []
    for lv in range(len(weights)):
        mu1, mu2 = filt(X), filt(Y)
        mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
        s1 = filt(X * X) - mu1_sq
        s2 = filt(Y * Y) - mu2_sq
        s12 = filt(X * Y) - mu1_mu2
        cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
        ssim_map = ((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs_map
        ssim, cs = torch.flatten(ssim_map, 2).mean(-1), torch.flatten(cs_map, 2).mean(-1)
        if levels_out is not None:
            levels_out.append(torch.stack([ssim, cs], -1))
        if lv < len(weights) - 1:
            mcs.append(torch.relu(cs))
            pad = [s % 2 for s in X.shape[2:]]
            X, Y = F.avg_pool3d(X, kernel_size=2, padding=pad), F.avg_pool3d(Y, kernel_size=2, padding=pad)
    w = X.new_tensor(weights)
    return torch.prod(torch.stack(mcs + [torch.relu(ssim)], 0) ** w.view(-1, 1, 1), dim=0).mean(1)
