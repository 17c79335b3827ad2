"""Validation metrics.  ``ms_ssim`` has the signature and defaults of ``pytorch_msssim.ms_ssim`` (0.2.1) and runs the fused HIP path
(``sa_ms_ssim``, csrc/metrics.hip).  Only 5-D inputs are in scope; there is no CPU fallback."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from .. import _ffi

DEFAULT_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MAX_WIN = 11        # csrc/metrics.hip: SSIM_MAX_WIN
MAX_LEVELS = 8      # csrc/metrics.hip: SSIM_MAX_LEVELS


def gaussian_window(win_size: int, win_sigma: float) -> torch.Tensor:
    """The package's ``_fspecial_gauss_1d``: exp(-c^2 / (2 sigma^2)) over c = arange(w) - w // 2, normalised, in fp32 on the CPU."""
    coords = torch.arange(win_size, dtype=torch.float32)
    coords -= win_size // 2
    g = torch.exp(-(coords ** 2) / (2 * win_sigma ** 2))
    g /= g.sum()
    return g


def _ms_ssim(X: torch.Tensor, Y: torch.Tensor, data_range=255, win_size=11, win_sigma=1.5, win: Optional[torch.Tensor] = None,
             weights: Optional[Sequence[float]] = None, K=(0.01, 0.03), level_means: bool = False):
    """(per-batch-element MS-SSIM [B], and with ``level_means`` the per-level means [levels, B, C, 2] = (ssim, cs)) from one ``sa_ms_ssim`` call."""
    if not X.shape == Y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {X.shape} and {Y.shape}.")
    if X.dim() != 5:
        raise ValueError(f"Input images should be 5-d tensors [B, C, D, H, W] (the 2-d path is out of scope), but got {X.shape}")
    if min(X.shape[2:]) < 2:
        raise ValueError(f"spatial sides of 1 (the package squeezes them) are out of scope, got {X.shape}")
    if win is not None:
        win_size = win.shape[-1]
        rows = win.detach().float().cpu().reshape(-1, win_size)
        if not bool((rows == rows[0]).all()):
            raise ValueError("a window that differs between channels is not supported")
        g = rows[0].contiguous()
    if not (win_size % 2 == 1):
        raise ValueError("Window size should be odd.")
    smaller_side = min(X.shape[-2:])
    assert smaller_side > (win_size - 1) * (2 ** 4), "Image size should be larger than %d due to the 4 downsamplings in ms-ssim" % (
        (win_size - 1) * (2 ** 4))
    if win is None:
        g = gaussian_window(win_size, win_sigma)
    w = [float(v) for v in (DEFAULT_WEIGHTS if weights is None else (weights.tolist() if torch.is_tensor(weights) else weights))]
    levels = len(w)
    if not 3 <= win_size <= MAX_WIN or not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"sa_ms_ssim covers window sizes 3..{MAX_WIN} and 1..{MAX_LEVELS} levels, got win_size={win_size}, {levels} levels")
    sides = list(X.shape[2:])
    for lv in range(levels):
        if min(sides) < win_size:
            raise ValueError(f"level {lv} has sides {sides}, shorter than the window ({win_size}): the package would skip smoothing there, "
                             "which is out of scope")
        sides = [(s + 1) // 2 for s in sides]
    _ffi.require_gpu()
    x = X.float().contiguous()
    y = Y.float().contiguous().to(x.device)
    B, C, D, H, W = x.shape
    K1, K2 = K
    c1, c2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    lib = _ffi.lib()
    nbytes = lib.sa_ms_ssim_workspace_bytes(B, C, D, H, W, win_size, levels)
    _ffi.check(nbytes if nbytes < 0 else 0, "sa_ms_ssim_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    lm = torch.empty(levels, B, C, 2, dtype=torch.float32, device=x.device) if level_means else None
    win_c = (ctypes.c_float * win_size)(*g.tolist())
    w_c = (ctypes.c_float * levels)(*w)
    _ffi.check(lib.sa_ms_ssim(_ffi.ptr(x), _ffi.ptr(y), B, C, D, H, W, ctypes.cast(win_c, ctypes.c_void_p), win_size, levels,
                              ctypes.cast(w_c, ctypes.c_void_p), float(c1), float(c2), _ffi.ptr(out), _ffi.ptr(lm), _ffi.ptr(ws), _ffi.stream()),
               "sa_ms_ssim")
    return (out, lm) if level_means else out


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, weights=None, K=(0.01, 0.03)):
    """``pytorch_msssim.ms_ssim`` (0.2.1) for [B, C, D, H, W] volumes: the mean over everything with ``size_average``, else one value per batch
    element (the mean over channels).  Refuses as the package does (``ValueError`` for mismatched shapes and an even window, ``AssertionError``
    for min(H, W) <= (win_size - 1) * 16) and, beyond it, raises ``ValueError`` for what the kernel does not cover (see ``_ms_ssim``)."""
    out = _ms_ssim(X, Y, data_range=data_range, win_size=win_size, win_sigma=win_sigma, win=win, weights=weights, K=K)
    return out.mean() if size_average else out
