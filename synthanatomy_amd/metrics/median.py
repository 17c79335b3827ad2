"""Masked 3-D median filter of an anomaly map (this project's own rule, **unpinned**: the reference has no counterpart).

``median_filter_map`` runs the fused HIP path (``sa_anomaly_median``, csrc/median.hip): the map is restricted to an optionally eroded byte mask by a
select, filtered with a ``size``³ median whose window is zero outside the volume, restricted again, and summarised into the record ``anomaly_map``
fills (sum, max, the two 256-bin histograms, TP / FP / FN at a threshold).  The median is an order statistic under a total order of the fp32 bits, so
the output holds the bits of one of its inputs (or ``+0.0``).  Everything stays on the device.  There is no CPU fallback."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

SIZES = (1, 3, 5)
MAX_EROSION = 4              # include/synthanatomy_hip.h: SA_MEDIAN_MAX_EROSION
TILE = (8, 16, 32)           # include/synthanatomy_hip.h: SA_MEDIAN_TILE_D / H / W, the block's output tile (D, H, W)
MAX_VOXELS = 2 ** 31 - 1     # a volume must stay below this


def check_arguments(shape, size, mask_shape, erosion, label_shape, threshold, hist_max):
    """Every refusal of ``median_filter_map`` (a ``ValueError`` before any launch).  ``shape`` is [B, 1, D, H, W] or [B, D, H, W]; ``mask_shape`` and
    ``label_shape`` are None without a mask / labels.  Returns ((B, D, H, W), size, erosion, threshold or None, inv_bin as np.float32)."""
    shape = tuple(int(v) for v in shape)
    if len(shape) not in (4, 5) or (len(shape) == 5 and shape[1] != 1):
        raise ValueError(f"median_filter_map takes [B, 1, D, H, W] or [B, D, H, W] volumes, got {shape}")
    if min(shape) < 1:
        raise ValueError(f"median_filter_map takes volumes with every side >= 1, got {shape}")
    vshape = (shape[0],) + shape[-3:]
    if vshape[0] > 65535:
        raise ValueError(f"a batch of {vshape[0]} volumes: at most 65535 go into one call")
    if vshape[1] * vshape[2] * vshape[3] >= MAX_VOXELS:
        raise ValueError(f"a volume of {vshape[1]} x {vshape[2]} x {vshape[3]} voxels: fewer than 2^31 - 1 are needed")
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or size not in SIZES:
        raise ValueError(f"size={size!r}: choices are {list(SIZES)} (the window's side)")
    if isinstance(erosion, bool) or not isinstance(erosion, (int, np.integer)) or not 0 <= erosion <= MAX_EROSION:
        raise ValueError(f"erosion={erosion!r}: an integer in 0..{MAX_EROSION} (6-neighbourhood steps) is needed")
    if mask_shape is not None and tuple(int(v) for v in mask_shape) != shape:
        raise ValueError(f"mask of shape {tuple(mask_shape)} does not match the volumes of shape {shape}")
    if erosion > 0 and mask_shape is None:
        raise ValueError(f"erosion={erosion!r} without a mask: there is nothing to erode")
    if label_shape is not None and tuple(int(v) for v in label_shape) != shape:
        raise ValueError(f"labels of shape {tuple(label_shape)} do not match the volumes of shape {shape}")
    try:
        hm = float(hist_max)
    except (TypeError, ValueError):
        raise ValueError(f"hist_max={hist_max!r}: a number > 0 is needed") from None
    if not (hm > 0.0 and math.isfinite(hm)):
        raise ValueError(f"hist_max={hist_max!r}: a finite number > 0 is needed")
    from .anomaly import HIST_BINS
    with np.errstate(over="ignore"):
        inv_bin = np.float32(HIST_BINS / hm)
    if not (np.isfinite(inv_bin) and inv_bin > 0):
        raise ValueError(f"hist_max={hist_max!r}: 256 / hist_max is not a positive finite float32")
    t = None
    if threshold is not None:
        try:
            t = float(threshold)
        except (TypeError, ValueError):
            raise ValueError(f"threshold={threshold!r}: a finite number (or None) is needed") from None
        with np.errstate(over="ignore"):
            if not (math.isfinite(t) and np.isfinite(np.float32(t))):
                raise ValueError(f"threshold={threshold!r}: a finite float32 number (or None) is needed")
    return vshape, int(size), int(erosion), t, inv_bin


def median_filter_map(a, *, size: int = 5, mask=None, erosion: int = 0, labels=None, threshold: Optional[float] = None, hist_max: float = 1.0):
    """``(out, summaries)`` of a device tensor ``a`` [B, 1, D, H, W] or [B, D, H, W] (an anomaly map).  ``mask`` (like ``a``: foreground where > 0.5, or
    a bool tensor; None: every voxel) is eroded ``erosion`` times with the 6-neighbourhood, everything outside the volume counting as background;
    outside the eroded mask the map is replaced by ``+0.0`` (a select), the ``size``³ median is taken with zeros outside the volume under the total order
    of the fp32 keys, and the result is restricted to the eroded mask again.  ``size=1`` is the mask alone.  ``out`` (fp32, the shape of ``a``, a new
    tensor) holds bits of ``a`` or ``+0.0``.  ``summaries`` is the dict ``anomaly_map`` returns, taken over ``out`` (``labels``, ``threshold`` and
    ``hist_max`` mean what they mean there; ``taps`` is None), so ``best_dice``, ``average_precision`` and ``dice_from_counts`` apply unchanged.
    Nothing synchronises with the host."""
    import ctypes

    import torch

    from .. import _ffi
    from .anomaly import _label_bytes, _summaries
    vshape, k, e, t, inv_bin = check_arguments(tuple(a.shape), size, None if mask is None else tuple(mask.shape), erosion,
                                               None if labels is None else tuple(labels.shape), threshold, hist_max)
    _ffi.require_gpu()
    av = a.float().contiguous()
    mb = _label_bytes(mask, av.device)
    lab = _label_bytes(labels, av.device)
    P = _ffi.MedianParams(B=vshape[0], D=vshape[1], H=vshape[2], W=vshape[3], size=k, erosion=e, has_mask=int(mb is not None),
                          has_labels=int(lab is not None), has_threshold=int(t is not None), inv_bin=float(inv_bin),
                          threshold=float(t) if t is not None else 0.0)
    lib = _ffi.lib()
    nbytes = lib.sa_anomaly_median_workspace_bytes(ctypes.byref(P))
    _ffi.check(nbytes if nbytes < 0 else 0, "sa_anomaly_median_workspace_bytes")
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=av.device)
    res = torch.empty(P.B, _ffi.ANOMALY_RESULT_WORDS, dtype=torch.int64, device=av.device)
    out = torch.empty_like(av)
    with torch.cuda.device(av.device):
        _ffi.check(lib.sa_anomaly_median(_ffi.ptr(av), _ffi.ptr(mb), _ffi.ptr(lab), _ffi.ptr(out), ctypes.byref(P), _ffi.ptr(res), _ffi.ptr(ws),
                                         _ffi.stream()), "sa_anomaly_median")
    return out, _summaries(res, P, t, inv_bin, None)
