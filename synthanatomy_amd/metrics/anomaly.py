"""Voxel-space anomaly maps from healed codes (this project's own rule, **unpinned**: the reference has no counterpart).

``anomaly_map`` runs the fused HIP path (``sa_anomaly_map``, csrc/anomaly.hip): the residual between a scan and the decoding of its healed codes,
weighted by a latent grid (the resampling mask or the NLL map of ``Performer.heal``) that is upsampled and Gaussian-smoothed inside the kernel, plus the
per-volume summaries (sum, max, a 256-bin histogram per label class, TP / FP / FN at a threshold).  ``anomaly_map_ensemble`` (``sa_anomaly_map_ensemble``,
DESIGN §7.15) is the mean of that map over K healings of the same scans, with the summaries of the mean, in one pass.  There is no CPU fallback.  The
helpers below them turn the two histograms into segmentation scores on the host and need numpy only."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

RESIDUALS = {"abs": 0, "positive": 1, "negative": 2}      # include/synthanatomy_hip.h: SA_ANOMALY_ABS / POSITIVE / NEGATIVE
MAX_SIGMA = 8.0                                            # R = ceil(3 sigma) <= SA_ANOMALY_MAX_R = 24
HIST_BINS = 256


def gaussian_taps(sigma: float) -> np.ndarray:
    """The 2R + 1 taps g_i = exp(-i^2 / 2 sigma^2) / sum_j exp(-j^2 / 2 sigma^2), R = ceil(3 sigma): made in fp64 and rounded ONCE to fp32 (what the
    kernel and the tests' reference both use).  sigma = 0: the single tap 1."""
    sigma = _check_sigma(sigma)
    R = int(math.ceil(3.0 * sigma))
    if R == 0:
        return np.ones(1, dtype=np.float32)
    i = np.arange(-R, R + 1, dtype=np.float64)
    g = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(np.float32)


def _check_sigma(sigma) -> float:
    try:
        s = float(sigma)
    except (TypeError, ValueError):
        raise ValueError(f"sigma={sigma!r}: a number in [0, {MAX_SIGMA:g}] is needed") from None
    if not (0.0 <= s <= MAX_SIGMA):      # (NaN fails both comparisons)
        raise ValueError(f"sigma={sigma!r} is outside [0, {MAX_SIGMA:g}] (the filter has at most {2 * 24 + 1} taps)")
    return s


def check_arguments(shape, weight_shape, sigma, residual, threshold, hist_max):
    """Every refusal of ``anomaly_map`` (a ``ValueError`` before any launch).  Returns (factors or None, sigma, residual id, threshold or None, inv_bin)."""
    if residual not in RESIDUALS:
        raise ValueError(f"residual={residual!r}: choices are {sorted(RESIDUALS)}")
    s = _check_sigma(sigma)
    try:
        hm = float(hist_max)
    except (TypeError, ValueError):
        raise ValueError(f"hist_max={hist_max!r}: a number > 0 is needed") from None
    if not (hm > 0.0 and math.isfinite(hm)):
        raise ValueError(f"hist_max={hist_max!r}: a finite number > 0 is needed")
    with np.errstate(over="ignore"):
        inv_bin = np.float32(HIST_BINS / hm)
    if not (np.isfinite(inv_bin) and inv_bin > 0):
        raise ValueError(f"hist_max={hist_max!r}: 256 / hist_max is not a positive finite float32")
    t = None
    if threshold is not None:
        t = float(threshold)
        if not math.isfinite(t):
            raise ValueError(f"threshold={threshold!r}: a finite number (or None) is needed")
    factors = None
    if weight_shape is not None:
        vol, lat = tuple(int(v) for v in shape[-3:]), tuple(int(v) for v in weight_shape[-3:])
        if len(weight_shape) != 4 or int(weight_shape[0]) != int(shape[0]) or min(lat) < 1 or any(v % c for v, c in zip(vol, lat)):
            raise ValueError(f"weight of shape {tuple(weight_shape)} does not divide the volumes of shape {tuple(shape)}: [B, d, h, w] with D = f_D d, "
                             "H = f_H h, W = f_W w for integer factors is needed")
        factors = tuple(v // c for v, c in zip(vol, lat))
    return factors, s, RESIDUALS[residual], t, inv_bin


def anomaly_map(x, recon, weight=None, *, sigma, residual: str = "abs", labels=None, threshold: Optional[float] = None, hist_max: float = 1.0):
    """``(map, summaries)`` of device tensors ``x`` (the scan as the encoder saw it) and ``recon`` (``decode_samples`` of the healed codes), both
    [B, 1, D, H, W] or [B, D, H, W]; ``weight`` [B, d, h, w] (the ``resampled`` mask as {0, 1} or the ``nll`` grid; None: the plain residual, no filter),
    ``labels`` like ``x`` (class 1 where > 0.5).  ``map`` has the shape of ``x``; ``summaries`` holds device tensors ``sum`` [B] (fp64), ``max`` [B],
    ``tp`` / ``fp`` / ``fn`` [B] (int64, of ``map >= threshold``; None without a threshold), ``hist`` [B, 2, 256] (int64: label class, bin
    ``min(255, int(map * inv_bin))``) and the fp32 numbers the kernel used: ``inv_bin``, ``threshold``, ``taps``.  Nothing synchronises with the host."""
    import ctypes

    import torch

    from .. import _ffi
    if x.dim() not in (4, 5) or (x.dim() == 5 and x.shape[1] != 1):
        raise ValueError(f"anomaly_map takes [B, 1, D, H, W] or [B, D, H, W] volumes, got {tuple(x.shape)}")
    if tuple(recon.shape) != tuple(x.shape):
        raise ValueError(f"the scan {tuple(x.shape)} and the reconstruction {tuple(recon.shape)} differ in shape")
    if labels is not None and tuple(labels.shape) != tuple(x.shape):
        raise ValueError(f"labels of shape {tuple(labels.shape)} do not match the volumes of shape {tuple(x.shape)}")
    vshape = (x.shape[0],) + tuple(x.shape[-3:])
    factors, s, mode, t, inv_bin = check_arguments(vshape, None if weight is None else tuple(weight.shape), sigma, residual, threshold, hist_max)
    _ffi.require_gpu()
    xv = x.float().contiguous()
    rv = recon.float().contiguous().to(xv.device)
    m = None if weight is None else weight.to(xv.device).float().contiguous()
    P, taps = _params(vshape, None if m is None else tuple(m.shape[1:]), s, mode, t, inv_bin)
    lab = _label_bytes(labels, xv.device)
    lib = _ffi.lib()
    ws, res, out = _buffers(lib, P, xv)
    with torch.cuda.device(xv.device):
        _ffi.check(lib.sa_anomaly_map(_ffi.ptr(xv), _ffi.ptr(rv), _ffi.ptr(m), _ffi.ptr(lab), _ffi.ptr(out), ctypes.byref(P), _ffi.ptr(res), _ffi.ptr(ws),
                                      _ffi.stream()), "sa_anomaly_map")
    return out, _summaries(res, P, t, inv_bin, taps if weight is not None else None)


def _params(vshape, latent, s, mode, t, inv_bin):
    """(sa_anomaly_params, the taps) for volumes (B, D, H, W) and a latent grid (d, h, w) or None"""
    from .. import _ffi
    B, D, H, W = vshape
    P = _ffi.AnomalyParams(B=B, D=D, H=H, W=W, residual=mode, has_threshold=int(t is not None), inv_bin=float(inv_bin),
                           threshold=float(t) if t is not None else 0.0)
    taps = gaussian_taps(s)
    if latent is not None:
        P.d, P.h, P.w = (int(v) for v in latent)
        P.R = (len(taps) - 1) // 2
        for i, g in enumerate(taps.tolist()):
            P.taps[i] = g
    return P, taps


def _label_bytes(labels, device):
    import torch
    if labels is None:
        return None
    return (labels if labels.dtype == torch.bool else labels > 0.5).to(device).to(torch.uint8).contiguous()


def _buffers(lib, P, xv):
    """(workspace, result records, the map's tensor) on the device of ``xv``"""
    import ctypes

    import torch

    from .. import _ffi
    nbytes = lib.sa_anomaly_map_workspace_bytes(ctypes.byref(P))
    _ffi.check(nbytes if nbytes < 0 else 0, "sa_anomaly_map_workspace_bytes")
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=xv.device)
    res = torch.empty(P.B, _ffi.ANOMALY_RESULT_WORDS, dtype=torch.int64, device=xv.device)
    return ws, res, torch.empty_like(xv)


def _summaries(res, P, t, inv_bin, taps):
    import torch
    head = res[:, :2].contiguous().view(torch.float64)
    counted = t is not None
    return {"sum": head[:, 0], "max": head[:, 1].float(), "tp": res[:, 2] if counted else None, "fp": res[:, 3] if counted else None,
            "fn": res[:, 4] if counted else None, "hist": res[:, 8:].reshape(P.B, 2, HIST_BINS), "inv_bin": inv_bin,
            "threshold": np.float32(P.threshold) if counted else None, "taps": taps}


MAX_MEMBERS = 16      # include/synthanatomy_hip.h: SA_ANOMALY_MAX_MEMBERS


def _members(value, name, lead):
    """``value`` as a list of K member tensors: a tensor whose first axis is the members (``lead`` dims per member) or a sequence of tensors"""
    if hasattr(value, "dim"):
        if value.dim() != lead + 1:
            raise ValueError(f"{name} of shape {tuple(value.shape)}: a tensor with the members on its first axis or a sequence of member tensors is needed")
        return list(value.unbind(0)), True
    return list(value), False


def anomaly_map_ensemble(x, recons, weights=None, *, sigma, residual: str = "abs", labels=None, threshold: Optional[float] = None,
                         hist_max: float = 1.0):
    """The ensemble map over K healings of the scans ``x``, one fused pass of ``sa_anomaly_map_ensemble``: with ``a_k`` the map
    ``anomaly_map(x, recons[k], weights[k])`` gives, ``s = a_0``, ``s = s + a_k`` in fp32 in member order, ``map = s * np.float32(1.0 / K)``.
    ``recons`` is [K, B, 1, D, H, W] or [K, B, D, H, W], or a sequence of K tensors shaped like ``x`` (stacked here); ``weights`` [K, B, d, h, w], a
    sequence of K grids [B, d, h, w], or None; sigma, residual, labels, threshold and hist_max are shared by the members and mean what they mean for
    ``anomaly_map``.  1 <= K <= 16.  Returns ``(map, summaries)`` like ``anomaly_map``, the summaries taken over the ensemble map, with ``members``
    (int) and ``inv_members`` (np.float32) added.  Every refusal is a ``ValueError`` before any launch; there is no CPU fallback."""
    import ctypes

    import torch

    from .. import _ffi
    if x.dim() not in (4, 5) or (x.dim() == 5 and x.shape[1] != 1):
        raise ValueError(f"anomaly_map_ensemble takes [B, 1, D, H, W] or [B, D, H, W] volumes, got {tuple(x.shape)}")
    recs, stacked = _members(recons, "recons", x.dim())
    K = len(recs)
    if not 1 <= K <= MAX_MEMBERS:
        raise ValueError(f"recons holds {K} members: 1 to {MAX_MEMBERS} are needed")
    for k, rk in enumerate(recs):
        if not hasattr(rk, "shape") or tuple(rk.shape) != tuple(x.shape):
            raise ValueError(f"recons[{k}] of shape {tuple(getattr(rk, 'shape', ()))} differs from the scan {tuple(x.shape)}")
    grids = None
    if weights is not None:
        grids, w_stacked = _members(weights, "weights", 4)
        if len(grids) != K or any(g is None for g in grids):
            have = sum(g is not None for g in grids)
            raise ValueError(f"weights for {have} of {K} members: every member or none needs a grid")
        for k, gk in enumerate(grids):
            if tuple(gk.shape) != tuple(grids[0].shape):
                raise ValueError(f"weights[{k}] of shape {tuple(gk.shape)} differs from weights[0] of shape {tuple(grids[0].shape)}")
    if labels is not None and tuple(labels.shape) != tuple(x.shape):
        raise ValueError(f"labels of shape {tuple(labels.shape)} do not match the volumes of shape {tuple(x.shape)}")
    vshape = (x.shape[0],) + tuple(x.shape[-3:])
    factors, s, mode, t, inv_bin = check_arguments(vshape, None if grids is None else tuple(grids[0].shape), sigma, residual, threshold, hist_max)
    _ffi.require_gpu()
    xv = x.float().contiguous()
    # one [K, ...] block per operand: a tensor that already is one is used as it is, a sequence is stacked (which copies members that are not contiguous)
    rv = (recons if stacked else torch.stack([rk.to(xv.device) for rk in recs])).to(xv.device).float().contiguous()
    m = None
    if grids is not None:
        m = (weights if w_stacked else torch.stack([gk.to(xv.device) for gk in grids])).to(xv.device).float().contiguous()
    P, taps = _params(vshape, None if m is None else tuple(m.shape[2:]), s, mode, t, inv_bin)
    lab = _label_bytes(labels, xv.device)
    lib = _ffi.lib()
    ws, res, out = _buffers(lib, P, xv)
    with torch.cuda.device(xv.device):
        _ffi.check(lib.sa_anomaly_map_ensemble(_ffi.ptr(xv), _ffi.ptr(rv), rv[0].numel(), _ffi.ptr(m), m[0].numel() if m is not None else 0,
                                               _ffi.ptr(lab), _ffi.ptr(out), ctypes.byref(P), K, _ffi.ptr(res), _ffi.ptr(ws), _ffi.stream()),
                   "sa_anomaly_map_ensemble")
    summaries = _summaries(res, P, t, inv_bin, taps if m is not None else None)
    summaries.update(members=K, inv_members=np.float32(1.0 / K))
    return out, summaries


# ---- host-side scores from the two histograms (numpy only) ----

def bin_edges(inv_bin) -> np.ndarray:
    """The lower edge of every bin in map units: k / inv_bin.  Thresholding at edge k calls the voxels of bins >= k anomalous."""
    return np.arange(HIST_BINS, dtype=np.float64) / float(inv_bin)


def _edge_counts(hist0, hist1):
    h0, h1 = np.asarray(hist0, dtype=np.int64).reshape(HIST_BINS), np.asarray(hist1, dtype=np.int64).reshape(HIST_BINS)
    tp = np.cumsum(h1[::-1])[::-1]      # class-1 voxels in bins >= k
    fp = np.cumsum(h0[::-1])[::-1]
    return tp, fp, int(h1.sum()) - tp


def dice_per_edge(hist0, hist1) -> np.ndarray:
    """Dice of [bin >= k] against the label for every bin edge k: 2 TP / (2 TP + FP + FN), 0 where the denominator is 0."""
    tp, fp, fn = _edge_counts(hist0, hist1)
    den = 2 * tp + fp + fn
    return np.where(den > 0, 2.0 * tp / np.maximum(den, 1), 0.0)


def best_dice(hist0, hist1, inv_bin):
    """(the best Dice over the bin edges, its threshold in map units); the lowest edge among equals."""
    dice = dice_per_edge(hist0, hist1)
    k = int(np.argmax(dice))
    return float(dice[k]), float(bin_edges(inv_bin)[k])


def average_precision(hist0, hist1) -> float:
    """sum_k (R_k - R_{k-1}) P_k over DESCENDING bin edges (R before the first edge is 0); P = TP / (TP + FP), taken as 0 where nothing is predicted (such
    a step adds no recall).  NaN when there is no class-1 voxel."""
    tp, fp, _ = _edge_counts(hist0, hist1)
    n1 = int(tp[0])
    if n1 == 0:
        return float("nan")
    tp, fp = tp[::-1].astype(np.float64), fp[::-1].astype(np.float64)
    recall = tp / n1
    precision = np.where(tp + fp > 0, tp / np.maximum(tp + fp, 1.0), 0.0)
    return float(np.sum(np.diff(np.concatenate([[0.0], recall])) * precision))


def dice_from_counts(tp, fp, fn) -> float:
    den = 2 * int(tp) + int(fp) + int(fn)
    return 2.0 * int(tp) / den if den > 0 else 0.0
