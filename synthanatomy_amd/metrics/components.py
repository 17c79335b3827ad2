"""Connected-component clean-up of a thresholded map and lesion scores (this project's own rule, **unpinned**: the reference has no
counterpart).

``connected_components`` runs the fused HIP path (``sa_components``, csrc/components.hip): the components of ``[map >= threshold]`` under 6-, 18- or
26-connectivity by a block-tiled union-find, canonical ids (1 + the smallest linear index of a component), the minimum-size filter and, against a label
volume, voxel and lesion counts.  Everything is an integer and stays on the device.  There is no CPU fallback.  ``lesion_scores`` turns the counts into
recall, precision and F1 on the host and needs numpy only."""
from __future__ import annotations

import math

import numpy as np

CONNECTIVITIES = (6, 18, 26)
TILE = (8, 16, 16)           # include/synthanatomy_hip.h: SA_COMPONENTS_TILE_D / H / W, the block's tile (D, H, W)
MAX_VOXELS = 2 ** 31 - 1     # a volume must stay below this: ids are int32 and 1 + a linear index
NAMES = ("components", "components_kept", "voxels_foreground", "voxels_kept", "largest_component")      # result words 0 .. 4
LABEL_NAMES = ("tp", "fp", "fn", "lesions", "lesions_detected", "kept_true")                               # result words 5 .. 10


def check_arguments(shape, threshold, connectivity, min_size, label_shape=None):
    """Every refusal of ``connected_components`` (a ``ValueError`` before any launch).  ``shape`` is [B, 1, D, H, W] or [B, D, H, W].  Returns
    ((B, D, H, W), the threshold as np.float32, connectivity, min_size)."""
    shape = tuple(int(v) for v in shape)
    if len(shape) not in (4, 5) or (len(shape) == 5 and shape[1] != 1):
        raise ValueError(f"connected_components takes [B, 1, D, H, W] or [B, D, H, W] volumes, got {shape}")
    if min(shape) < 1:
        raise ValueError(f"connected_components takes volumes with every side >= 1, got {shape}")
    if label_shape is not None and tuple(int(v) for v in label_shape) != shape:
        raise ValueError(f"labels of shape {tuple(label_shape)} do not match the volumes of shape {shape}")
    vshape = (shape[0],) + shape[-3:]
    if vshape[1] * vshape[2] * vshape[3] >= MAX_VOXELS:
        raise ValueError(f"a volume of {vshape[1]} x {vshape[2]} x {vshape[3]} voxels: fewer than 2^31 - 1 are needed (ids are int32)")
    try:
        t = float(threshold)
    except (TypeError, ValueError):
        raise ValueError(f"threshold={threshold!r}: a finite number is needed") from None
    with np.errstate(over="ignore"):
        t32 = np.float32(t)
    if not (math.isfinite(t) and np.isfinite(t32)):
        raise ValueError(f"threshold={threshold!r}: a finite float32 number is needed")
    if isinstance(connectivity, bool) or connectivity not in CONNECTIVITIES:
        raise ValueError(f"connectivity={connectivity!r}: choices are {list(CONNECTIVITIES)}")
    if isinstance(min_size, bool) or not isinstance(min_size, (int, np.integer)) or min_size < 1:
        raise ValueError(f"min_size={min_size!r}: an integer >= 1 (voxels) is needed")
    if min_size >= MAX_VOXELS:
        raise ValueError(f"min_size={min_size!r}: no volume this call takes has that many voxels")
    return vshape, t32, int(connectivity), int(min_size)


def connected_components(a, *, threshold, connectivity: int = 26, min_size: int = 1, labels=None):
    """``(ids, summaries)`` of a device tensor ``a`` [B, 1, D, H, W] or [B, D, H, W] (an anomaly map) and optional ``labels`` like ``a`` (class 1 where
    > 0.5, or a bool tensor).  ``ids`` (int32, the shape of ``a``) holds, on every voxel of a component of ``[a >= threshold]`` (fp32 compare, NaN is
    background) with at least ``min_size`` voxels, 1 + the smallest linear index ``d H W + h W + w`` of the component, and 0 elsewhere; the cleaned
    segmentation is ``ids > 0``.  ``summaries`` holds int64 device tensors [B]: ``components``, ``components_kept``, ``voxels_foreground``,
    ``voxels_kept``, ``largest_component`` and, with labels (None without), ``tp`` / ``fp`` / ``fn`` of the kept mask, ``lesions`` (the label volume's
    components under the same connectivity), ``lesions_detected`` (those with a kept voxel) and ``kept_true`` (kept components with a class-1 voxel).
    Nothing synchronises with the host."""
    import ctypes

    import torch

    from .. import _ffi
    from .anomaly import _label_bytes
    vshape, t32, c, n = check_arguments(tuple(a.shape), threshold, connectivity, min_size, None if labels is None else tuple(labels.shape))
    _ffi.require_gpu()
    av = a.float().contiguous()
    lab = _label_bytes(labels, av.device)
    P = _ffi.ComponentsParams(B=vshape[0], D=vshape[1], H=vshape[2], W=vshape[3], connectivity=c, min_size=n, has_labels=int(lab is not None),
                              threshold=float(t32))
    lib = _ffi.lib()
    nbytes = lib.sa_components_workspace_bytes(ctypes.byref(P))
    _ffi.check(nbytes if nbytes < 0 else 0, "sa_components_workspace_bytes")
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=av.device)
    res = torch.empty(P.B, _ffi.COMPONENTS_RESULT_WORDS, dtype=torch.int64, device=av.device)
    ids = torch.empty(av.shape, dtype=torch.int32, device=av.device)
    with torch.cuda.device(av.device):
        _ffi.check(lib.sa_components(_ffi.ptr(av), _ffi.ptr(lab), _ffi.ptr(ids), ctypes.byref(P), _ffi.ptr(res), _ffi.ptr(ws), _ffi.stream()),
                   "sa_components")
    summaries = {name: res[:, i] for i, name in enumerate(NAMES)}
    summaries.update({name: res[:, 5 + i] if lab is not None else None for i, name in enumerate(LABEL_NAMES)})
    return ids, summaries


def lesion_scores(lesions, lesions_detected, kept, kept_true):
    """(recall, precision, F1) per lesion: recall = lesions_detected / lesions (NaN when there is no lesion, as ``average_precision`` gives it),
    precision = kept_true / kept (0 when nothing is kept), F1 = 2 P R / (P + R) (0 where P + R is 0 or recall is undefined)."""
    lesions, lesions_detected, kept, kept_true = int(lesions), int(lesions_detected), int(kept), int(kept_true)
    recall = lesions_detected / lesions if lesions > 0 else float("nan")
    precision = kept_true / kept if kept > 0 else 0.0
    r = 0.0 if math.isnan(recall) else recall
    f1 = 2.0 * precision * r / (precision + r) if precision + r > 0 else 0.0
    return recall, precision, f1
