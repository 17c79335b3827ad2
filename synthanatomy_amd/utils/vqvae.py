"""VQ-VAE helpers of the reference's ``src/utils/vqvae.py`` that the training loop needs: the MS-SSIM window and the training augmentations
(``get_transformations``, reference ``src/utils/vqvae.py:183-371``) as per-sample parameter records for ``sa_augment`` (csrc/augment.hip)."""
from __future__ import annotations

from enum import Enum
from math import floor

import numpy as np


class AugmentationStrengthScalers(Enum):
    """Per-transform scale of ``--augmentation_strength`` (reference ``src/utils/vqvae.py:46-53``)."""
    AFFINEROTATE = 0.2
    AFFINETRANSLATE = 1
    AFFINESCALE = 0.01
    ADJUSTCONTRASTGAMMA = 0.01
    SHIFTINTENSITYOFFSET = 0.025
    GAUSSIANNOISESTD = 0.01


AUG_IDENTITY, AUG_AFFINE, AUG_SIGNED_PERM = 0, 1, 2                 # include/synthanatomy_hip.h: SA_AUG_*
AUG_GAMMA, AUG_SHIFT, AUG_NOISE, AUG_CLAMP = 1, 2, 4, 8
# sa_augment_params (128 bytes)
AUG_DTYPE = np.dtype([("mode", "<i4"), ("flags", "<i4"), ("off", "<i4", 3), ("ext", "<i4", 3), ("perm", "<i4", 3), ("sign", "<i4", 3), ("M", "<f4", 12),
                      ("gamma", "<f4"), ("shift", "<f4"), ("noise_std", "<f4"), ("reserved", "<i4", 3)])
assert AUG_DTYPE.itemsize == 128


def augmentation_ranges(augmentation_strength: float) -> dict:
    """The ranges of reference ``src/utils/vqvae.py:257-357``: half widths of the affine draws, (low, high) of gamma, the largest shift and noise std."""
    s = augmentation_strength
    return {"rotate": 0.04 + AugmentationStrengthScalers.AFFINEROTATE.value * s,
            "translate": 2 + int(round(AugmentationStrengthScalers.AFFINETRANSLATE.value * s)),
            "scale": 0.05 + AugmentationStrengthScalers.AFFINESCALE.value * s,
            "gamma": (0.99 - AugmentationStrengthScalers.ADJUSTCONTRASTGAMMA.value * s, 1.01 + AugmentationStrengthScalers.ADJUSTCONTRASTGAMMA.value * s),
            "shift": 0.05 + AugmentationStrengthScalers.SHIFTINTENSITYOFFSET.value * s,
            "noise_std": 0.02 + AugmentationStrengthScalers.GAUSSIANNOISESTD.value * s}


def is_augmented(config: dict, mode: str) -> bool:
    """Upstream: training always augments and extraction does with ``no_augmented_extractions != 0``; here training augments behind the opt-in
    ``--augmentation`` switch (run_vqvae.py)."""
    return bool(mode == "training" and config.get("augmentation")) or bool(mode == "extracting" and config.get("no_augmented_extractions", 0) != 0)


def affine_matrix(rotate, translate, scale) -> np.ndarray:
    """Row-major 3 x 4 fp64 matrix of MONAI's ``AffineGrid``: rotate . shear (none) . translate . scale, rotation = Rx(r0) . Ry(r1) . Rz(r2) about the three
    spatial axes (axis 0 = D).  UNPINNED: MONAI is not available offline; composition order and Euler convention are this package's restatement."""
    r0, r1, r2 = (float(v) for v in rotate)
    c, s = np.cos(r0), np.sin(r0)
    rx = np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=np.float64)
    c, s = np.cos(r1), np.sin(r1)
    ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=np.float64)
    c, s = np.cos(r2), np.sin(r2)
    rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64)
    rot = np.eye(4)
    rot[:3, :3] = rx @ ry @ rz
    tr = np.eye(4)
    tr[:3, 3] = np.asarray(translate, dtype=np.float64)
    sc = np.diag([*np.asarray(scale, dtype=np.float64), 1.0])
    return (rot @ tr @ sc)[:3]


def compose_signed_perm(flips, ks):
    """(perm, sign) of ``SA_AUG_SIGNED_PERM`` for np.flip over axis a where ``flips[a]``, then np.rot90(k=ks[0], axes=(0, 1)), np.rot90(k=ks[1], axes=(1, 2)),
    np.rot90(k=ks[2], axes=(0, 2)) -- the order of the reference's transform list.  Output axis a reads source axis perm[a], backwards where sign[a] < 0."""
    perm, sign = [0, 1, 2], [1, 1, 1]
    for a in range(3):
        if flips[a]:
            sign[a] = -sign[a]
    for k, (i, j) in zip(ks, ((0, 1), (1, 2), (0, 2))):
        for _ in range(int(k) % 4):      # np.rot90(m, 1, (i, j)) = swapaxes(flip(m, j), i, j)
            sign[j] = -sign[j]
            perm[i], perm[j] = perm[j], perm[i]
            sign[i], sign[j] = sign[j], sign[i]
    return perm, sign


def identity_record(dims, off=(0, 0, 0)) -> np.ndarray:
    """A record that copies the window of size ``dims`` at ``off``; every intensity bit off."""
    rec = np.zeros((), dtype=AUG_DTYPE)
    rec["mode"] = AUG_IDENTITY
    rec["off"], rec["ext"] = off, dims
    rec["perm"], rec["sign"] = (0, 1, 2), (1, 1, 1)
    rec["M"] = np.eye(3, 4, dtype=np.float32).reshape(-1)
    rec["gamma"] = 1.0
    return rec


def check_patch_size(config: dict, mode: str):
    """The three RandRotate90d of the patch pipeline swap the sides of every axis pair: with unequal sides the reference's batch collation fails."""
    ps = config.get("patch_size")
    if ps and is_augmented(config, mode) and config.get("augmentation_probability", 0) > 0 and len(set(int(p) for p in ps)) != 1:
        raise ValueError(f"--patch_size={tuple(ps)}: the patch augmentations rotate by 90 degrees over every axis pair, which needs equal sides "
                         "(set --augmentation_probability=0 or a cubic --patch_size)")


def draw_augmentation(config: dict, mode: str, seed: int, epoch: int, subject_index: int, in_dims) -> np.ndarray:
    """The parameter record (0-d array of ``AUG_DTYPE``) of one subject: what the reference's transform list would draw.  The draws are a pure function of
    (seed, epoch, subject_index) -- numpy ``Generator`` seeded with that triple, every value drawn in a fixed order whether its transform fires or not --
    so they do not depend on rank, batch composition or call order and a resumed run repeats them.  Each transform fires with probability
    ``augmentation_probability``.  Without ``patch_size``: RandAffined (else identity); with it: a random crop, then three flips and three rot90s
    (k in 1..3).  Then gamma ~ U(range), shift ~ U(0, max), noise std ~ U(0, max) (MONAI's RandGaussianNoise draws its std), and the clamp whenever an
    intensity step fired (on [0, 1] data the reference's unconditional clamp is a no-op otherwise)."""
    in_dims = tuple(int(v) for v in in_dims)
    ps = config.get("patch_size")
    check_patch_size(config, mode)
    rng = np.random.default_rng([int(seed), int(epoch), int(subject_index)])
    p = float(config.get("augmentation_probability", 0.0))
    rg = augmentation_ranges(config.get("augmentation_strength", 0))
    fire = rng.random(10) < p          # affine, flip 0 1 2, rot90 (0,1) (1,2) (0,2), gamma, shift, noise
    rotate = rng.uniform(-rg["rotate"], rg["rotate"], 3)
    translate = rng.uniform(-rg["translate"], rg["translate"], 3)
    scale = 1.0 + rng.uniform(-rg["scale"], rg["scale"], 3)
    ks = rng.integers(1, 4, 3)
    gamma = rng.uniform(*rg["gamma"])
    shift = rng.uniform(0.0, rg["shift"])
    std = rng.uniform(0.0, rg["noise_std"])
    corner = rng.random(3)
    if ps:
        ps = tuple(int(v) for v in ps)
        if len(ps) != 3 or any(q < 1 or q > n for q, n in zip(ps, in_dims)):
            raise ValueError(f"--patch_size={ps} does not fit into volumes of {in_dims}")
        off = [min(int(c * (n - q + 1)), n - q) for c, n, q in zip(corner, in_dims, ps)]      # RandSpatialCropd: a uniform corner among the n - q + 1 legal ones
        rec = identity_record(ps, off)
    else:
        rec = identity_record(in_dims)
    if not is_augmented(config, mode):
        return rec
    if ps:
        flips = [bool(f) for f in fire[1:4]]
        k3 = [int(k) if f else 0 for k, f in zip(ks, fire[4:7])]
        if any(flips) or any(k3):
            rec["mode"] = AUG_SIGNED_PERM
            rec["perm"], rec["sign"] = compose_signed_perm(flips, k3)
    elif fire[0]:
        rec["mode"] = AUG_AFFINE
        rec["M"] = affine_matrix(rotate, translate, scale).astype(np.float32).reshape(-1)
    flags = 0
    if fire[7]:
        flags |= AUG_GAMMA
        rec["gamma"] = gamma
    if fire[8]:
        flags |= AUG_SHIFT
        rec["shift"] = shift
    if fire[9]:
        flags |= AUG_NOISE
        rec["noise_std"] = std
    if flags:
        flags |= AUG_CLAMP
    rec["flags"] = flags
    return rec


def roi_window(roi, in_dims):
    """(start, size) of the reference's ROI crop inside a volume of ``in_dims``: three ints = CenterSpatialCropd (start = n // 2 - r // 2), three
    (start, stop) pairs = SpatialCropd; both clipped to the volume, so ``size`` is smaller than the ROI where the volume is (then ``pad_to_roi``)."""
    in_dims = [int(v) for v in in_dims]
    if not roi:
        return [0, 0, 0], in_dims
    if isinstance(roi[0], (int, np.integer)):
        start = [max(n // 2 - int(r) // 2, 0) for n, r in zip(in_dims, roi)]
        stop = [min(s + int(r), n) for s, r, n in zip(start, roi, in_dims)]
    elif isinstance(roi[0], (tuple, list)):
        start = [min(max(int(a[0]), 0), n) for a, n in zip(roi, in_dims)]
        stop = [min(max(int(a[1]), s), n) for a, s, n in zip(roi, start, in_dims)]
    else:
        raise ValueError(f"roi should be either a Tuple with three ints like (0,1,2) or a Tuple with three Tuples that have two ints like "
                         f"((0,1),(2,3),(4,5)). But received {roi}.")
    return start, [b - a for a, b in zip(start, stop)]


def roi_shape(roi):
    return [int(r) for r in roi] if isinstance(roi[0], (int, np.integer)) else [int(a[1]) - int(a[0]) for a in roi]


def pad_to_roi(volume: np.ndarray, roi) -> np.ndarray:
    """SpatialPadd(spatial_size = the ROI's shape, mode = SYMMETRIC) on the last three axes of a host array: mirror padding, the odd voxel behind."""
    want = roi_shape(roi)
    width = [(0, 0)] * (volume.ndim - 3) + [((w - n) // 2, (w - n) - (w - n) // 2) if w > n else (0, 0) for w, n in zip(want, volume.shape[-3:])]
    return np.pad(volume, width, mode="symmetric") if any(a or b for a, b in width) else volume


def in_window(rec: np.ndarray, start) -> np.ndarray:
    """The record moved into the window that starts at ``start`` of a larger volume (the ROI): its offsets are relative to that window."""
    rec = rec.copy()
    rec["off"] = rec["off"] + np.asarray(start, dtype=np.int32)
    return rec


def check_records(records: np.ndarray, in_dims, out_dims):
    """The conditions sa_augment puts on its records (the kernel answers a broken one with zeros; the host refuses it)."""
    for b, r in enumerate(records):
        off, ext = [int(v) for v in r["off"]], [int(v) for v in r["ext"]]
        if r["mode"] == AUG_AFFINE:
            ok = all(o >= 0 and e >= 1 and o + e <= n for o, e, n in zip(off, ext, in_dims))
        elif r["mode"] in (AUG_IDENTITY, AUG_SIGNED_PERM):
            perm = [int(v) for v in r["perm"]] if r["mode"] == AUG_SIGNED_PERM else [0, 1, 2]
            ok = sorted(perm) == [0, 1, 2] and all(off[perm[a]] >= 0 and off[perm[a]] + out_dims[a] <= in_dims[perm[a]] for a in range(3))
        else:
            ok = False
        if not ok:
            raise ValueError(f"augmentation record {b} (mode {int(r['mode'])}, off {off}, ext {ext}) does not fit input {tuple(in_dims)} -> output {tuple(out_dims)}")


_AUG_WS = {}      # device index -> zeroed workspace (sa_augment keeps it usable from call to call)


def hip_augment(x, records: np.ndarray, out_dims, seed: int, return_workspace: bool = False):
    """``sa_augment``: x [B, 1, Di, Hi, Wi] fp32 on the device, ``records`` B entries of ``AUG_DTYPE`` (one upload), -> y [B, 1, *out_dims].  Two launches on
    the current stream.  ``return_workspace``: also the int64 view [B, 4] of the workspace (word 2 = the float min | max << 32 a gamma step used, word 3 =
    status)."""
    import torch
    from .. import _ffi
    _ffi.require_gpu()
    records = np.ascontiguousarray(np.atleast_1d(records), dtype=AUG_DTYPE)
    if x.dim() != 5 or x.shape[1] != 1 or x.dtype != torch.float32 or records.shape != (x.shape[0],):
        raise ValueError(f"hip_augment: x must be fp32 [B, 1, D, H, W] with one record per sample, got {tuple(x.shape)} {x.dtype} and {records.shape} records")
    B, in_dims, out_dims = int(x.shape[0]), [int(v) for v in x.shape[2:]], [int(v) for v in out_dims]
    check_records(records, in_dims, out_dims)
    x = x.contiguous()
    lib = _ffi.lib()
    ws = _AUG_WS.get(x.device.index)
    if ws is None or ws.numel() < 4 * B:
        ws = _AUG_WS[x.device.index] = torch.zeros(4 * max(B, 64), dtype=torch.int64, device=x.device)
    assert lib.sa_augment_workspace_bytes(B) <= ws.numel() * 8
    params = torch.from_numpy(records.view(np.uint8).reshape(B, AUG_DTYPE.itemsize)).to(x.device)
    y = torch.empty((B, 1, *out_dims), dtype=torch.float32, device=x.device)
    _ffi.check(lib.sa_augment(_ffi.ptr(x), _ffi.ptr(y), B, *in_dims, *out_dims, _ffi.ptr(params), int(seed) & 0xFFFFFFFFFFFFFFFF, _ffi.ptr(ws), _ffi.stream()),
               "sa_augment")
    return (y, ws[:4 * B].view(B, 4)) if return_workspace else y


INGEST_NORMALIZE = 1      # include/synthanatomy_hip.h: SA_INGEST_NORMALIZE
_INGEST_WS = {}           # device index -> zeroed workspace (sa_volume_ingest resets it)


def hip_ingest(header, raw, window=None, normalize: bool = True, canonical: bool = True, device=None, return_workspace: bool = False):
    """``sa_volume_ingest``: the voxel block ``raw`` of a NIfTI-1 file (``utils.nifti.read_nifti``) -> [1, *ext] fp32 on the device in canonical axes (the
    stored order without ``canonical``).  ``window`` = (start, size) in those axes, None = the whole volume; ``normalize`` = ScaleIntensityd(0, 1) over the
    WHOLE volume.  One upload of the block as stored, at most two launches on the current stream.  ``return_workspace``: also the int64 view of the
    workspace (word 2 = the float min | max << 32 of the finite voxels, word 3 = the number of non-finite voxels, which came out as 0)."""
    import ctypes
    import warnings

    import torch
    from .. import _ffi
    from .nifti import header_orientation
    _ffi.require_gpu()
    perm, sign = header_orientation(header, canonical)
    n_can = [int(header.dims[k]) for k in perm]
    start, size = ([0, 0, 0], n_can) if window is None else ([int(v) for v in window[0]], [int(v) for v in window[1]])
    if len(start) != 3 or len(size) != 3 or any(s < 0 or e < 1 or s + e > n for s, e, n in zip(start, size, n_can)):
        raise ValueError(f"hip_ingest: window start {start} size {size} does not fit the volume {tuple(n_can)} of {header.path}")
    if len(raw) < header.nbytes:
        raise ValueError(f"hip_ingest: {header.path}: the voxel block holds {len(raw)} bytes, dims {tuple(header.dims)} need {header.nbytes}")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)      # (a read-only buffer: it is only read)
        block = torch.frombuffer(raw, dtype=torch.uint8, count=header.nbytes).to(dev)
    lib = _ffi.lib()
    ws = _INGEST_WS.get(dev.index)
    if ws is None:
        ws = _INGEST_WS[dev.index] = torch.zeros(8, dtype=torch.int64, device=dev)
    assert lib.sa_volume_ingest_workspace_bytes() <= ws.numel() * 8
    P = _ffi.IngestParams(dtype=header.datatype, byteswap=int(header.byteswap), flags=INGEST_NORMALIZE if normalize else 0, slope=header.slope,
                          inter=header.inter)
    P.n[:], P.perm[:], P.sign[:], P.off[:], P.ext[:] = [int(v) for v in header.dims], perm, sign, start, size
    y = torch.empty((1, *size), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _ffi.check(lib.sa_volume_ingest(_ffi.ptr(block), header.nbytes, _ffi.ptr(y), ctypes.byref(P), _ffi.ptr(ws), _ffi.stream()), "sa_volume_ingest")
    return (y, ws) if return_workspace else y


def get_ms_ssim_window(config: dict, logger=None) -> int:
    """Window size of the MS-SSIM key metric (reference ``src/utils/vqvae.py:499-543``).  The smallest spatial side comes from ``eval_patch_size``,
    else from ``roi`` (ints or (start, stop) pairs), else from ``input_shape``.  A side > 160 gives 11; otherwise w = floor((side / 16 + 1) / 2),
    ``ValueError`` for w <= 1, and an even w becomes the next odd number (default roi 160 -> 5, 112 -> 5, 48 -> 3, 47 -> ValueError)."""
    if config.get("eval_patch_size"):
        min_ps = min(config["eval_patch_size"])
    elif config.get("roi"):
        roi = config["roi"]
        if isinstance(roi[0], int):
            min_ps = min(roi)
        else:
            min_ps = min(a[1] - a[0] for a in roi)
    else:
        min_ps = min(config["input_shape"])

    if min_ps > 160:
        win_size = 11
    else:
        win_size = floor(((min_ps / 2 ** 4) + 1) / 2)
        if win_size <= 1:
            raise ValueError("Window size for MS-SSIM can't be calculated. Please increase patch_size's smallest dimension.")
        if win_size % 2 == 0:
            win_size += 1

    if logger:
        logger.info("MS-SSIM window calculation:")
        if config.get("eval_patch_size"):
            logger.info(f"\tMinimum spatial dimension: {min_ps}")
        logger.info(f"\tWindow size {win_size}")
    return win_size
