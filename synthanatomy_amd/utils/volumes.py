"""Volumes in and out of ``run_vqvae.py``'s stages: the loaders of ``.npy``, NIfTI-1 and ``synthetic_<k>`` inputs, as plain batches or through
``sa_augment``, and ``VolumeWriter`` for what a stage writes.  Importing the module loads no kernel."""
import os

import numpy as np
import torch

from .general import save_npy, stem


def _output_path(cfg, filename, postfix):
    """``<outputs>/<name>/<name>_<postfix><--output_ext>``: utils.general.save_npy's layout."""
    name = stem(filename)
    return os.path.join(cfg["outputs_directory"], name, f"{name}_{postfix}{cfg['output_ext']}")


def _augmented_name(f, i):
    """get_subjects' augmentation_id in the file name (reference src/utils/vqvae.py:601-608): <name>_<i><extension>"""
    cut = len(f) - (len(os.path.basename(f)) - len(stem(f)))      # where the extension starts
    return f[:cut] + f"_{i}" + f[cut:]


class VolumeWriter:
    """What a stage writes under ``--output_ext``: ``save`` takes a batch's names, {postfix: volumes [B, 1, D, H, W]} and the NIfTI headers the subjects were
    read with (None: the identity geometry).  ``batch()`` opens a batch of the NIfTI writer threads; ``close()`` joins them and re-raises their exception."""

    def __init__(self, cfg):
        self.cfg, self.saver = cfg, None
        if cfg["output_ext"] != ".npy":
            from .vqvae import NiftiSaver
            self.saver = NiftiSaver(cfg["output_ext"], cfg["output_dtype"], min(int(cfg.get("num_workers") or 0), 8))

    def batch(self):
        if self.saver is not None:
            self.saver.batch()

    def save(self, names, volumes, headers=None):
        if self.saver is None:      # one copy to the host per batch tensor
            for postfix, x in volumes.items():
                for n, v in zip(names, x.float().cpu().numpy()):
                    save_npy(v[0], self.cfg["outputs_directory"], n, postfix, np.float32)
            return
        from .vqvae import nifti_output_geometry
        size = next(iter(volumes.values())).shape[-3:]
        for j, (n, h) in enumerate(zip(names, headers or [None] * len(names))):      # straight from the device tensors, in the source file's own axes
            geometry = nifti_output_geometry(h, self.cfg["roi"], bool(self.cfg.get("load_nii_canonical", True)), size)
            for postfix, x in volumes.items():
                self.saver.save(x[j, 0], _output_path(self.cfg, n, postfix), *geometry)

    def close(self):
        if self.saver is not None:
            self.saver.close()


def _load_volume(path, cfg, gen, dev, block=None):
    from .vqvae import roi_shape
    if path.startswith("synthetic"):   # a volume that depends on its NAME only (not on how many were drawn before it): resumable, rank-independent
        g = torch.Generator(device=dev).manual_seed(cfg["seed"] * 1000003 + int(path.split("_")[-1]))
        return torch.rand(1, *roi_shape(cfg["roi"]), generator=g, device=dev)
    if _is_nifti(path):
        return _nifti_volume(path, cfg, dev, block)[0]
    return _read_volume(path, cfg).to(dev)


def _read_volume(path, cfg, dev=None, block=None):
    if _is_nifti(path):                # the whole volume in canonical axes, converted and normalised by sa_volume_ingest (there is no host decoder)
        return _nifti_volume(path, dict(cfg, roi=None), dev, block)[0].cpu()
    v = torch.from_numpy(np.load(path).astype(np.float32))
    if v.dim() == 3:
        v = v[None]
    if cfg["normalize"]:
        v = (v - v.min()) / (v.max() - v.min() + 1e-8)  # ScaleIntensityd(0, 1)
    return v


def _is_nifti(path):
    return path.endswith((".nii", ".nii.gz"))


def _nifti_volume(path, cfg, dev, block=None, whole=False):
    """A NIfTI-1 volume through sa_volume_ingest and where the ROI starts inside what is returned: LoadImaged(as_closest_canonical =
    --load_nii_canonical), ScaleIntensityd(0, 1) over the whole volume with --normalize, then the ROI as the kernel's window (``whole``: the whole canonical
    volume and the ROI's start, for sa_augment to crop).  A file smaller than the ROI is ingested whole, cropped and mirror-padded on the host (the rare
    path of ``_load_input``).  ``block`` = (header, voxel block) when a worker has read the file already."""
    from .nifti import header_orientation, read_nifti
    from .vqvae import hip_ingest, pad_to_roi, roi_shape, roi_window
    header, raw = block if block is not None else read_nifti(path)
    canonical = bool(cfg.get("load_nii_canonical", True))
    kw = dict(normalize=bool(cfg["normalize"]), canonical=canonical, device=dev)
    if not cfg["roi"]:
        return hip_ingest(header, raw, None, **kw), [0, 0, 0]
    start, size = roi_window(cfg["roi"], [header.dims[k] for k in header_orientation(header, canonical)[0]])
    if size != roi_shape(cfg["roi"]):
        v = hip_ingest(header, raw, None, **kw)
        crop = v[..., start[0]:start[0] + size[0], start[1]:start[1] + size[1], start[2]:start[2] + size[2]].cpu().numpy()
        return torch.from_numpy(np.ascontiguousarray(pad_to_roi(crop, cfg["roi"]))).to(v.device), [0, 0, 0]
    if whole:
        return hip_ingest(header, raw, None, **kw), start
    return hip_ingest(header, raw, (start, size), **kw), [0, 0, 0]


def _with_nifti_blocks(chunks, path_of, cfg):
    """(chunk, blocks) for every chunk, ``blocks[j]`` = (header, voxel block) of the chunk's j-th file when it is a NIfTI file, else None.  File read and
    gunzip are host work that releases the GIL: with ``--num_workers`` > 0 the NEXT chunk's files are fetched on min(num_workers, 8) threads while the
    caller works on the current one; 0 reads inline.  Order and content do not depend on the worker count."""
    from .nifti import read_nifti
    workers = min(int(cfg.get("num_workers") or 0), 8)
    if workers <= 0 or not any(_is_nifti(path_of(it)) for c in chunks for it in c):
        for c in chunks:
            yield c, [read_nifti(path_of(it)) if _is_nifti(path_of(it)) else None for it in c]
        return
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(workers) as ex:
        def submit(c):
            return [ex.submit(read_nifti, path_of(it)) if _is_nifti(path_of(it)) else None for it in c]
        ahead = submit(chunks[0])
        for i, c in enumerate(chunks):
            current, ahead = ahead, (submit(chunks[i + 1]) if i + 1 < len(chunks) else None)
            yield c, [f.result() if f is not None else None for f in current]


def _batches(files, order, bs, cfg, gen, dev):
    """Batches of this rank's shard (``order`` = indices into ``files`` from utils.general.shard_for_rank)."""
    chunks = [[files[k] for k in order[i:i + bs]] for i in range(0, len(order), bs)]
    for chunk, blocks in _with_nifti_blocks(chunks, lambda f: f, cfg):
        headers = [b[0] if b is not None else None for b in blocks]      # the NIfTI headers already read (utils.vqvae.nifti_output_geometry); None for other inputs
        yield chunk, torch.stack([_load_volume(f, cfg, gen, dev, b) for f, b in zip(chunk, blocks)]), headers


def _noise_seed(seed, counter, stream=0):
    """64-bit noise seed of one batch: a splitmix64 hash of (--seed, stream, counter); stream 0 = training iterations, 1 = evaluator, 2 = extraction.
    The callers fold the rank into the counter (counter * world + rank)."""
    z = (int(seed) * 0x9E3779B97F4A7C15 + int(counter) * 0xBF58476D1CE4E5B9 + int(stream) * 0x94D049BB133111EB + 0x2545F4914F6CDD1D) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return z ^ (z >> 31)


def _load_input(path, cfg, dev, block=None):
    """A volume for the sa_augment path and where the ROI starts inside it: the kernel crops (CenterSpatialCropd for three ints, SpatialCropd for three
    pairs); a file smaller than the ROI is cropped and mirror-padded on the host first (SpatialPadd SYMMETRIC, the rare path)."""
    from .vqvae import pad_to_roi, roi_shape, roi_window
    if _is_nifti(path):
        return _nifti_volume(path, cfg, dev, block, whole=True)
    if path.startswith("synthetic") or not cfg["roi"]:
        return _load_volume(path, cfg, None, dev), [0, 0, 0]
    v = _read_volume(path, cfg)
    start, size = roi_window(cfg["roi"], v.shape[-3:])
    if size != roi_shape(cfg["roi"]):
        crop = v[..., start[0]:start[0] + size[0], start[1]:start[1] + size[1], start[2]:start[2] + size[2]]
        v, start = torch.from_numpy(np.ascontiguousarray(pad_to_roi(crop.numpy(), cfg["roi"]))), [0, 0, 0]
    return v.to(dev), start


def _augmented_batches(items, bs, cfg, dev, mode, noise_seed):
    """Batches through sa_augment.  ``items``: (output name, file, epoch key, subject index) -- the draws of a sample depend on (--seed, epoch key, subject
    index) only (synthanatomy_amd.utils.vqvae.draw_augmentation); ``noise_seed(k)`` is the noise seed of batch k.  Yields (names, batch, noise seed)."""
    from .vqvae import draw_augmentation, hip_augment, in_window, roi_shape
    chunks = [items[i:i + bs] for i in range(0, len(items), bs)]
    for i, (chunk, blocks) in zip(range(0, len(items), bs), _with_nifti_blocks(chunks, lambda it: it[1], cfg)):
        vols, recs = [], []
        for (_, f, epoch_key, subject), block in zip(chunk, blocks):
            v, start = _load_input(f, cfg, dev, block)
            dims = roi_shape(cfg["roi"]) if cfg["roi"] else list(v.shape[-3:])
            recs.append(in_window(draw_augmentation(cfg, mode, cfg["seed"], epoch_key, subject, dims), start))
            vols.append(v)
        ns = noise_seed(i // bs)
        yield [c[0] for c in chunk], hip_augment(torch.stack(vols), np.stack(recs), cfg["patch_size"] or dims, ns), ns
