#!/usr/bin/env python3
"""VQ-VAE entry point with the reference's flags and modes (reference run_vqvae.py:538-859):

    python run_vqvae.py run --training_subjects=synthetic:16 --validation_subjects=synthetic:2 --project_directory=/tmp/proj/ \\
        --experiment_name=exp --mode=training|extracting|decoding|anomaly  [--no_levels=4 --no_channels=256 ...]

MONAI/ignite/fire/deepspeed are not on the target, so the loop is a minimal in-house one: Adam + per-iteration ExponentialLR
(run_vqvae.py:82-91,162), losses "mse", "jukebox" (spectral), "spectral" / "hartley" / "wavegan" (FFT amplitude + phase, weighted Hartley and
spectral convergence + log magnitude; their factors are not scheduled, as upstream) and "baur" (L1 + L2 + image-gradient difference, its factor scheduled per epoch
by --initial_factor_value / --initial_factor_steps / --max_factor_steps / --max_factor_value) and "perceptual" / "jukebox_perceptual" / "hartley_perceptual"
(2.5D LPIPS-alex on HIP; they need --perceptual_weights=<file in the lpips.LPIPS(net='alex') state-dict layout, see tools/make_lpips_weights.py |
random:seed>, nothing is downloaded) and "baseline" (L1 + five-axis FFT amplitude + three-plane LPIPS-squeeze; it needs --perceptual_weights in the
lpips.LPIPS(net='squeeze') layout, tools/make_lpips_weights.py --net=squeeze), optional adversarial component
(src/engines/trainer.py semantics incl. the adaptive weight; criteria vanilla / hinge / least_square), checkpoints with the reference's keys
(network, optimizer, lr_scheduler, trainer, d_*) restored on resume, uint16 ``.npy`` code files.
Inputs: ``.npy`` volumes, single-file NIfTI-1 volumes (``.nii`` / ``.nii.gz``: read with the standard library, then converted, reoriented to the
closest canonical axes with ``--load_nii_canonical``, scaled to [0, 1] with ``--normalize`` and cropped to ``--roi`` on the device by ``sa_volume_ingest``,
DESIGN 7.7; ``--num_workers`` threads read the next batch's files ahead) -- any of dir / glob / csv listing -- or ``synthetic:<n>`` (uniform [0,1)
volumes of ``--roi`` size).
Multi-GPU: launch with torchrun; one process per GPU, RCCL.

``--augmentation=True`` (MI355X-only switch, default False) turns on the reference's training augmentations (src/utils/vqvae.py:183-371, which upstream
always applies in ``--mode=training``): every transform fires with ``--augmentation_probability``, ranges scale with ``--augmentation_strength``; without
``--patch_size`` a random affine resample, with it a random crop, three flips and three 90-degree rotations; then gamma contrast, intensity shift,
Gaussian noise and the clamp to [0, 1].  Training batches AND the evaluator's batches go through it (as upstream's evaluation transform does), on the
device in two launches of ``sa_augment``; the draws are keyed on (seed, epoch, subject), the noise on (seed, iteration).  With the default
False the loop is untouched and ``--augmentation_probability`` stays inert.  ``--patch_size`` crops training batches with or without the switch, and
``--mode=extracting --no_augmented_extractions=n`` writes n augmented extractions ``<name>_<i>`` per subject (no switch needed, as upstream).

``--output_ext=.npy|.nii|.nii.gz`` and ``--output_dtype=float32|int16|uint8`` (MI355X-only switches, defaults ``.npy`` / ``float32``: nothing changes for
existing runs) write the volumes of ``--mode=extracting`` (``<name>_reconstruction``) and ``--mode=decoding`` (``<name>_sample``) as single-file NIfTI-1,
what upstream's ``SegmentationSaver(output_ext=".nii.gz", resample=False, dtype=float32)`` produces (reference run_vqvae.py:467-514).  The voxel block is
made on the device by ``sa_volume_egress`` straight from the decoder's output: a reconstruction of a NIfTI input goes back into its source
file's own axes with an affine that puts the ROI where the source has it; other inputs and every decoded sample get the identity.  Integer dtypes are
auto-scaled to the full code range (scl_slope / scl_inter in the header).  ``--num_workers`` threads (at most 8) compress and write while the next batch
is decoded.  The code files stay uint16 ``.npy``.  The flags act or refuse: an unknown value, an integer dtype with ``.npy``, a NIfTI extension with
``--mode=training`` or with ``--no_augmented_extractions > 0`` raise a ``ValueError`` before anything runs.

``--codebook_restart_patience=<steps>`` (MI355X-only; default None: nothing changes) restarts dead codes of the EMA codebook: a code that no
encoder output of any rank chose for that many consecutive training steps is re-seeded from a row of the current step's encoder output, at most
``--codebook_restart_max`` (default 32, 1..64) codes per step, inside the EMA update's launch (``sa_vq_ema_update_restart``).  The draw is keyed on
(``--seed``, global iteration), the counters travel in the checkpoint's ``codebook_restart`` entry, and the log line gains ``codebook_dead <n> restarted <r>``.
``--decay_warmup=step|linear`` with ``--max_decay_epochs=<n>|auto`` schedules the EMA decay from ``--decay`` to 0.99 at every finished epoch
(networks/vqvae/configure.py: decay_schedule).  All four flags act or refuse by name before anything touches the device.

``--mode=anomaly`` (MI355X-only; the rule is this project's own) is the last stage of the healing application: every ``--validation_subjects``
scan goes through the usual input path, the files ``run_transformer.py --mode=healing`` wrote for its codes (``<stem>_quantization_0_healed_sample.npy``,
``..._resampled.npy``, ``..._nll.npy``) are found by stem under ``--anomaly_codes=<dir|glob>`` (default: this experiment's outputs directory), the healed
codes are decoded and ``sa_anomaly_map`` turns scan, decoding and the latent weight grid into ``<name>_anomaly_map`` on the device, with no file in
between; ``<name>_healed_reconstruction`` is written next to it (``.npy``, or NIfTI with the source geometry under ``--output_ext``) and every rank
writes ``anomaly_scores_rank<k>.csv`` (subject, sum, max and, with ``--anomaly_labels``, Dice at the threshold, the best Dice over the 256 histogram
edges with its threshold, and the average precision).  ``--anomaly_weight=mask|nll|none`` picks the grid, ``--anomaly_sigma`` the Gaussian that smooths
its upsampling (None: half the down-sampling factor), ``--anomaly_residual=abs|positive|negative`` the sign convention, ``--anomaly_threshold`` the
operating point of the TP / FP / FN counts, ``--anomaly_hist_max`` the top of the histogram, ``--anomaly_labels`` any input spec of label volumes
(matched by stem, reoriented and cropped like the scans, never normalised, class 1 where > 0.5).

``--anomaly_ensemble=<dir|glob>,<dir|glob>[,...]`` (MI355X-only; default None: nothing changes) scores every scan against 2 to 16 healings of
its codes, one ``run_transformer.py --mode=healing`` outputs directory per ordering or seed: every spec is searched like ``--anomaly_codes`` (which it
replaces; giving both is refused), every member is decoded on its own, and ``sa_anomaly_map_ensemble`` writes the mean of the members' weighted residuals
as ``<name>_anomaly_map`` in one pass, with the scores of that mean; ``<name>_healed_reconstruction_m<k>`` is member k's decoding in flag order and
``anomaly_scores_rank<k>.csv`` gains a last column ``members``.  The other ``--anomaly_*`` flags are shared by the members.

``--anomaly_min_component=<voxels>`` (MI355X-only; default None: nothing changes) cleans the segmentation ``[map >= --anomaly_threshold]``
(which it needs) on the device: ``sa_components`` labels its connected components under ``--anomaly_connectivity=6|18|26`` (default 26), drops those
below that many voxels and counts lesions; the single map and the ensemble map both go through it.  ``<name>_anomaly_segmentation`` ({0, 1}) is
written like the map and the CSV gains ``components``, ``components_kept``, ``voxels_kept``, ``largest_component`` and, with ``--anomaly_labels``,
``dice_cleaned``, ``lesions``, ``lesions_detected``, ``lesion_recall``, ``lesion_precision``, ``lesion_f1`` (before ``members``).

``--anomaly_median=1|3|5`` and ``--anomaly_mask=scan|<dir|glob>`` (MI355X-only; default None: nothing changes) filter the map, single or
ensemble, on the device before the components: ``sa_anomaly_median`` restricts it to the mask by a select, takes the 3-D median of that side (zeros
outside the volume) and restricts it again; a mask alone means side 1.  ``scan`` is ``[x > --anomaly_mask_threshold]`` (default 0.0, only valid with
``scan``) of the scan as the encoder saw it; otherwise mask volumes are matched to the subjects by stem and loaded like ``--anomaly_labels``
(reoriented and cropped like the scan, never normalised; foreground where > 0.5).  ``--anomaly_mask_erosion=0..4`` (default 0, needs a mask) erodes the
mask that many times with the 6-neighbourhood, the outside of the volume counting as background.  ``<name>_anomaly_map`` stays the raw map,
``<name>_anomaly_map_filtered`` is written like it, ``--anomaly_min_component`` then cleans the filtered map, and the CSV keeps its columns (the raw
map's) and gains ``filtered_sum``, ``filtered_max`` and, with ``--anomaly_labels``, ``filtered_dice``, ``filtered_best_dice``,
``filtered_best_dice_threshold``, ``filtered_average_precision`` before the component columns.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from synthanatomy_amd.utils.general import (REQUIRED, check_for_checkpoints, create_folder_structure, list_inputs, load_checkpoint,  # noqa: E402
                                            load_network_state, log, parse_flags, save_checkpoint, save_npy, shard_for_rank)

DEFAULTS = dict(
    training_subjects=REQUIRED, validation_subjects=REQUIRED, project_directory=REQUIRED, experiment_name=REQUIRED, mode="training",
    no_augmented_extractions=0, device=0, distributed_port=29500, amp=True, deterministic=False, cuda_benchmark=True, seed=4, epochs=100,
    learning_rate=0.0003, gamma=0.99999, log_every=1, checkpoint_every=1, eval_every=5, augmentation_probability=0.2, augmentation_strength=0,
    loss="mse", adversarial_component=False, finetune_adversarial_component=None, finetune_patience=100,
    discriminator_network="baseline_discriminator", discriminator_learning_rate=0.0005, discriminator_loss="least_square",
    generator_loss="least_square", use_adversarial_adaptive_weight=False, adaptive_adversarial_weight_threshold=0,
    adaptive_adversarial_weight_value=1, initial_factor_value=0, initial_factor_steps=25, max_factor_steps=50, max_factor_value=5, normalize=True,
    roi=((16, 176), (16, 240), (96, 256)), augmentation=False, batch_size=3, patch_size=None, eval_batch_size=3, eval_patch_size=None, training_epoch_length=None,
    num_workers=8, prefetch_factor=8, starting_epoch=0, network="baseline_vqvae", use_subpixel_conv=False, use_slim_residual=True, no_levels=3,
    downsample_parameters=((4, 2, 1, 1),) * 3, upsample_parameters=((4, 2, 1, 0, 1),) * 3, no_res_layers=3, no_channels=256, codebook_type="ema",
    num_embeddings=(256,), embedding_dim=(256,), embedding_init=("normal",), commitment_cost=(0.25,), decay=(0.99,), decay_warmup=None,
    max_decay_epochs=50, norm=None, dropout=0.0, act="RELU", output_act=None, evaluation_checkpoint="recent", load_nii_canonical=True,
    output_ext=".npy", output_dtype="float32", perceptual_weights=None,
    codebook_restart_patience=None, codebook_restart_max=32,
    anomaly_codes=None, anomaly_weight="mask", anomaly_sigma=None, anomaly_residual="abs", anomaly_threshold=None, anomaly_hist_max=1.0, anomaly_labels=None,
    anomaly_ensemble=None, anomaly_min_component=None, anomaly_connectivity=26,
    anomaly_median=None, anomaly_mask=None, anomaly_mask_threshold=0.0, anomaly_mask_erosion=0,
)
MODES = ["training", "extracting", "decoding", "anomaly"]


def _check_output_flags(cfg):
    """--output_ext / --output_dtype act or refuse (before anything touches the device)."""
    ext, dt, n_aug = cfg["output_ext"], cfg["output_dtype"], int(cfg["no_augmented_extractions"] or 0)
    if ext not in (".npy", ".nii", ".nii.gz"):
        raise ValueError(f"--output_ext={ext}: choices are .npy, .nii and .nii.gz")
    if dt not in ("float32", "int16", "uint8"):
        raise ValueError(f"--output_dtype={dt}: choices are float32, int16 and uint8")
    if ext == ".npy" and dt != "float32":
        raise ValueError(f"--output_dtype={dt} needs a NIfTI --output_ext (.nii or .nii.gz): .npy outputs are float32")
    if ext != ".npy" and cfg["mode"] == "training":
        raise ValueError(f"--output_ext={ext}: --mode=training writes no volumes (the flag belongs to --mode=extracting and --mode=decoding)")
    if ext != ".npy" and n_aug > 0:
        raise ValueError(f"--output_ext={ext} with --no_augmented_extractions={n_aug}: augmented extractions are not on the source grid and exist for "
                         "their codes; leave --output_ext at .npy")


def _check_codebook_flags(cfg):
    """--codebook_restart_patience / --codebook_restart_max and --decay_warmup / --max_decay_epochs act or refuse, before anything touches the
    device."""
    from synthanatomy_amd.networks.vqvae.baseline import check_restart_args
    from synthanatomy_amd.networks.vqvae.configure import check_decay_warmup
    check_decay_warmup(cfg)
    p, r = cfg["codebook_restart_patience"], cfg["codebook_restart_max"]
    if p is not None and cfg["mode"] != "training":
        raise ValueError(f"--codebook_restart_patience={p}: codes are restarted by training steps (--mode=training), not by --mode={cfg['mode']}")
    if r != DEFAULTS["codebook_restart_max"] and cfg["mode"] != "training":
        raise ValueError(f"--codebook_restart_max={r}: codes are restarted by training steps (--mode=training), not by --mode={cfg['mode']}")
    try:
        check_restart_args(1 if p is None else p, r)
    except ValueError as e:
        raise ValueError(f"--{e}") from None
    if p is None and r != DEFAULTS["codebook_restart_max"]:
        raise ValueError(f"--codebook_restart_max={r} needs --codebook_restart_patience=<steps>: without it no code is ever restarted")
    if p is not None and cfg["codebook_type"] != "ema":
        raise ValueError(f"--codebook_restart_patience={p}: restarts belong to the EMA quantizer (--codebook_type=ema)")


def _check_perceptual_flags(cfg):
    """--loss=*perceptual (LPIPS-alex) and --loss=baseline (LPIPS-squeeze) need --perceptual_weights: the file is read and checked by key and shape here, on
    the host, before anything touches the device (wrong weights, the other network's included, are refused by name, never replaced).  Returns the validated
    state dict, or None for every other loss."""
    if not str(cfg["loss"]).endswith("perceptual") and cfg["loss"] != "baseline":
        return None
    net = "squeeze" if cfg["loss"] == "baseline" else "alex"
    spec = cfg.get("perceptual_weights")
    if not spec:
        raise ValueError(f"--loss={cfg['loss']} needs --perceptual_weights=<file | random:seed>: a torch.save'd dict in the key layout of "
                         f"lpips.LPIPS(net='{net}').state_dict() (tools/make_lpips_weights.py merges the two upstream files; nothing is downloaded)")
    from synthanatomy_amd.losses.lpips import load_weights
    return load_weights(str(spec), net=net)


def _output_path(cfg, filename, postfix):
    """``<outputs>/<name>/<name>_<postfix><--output_ext>``: utils.general.save_npy's layout."""
    name = os.path.basename(filename)
    for ext in (".nii.gz", ".nii", ".npy"):
        if name.endswith(ext):
            name = name[:-len(ext)]
    return os.path.join(cfg["outputs_directory"], name, f"{name}_{postfix}{cfg['output_ext']}")


def _roi_shape(cfg):
    return tuple(int(b - a) for a, b in cfg["roi"])


def _load_volume(path, cfg, gen, dev, block=None):
    if path.startswith("synthetic"):   # a volume that depends on its NAME only (not on how many were drawn before it): resumable, rank-independent
        g = torch.Generator(device=dev).manual_seed(cfg["seed"] * 1000003 + int(path.split("_")[-1]))
        return torch.rand(1, *_roi_shape(cfg), generator=g, device=dev)
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
    from synthanatomy_amd.utils.nifti import header_orientation, read_nifti
    from synthanatomy_amd.utils.vqvae import hip_ingest, pad_to_roi, roi_shape, roi_window
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
    from synthanatomy_amd.utils.nifti import read_nifti
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
    from synthanatomy_amd.utils.vqvae import pad_to_roi, roi_shape, roi_window
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
    from synthanatomy_amd.utils.vqvae import draw_augmentation, hip_augment, in_window, roi_shape
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


def _augmented_name(f, i):
    """get_subjects' augmentation_id in the file name (reference src/utils/vqvae.py:601-608): <name>_<i><extension>"""
    for ext in (".nii.gz", ".nii", ".npy"):
        if f.endswith(ext):
            return f[:-len(ext)] + f"_{i}" + ext
    return f"{f}_{i}"


def build_network(cfg, dev):
    from synthanatomy_amd.networks.vqvae.configure import get_vqvae_network
    cfg = dict(cfg)
    cfg["compute_dtype"] = torch.bfloat16 if cfg["amp"] else torch.float32  # --amp=True (reference: fp16 autocast) -> bf16 MFMA
    return get_vqvae_network(cfg).to(dev)


def _evaluate(net, files, cfg, gen, dev, rank, world, win_size, epoch=0, index_base=0):
    """The evaluator of run_vqvae.py:122-146,248-289 over the validation subjects: ``mse`` is the mean reconstruction MSE this build has always
    logged (``hip_mse``), ``metrics`` the reference's Metric-MS-SSIM_<w> (when ``win_size`` is not None), Metric-MAE and Metric-MSE-Reconstruction
    (synthanatomy_amd.metrics.vqvae; each all-reduces its sum and count over the ranks in ``compute``).  With ``--augmentation=True`` the batches are
    augmented like the training ones (upstream builds the evaluation transform with the same patch_size and augmentations), drawn for
    (``epoch``, ``index_base`` + the subject's index)."""
    from synthanatomy_amd.losses.vqvae import hip_mse
    from synthanatomy_amd.metrics.vqvae import MAE, MSE, MultiScaleSSIM
    import torch.distributed as dist
    metrics = {}
    if win_size is not None:
        metrics[f"Metric-MS-SSIM_{win_size}-Reconstruction"] = MultiScaleSSIM(ms_ssim_kwargs={"win_size": win_size})
    metrics["Metric-MAE-Reconstruction"] = MAE()
    metrics["Metric-MSE-Reconstruction"] = MSE()
    was = net.training
    net.eval()
    tot = torch.zeros(2, device=dev, dtype=torch.float64)
    with torch.no_grad():
        order = shard_for_rank(len(files), rank, world, shuffle=False, pad=False)
        if cfg.get("augmentation"):
            batches = _augmented_batches([(files[k], files[k], epoch, index_base + k) for k in order], cfg["eval_batch_size"], cfg, dev, "training",
                                         lambda k: _noise_seed(cfg["seed"], ((epoch << 24) + k) * world + rank, 1))
        else:
            batches = _batches(files, order, cfg["eval_batch_size"], cfg, gen, dev)
        for _, x, *_ in batches:
            rec = net(x)["reconstruction"][0]
            tot[0] += hip_mse(rec, x).double() * x.shape[0]
            tot[1] += x.shape[0]
            for m in metrics.values():
                m.update((rec, x))
    if world > 1:
        dist.all_reduce(tot)
    net.train(was)
    return float(tot[0] / tot[1].clamp(min=1)), {k: m.compute() for k, m in metrics.items()}


def training(cfg, rank, local, world, dev):
    from synthanatomy_amd.engines.trainer import AdversarialTrainer
    from synthanatomy_amd.losses.adversarial import get_discriminator_loss, get_generator_loss
    from synthanatomy_amd.losses.vqvae import gdl_factor_schedule, get_vqvae_loss
    from synthanatomy_amd.networks.vqvae.configure import decay_schedule
    from synthanatomy_amd.runtime.ddp import GradReducer
    from synthanatomy_amd.runtime.optim import ExponentialLR, FlatParams, FusedAdam, TrainerState
    loss_fn = get_vqvae_loss(dict(cfg, perceptual_weights=cfg.get("perceptual_state") or cfg.get("perceptual_weights")))
    baur = cfg["loss"] == "baur"      # gdl_factor scheduled at every finished epoch (src/losses/vqvae/configure.py:56-76)
    perceptual = hasattr(loss_fn, "set_step")      # the LPIPS family: frozen weights as buffers on the device, slice draw keyed on the global iteration
    if perceptual:
        loss_fn.to(dev)
        if str(cfg.get("perceptual_weights")).startswith("random:"):
            log(rank, f"--perceptual_weights={cfg['perceptual_weights']}: seeded STAND-IN weights (tests, smoke runs, benchmarks): the perceptual term measures nothing")
    net = build_network(cfg, dev).train()
    flat = FlatParams(net.parameters())
    red = GradReducer(flat)
    net.set_grad_sink(red)
    from synthanatomy_amd import debug
    if cfg["adversarial_component"] or not debug.host("opt_in_backward"):      # (the adversarial iteration runs several backward passes per optimizer step)
        opt = FusedAdam(flat, lr=cfg["learning_rate"])
        opt.on_step.append(net.invalidate_packed_weights)
    else:                                 # SA_OPT_IN_BACKWARD=1: a bucket's Adam slice + operand re-pack run behind its gradients (runtime/optim.py)
        opt = FusedAdam(flat, lr=cfg["learning_rate"], in_backward=red)
        repacker = net.range_repacker(flat)
        opt.on_range.append(repacker)
        opt.on_step.append(repacker.finish)
    gamma = float(cfg["gamma"]) if cfg["gamma"] != "auto" else 0.99999
    sched = ExponentialLR(opt, gamma=gamma)
    files = list_inputs(cfg["training_subjects"])
    val_files = list_inputs(cfg["validation_subjects"])
    per_rank = (len(files) + world - 1) // world
    epoch_length = cfg["training_epoch_length"] or (per_rank + cfg["batch_size"] - 1) // cfg["batch_size"]
    state = TrainerState(epoch_length=epoch_length, max_epochs=cfg["epochs"])
    to_save = {"network": net, "optimizer": opt, "lr_scheduler": sched, "trainer": state}
    restarting = cfg["codebook_restart_patience"] is not None      # dead-code restarts: the donor draw is keyed on (--seed, global iteration)
    if restarting:
        net.set_codebook_restart(cfg["codebook_restart_patience"], cfg["codebook_restart_max"], cfg["seed"])
        to_save["codebook_restart"] = net.codebook_restart_state()      # idle counters + running total: resuming equals not stopping
    warming = cfg["decay_warmup"] is not None                      # EMA decay scheduled at every finished epoch (networks/vqvae/configure.py: decay_schedule)
    decay_cfg = dict(cfg, epoch_length=epoch_length)
    trainer = None
    if cfg["adversarial_component"]:
        from synthanatomy_amd.networks.discriminator.configure import get_discriminator_network
        dcfg = dict(cfg, compute_dtype=torch.bfloat16 if cfg["amp"] else torch.float32)
        disc = get_discriminator_network(dcfg).to(dev).train()
        d_flat = FlatParams(disc.parameters())
        d_opt = FusedAdam(d_flat, lr=cfg["discriminator_learning_rate"])
        d_opt.on_step.append(disc.invalidate_packed_weights)
        d_sched = ExponentialLR(d_opt, gamma=gamma)
        trainer = AdversarialTrainer(net, opt, get_generator_loss(cfg), loss_fn, disc, d_opt, get_discriminator_loss(cfg),
                                     use_adversarial_adaptive_weight=cfg["use_adversarial_adaptive_weight"],
                                     adaptive_adversarial_weight_threshold=cfg["adaptive_adversarial_weight_threshold"],
                                     adaptive_adversarial_weight_value=cfg["adaptive_adversarial_weight_value"],
                                     g_reducer=red, d_reducer=GradReducer(d_flat), g_scheduler=sched, d_scheduler=d_sched)
        to_save.update(d_network=disc, d_optimizer=d_opt, d_lr_scheduler=d_sched)
    # resume (run_vqvae.py:328-345): everything in to_save, except the d_* entries when the adversarial component is being fine-tuned in
    ckpt = check_for_checkpoints(cfg)
    if ckpt:
        to_load = {k: v for k, v in to_save.items() if not (cfg["finetune_adversarial_component"] and k.startswith("d_")) and k != "codebook_restart"}
        loaded = load_checkpoint(ckpt, to_load, map_location=dev)
        if restarting and "codebook_restart" in loaded:
            to_save["codebook_restart"].load_state_dict(loaded["codebook_restart"])
        elif restarting:
            log(rank, f"{ckpt} has no codebook_restart entry (written without --codebook_restart_patience): the idle counters start at zero")
        state.rebase(epoch_length, cfg["epochs"])      # finished epochs by the CHECKPOINT's epoch length; this run's data set / --epochs decide the rest
        net.invalidate_packed_weights()
        log(rank, f"resumed from {ckpt}: epoch {state.epoch}, iteration {state.iteration}, lr {opt.lr:.6e}")
        if baur and state.epoch > 0:      # (upstream restarts at the class default 0.0 for this epoch; resuming equals not stopping here)
            loss_fn.set_gdl_factor(gdl_factor_schedule(cfg, state.epoch))
        if warming:
            net.set_ema_decay(decay_schedule(decay_cfg, state.epoch))
            log(rank, f"resumed with --decay_warmup={cfg['decay_warmup']}: decay {net.get_ema_decay()[0]:.6g}")
    # key metric (run_vqvae.py:122): MS-SSIM with get_ms_ssim_window's window; where the reference refuses to start (smallest side < 48), -MSE
    from synthanatomy_amd.utils.vqvae import get_ms_ssim_window
    try:      # (--augmentation with --patch_size: the evaluator sees patches, so they size the window unless --eval_patch_size does)
        win_size = get_ms_ssim_window(dict(cfg, eval_patch_size=cfg["eval_patch_size"] or cfg["patch_size"]) if cfg["augmentation"] else cfg)
    except ValueError as e:
        win_size = None
        log(rank, f"MS-SSIM key metric unavailable ({e}): the best checkpoint is chosen by -validation mse")
    key_name = f"Metric-MS-SSIM_{win_size}-Reconstruction" if win_size is not None else None
    gen = torch.Generator(device=dev).manual_seed(cfg["seed"] + rank)
    from synthanatomy_amd.utils.vqvae import check_patch_size
    check_patch_size(cfg, "training")
    augmenting = bool(cfg["augmentation"] or cfg["patch_size"])      # training batches go through sa_augment (--patch_size alone: the random crop only)
    for epoch in range(state.epoch, cfg["epochs"]):
        # DistributedSampler semantics: one epoch-seeded permutation shared by all ranks, padded so every rank runs the same number of steps
        order = shard_for_rank(len(files), rank, world, epoch=epoch, seed=cfg["seed"])
        done = 0
        if augmenting:
            batches = _augmented_batches([(files[k], files[k], epoch, k) for k in order], cfg["batch_size"], cfg, dev, "training",
                                         lambda k: _noise_seed(cfg["seed"], (state.iteration + 1) * world + rank))
        else:
            batches = _batches(files, order, cfg["batch_size"], cfg, gen, dev)
        for names, x, *noise_seed in batches:
            if perceptual:
                loss_fn.set_step(state.iteration * world + rank)
            if restarting:
                net.set_codebook_restart_step(state.iteration)      # identical on all ranks
            if trainer is not None:
                res = trainer.iteration(x, x, epoch + 1)      # ignite's state.epoch is 1 during the first epoch (trainer.py:176)
                loss = res["loss"]
            else:
                flat.zero_grad()
                out = net(x)
                loss = loss_fn(out, x)
                loss.backward()
                opt.step(grad_scale=red.finish())
                sched.step()
                res = None
            state.iteration += 1
            done += 1
            if state.iteration % cfg["log_every"] == 0:
                extra = f" g_loss {float(res['g_loss']):.6f} d_loss {float(res['d_loss']):.6f} adv_weight {float(res['adversarial_weight']):.4f}" if res else ""
                if baur:
                    extra += f" gdl_factor {loss_fn.get_gdl_factor():.6g}"
                if perceptual:
                    extra += "".join(f" {k} {float(v):.6g}" for k, v in loss_fn.get_summaries()["scalar"].items() if k.startswith("Loss-" if cfg["loss"] == "baseline" else "Loss-Perceptual_"))
                if augmenting:
                    extra += f" input {'x'.join(str(n) for n in x.shape[2:])} noise_seed {noise_seed[0]:#018x}"
                if restarting:
                    info = net.get_codebook_restart_info()
                    extra += f" codebook_dead {info['dead']} restarted {info['restarted']}"
                log(rank, f"epoch {epoch} it {state.iteration} loss {loss.item():.6f}{extra} perplexity {net.get_perplexity()[0].item():.2f} lr {opt.lr:.3e}")
            if done == epoch_length:
                break
        state.iteration = (epoch + 1) * epoch_length      # (a short last batch list still closes the epoch)
        if baur:                                          # ParamSchedulerHandler(epoch_level=True) at EPOCH_COMPLETED, state.epoch = finished epochs
            loss_fn.set_gdl_factor(gdl_factor_schedule(cfg, epoch + 1))
        if warming:                                       # the same handler on set_ema_decay (src/networks/vqvae/configure.py:42-86)
            net.set_ema_decay(decay_schedule(decay_cfg, epoch + 1))
            log(rank, f"epoch {epoch} decay {net.get_ema_decay()[0]:.6g}")
        if (epoch + 1) % cfg["eval_every"] == 0 and val_files:
            mse, metrics = _evaluate(net, val_files, cfg, gen, dev, rank, world, win_size, epoch=epoch, index_base=len(files))
            log(rank, f"epoch {epoch} validation mse {mse:.6f}")
            log(rank, f"epoch {epoch} validation " + " ".join(f"{k} {v:.6f}" for k, v in metrics.items()))
            if rank == 0:                                                       # evaluator's key-metric checkpoint, key_metric_n_saved=1
                if key_name is not None:
                    save_checkpoint(cfg, epoch + 1, to_save, key_metric=metrics[key_name], key_metric_name=key_name)
                else:
                    save_checkpoint(cfg, epoch + 1, to_save, key_metric=-mse)
        if rank == 0 and (epoch + 1) % cfg["checkpoint_every"] == 0:
            save_checkpoint(cfg, epoch + 1, to_save)                            # ignite numbers checkpoints by finished epochs
    if rank == 0:
        torch.save(net.state_dict(), os.path.join(cfg["checkpoint_directory"], f"model_state_dict_epoch={cfg['epochs']}.pt"))


def inference(cfg, rank, local, world, dev):
    net = build_network(cfg, dev).eval()
    path = check_for_checkpoints(cfg)     # starting_epoch > 0: that epoch; else evaluation_checkpoint = "recent" | "best"
    if path:
        load_network_state(net, path)
        log(rank, f"loaded {path}")
    gen = torch.Generator(device=dev).manual_seed(cfg["seed"] + rank)
    files = list_inputs(cfg["validation_subjects"] if cfg["mode"] == "extracting" else cfg["training_subjects"])
    saver = None
    if cfg["output_ext"] != ".npy":      # volumes leave through sa_volume_egress and writer threads; the codes stay uint16 .npy
        from synthanatomy_amd.utils.vqvae import NiftiSaver, nifti_output_geometry
        saver = NiftiSaver(cfg["output_ext"], cfg["output_dtype"], min(int(cfg.get("num_workers") or 0), 8))
        canonical = bool(cfg.get("load_nii_canonical", True))
    try:
        with torch.no_grad():
            if cfg["mode"] == "extracting":
                order = shard_for_rank(len(files), rank, world, shuffle=False, pad=False)   # even_divisible=False: no duplicates, no collectives
                n_aug = int(cfg["no_augmented_extractions"] or 0)
                if n_aug > 0:      # every subject n_aug times, augmentation_id i drawn as "epoch" i (reference src/utils/vqvae.py:126-181,194-196)
                    batches = _augmented_batches([(_augmented_name(files[k], i), files[k], i, k) for k in order for i in range(n_aug)], cfg["eval_batch_size"],
                                                 cfg, dev, "extracting", lambda k: _noise_seed(cfg["seed"], k * world + rank, 2))
                else:
                    batches = _batches(files, order, cfg["eval_batch_size"], cfg, gen, dev)
                for names, x, *headers in batches:
                    idx = net.index_quantize(x)[0]
                    rec = net.decode_samples([idx])
                    if saver is None:
                        for n, i_, r_ in zip(names, idx.cpu().numpy(), rec.float().cpu().numpy()):
                            save_npy(i_, cfg["outputs_directory"], n, "quantization_0", np.uint16)
                            save_npy(r_[0], cfg["outputs_directory"], n, "reconstruction", np.float32)
                    else:          # straight from the decoder's output tensor, in the source file's own axes; the writers work while the next batch runs
                        saver.batch()
                        for n, r_, h in zip(names, rec, headers[0]):
                            saver.save(r_[0], _output_path(cfg, n, "reconstruction"), *nifti_output_geometry(h, cfg["roi"], canonical, r_.shape[-3:]))
                        for n, i_ in zip(names, idx.cpu().numpy()):
                            save_npy(i_, cfg["outputs_directory"], n, "quantization_0", np.uint16)
            else:  # decoding: .npy uint16 code grids -> reconstructions (prepare_decoding_batch: .long())
                files = list_inputs(cfg["training_subjects"], postfix="sample")[rank::world]
                group = max(min(int(cfg.get("num_workers") or 0), 8), 1)      # decoded volumes per batch of the saver: one per writer thread
                for k, f in enumerate(files):
                    codes = np.load(f).astype(np.int64)
                    if codes.min() < 0 or codes.max() >= net.n_embed:   # e.g. a sampled BOS id (== vocab_size): torch's embedding lookup raises upstream too
                        raise ValueError(f"{f}: code {int(codes.max())} is not a codebook entry (num_embeddings={net.n_embed})")
                    idx = torch.from_numpy(codes)[None].to(dev)
                    rec = net.decode_samples([idx])
                    if saver is None:
                        save_npy(rec[0, 0].float().cpu().numpy(), cfg["outputs_directory"], f, "sample", np.float32)
                    else:          # no source metadata (upstream has none here either): the identity orientation and affine
                        if k % group == 0:
                            saver.batch()
                        saver.save(rec[0, 0], _output_path(cfg, f, "sample"))
    finally:
        if saver is not None:      # every writer is joined (and its exception re-raised here) before "done"
            saver.close()
    log(rank, f"{cfg['mode']} done: {len(files)} inputs -> {cfg['outputs_directory']}")


def _stem(path):
    name = os.path.basename(path)
    for ext in (".nii.gz", ".nii", ".npy"):
        if name.endswith(ext):
            return name[:-len(ext)]
    return name


def _downsampling_factor(cfg):
    f = 1
    for p in list(cfg["downsample_parameters"])[:int(cfg["no_levels"])]:
        f *= int(p[1])
    return f


def _anomaly_sigma(cfg):
    """--anomaly_sigma, or half the largest down-sampling factor of the network the flags describe"""
    return cfg["anomaly_sigma"] if cfg["anomaly_sigma"] is not None else _downsampling_factor(cfg) / 2.0


def _ensemble_specs(cfg):
    """--anomaly_ensemble as a list of specs (a comma-separated string, a tuple or a list), or None without the flag"""
    v = cfg["anomaly_ensemble"]
    if v is None:
        return None
    return v.split(",") if isinstance(v, str) else list(v) if isinstance(v, (tuple, list)) else [v]


def _check_anomaly_flags(cfg):
    """the --anomaly_* flags act or refuse (before anything touches the device)"""
    from synthanatomy_amd.metrics.anomaly import MAX_MEMBERS, MAX_SIGMA, RESIDUALS
    from synthanatomy_amd.metrics.components import CONNECTIVITIES
    _check_median_flags(cfg)
    for name, given in (("anomaly_min_component", cfg["anomaly_min_component"] is not None),
                        ("anomaly_connectivity", cfg["anomaly_connectivity"] != DEFAULTS["anomaly_connectivity"])):
        if not given:
            continue
        flag = f"--{name}={cfg[name]}"
        if cfg["mode"] != "anomaly":
            raise ValueError(f"{flag}: the flag belongs to --mode=anomaly, not --mode={cfg['mode']}")
        if cfg["anomaly_threshold"] is None:
            raise ValueError(f"{flag}: the components are those of [map >= --anomaly_threshold], which is not given")
    n = cfg["anomaly_min_component"]
    if n is not None and (isinstance(n, bool) or not isinstance(n, int) or n < 1 or n >= 2 ** 31 - 1):
        raise ValueError(f"--anomaly_min_component={n}: an integer >= 1 (voxels) or None is needed")
    c = cfg["anomaly_connectivity"]
    if isinstance(c, bool) or c not in CONNECTIVITIES:
        raise ValueError(f"--anomaly_connectivity={c}: choices are 6, 18 and 26")
    specs = _ensemble_specs(cfg)
    if specs is not None:
        flag = f"--anomaly_ensemble={cfg['anomaly_ensemble']}"
        if cfg["mode"] != "anomaly":
            raise ValueError(f"{flag}: the flag belongs to --mode=anomaly, not --mode={cfg['mode']}")
        for sp in specs:
            if not isinstance(sp, str):
                raise ValueError(f"{flag}: {sp!r} is not a directory or a glob (a comma-separated string or a tuple of strings is needed)")
            if not sp.strip():
                raise ValueError(f"{flag}: an empty spec (one directory or glob per member is needed)")
        if not 2 <= len(specs) <= MAX_MEMBERS:
            raise ValueError(f"{flag}: {len(specs)} members, 2 to {MAX_MEMBERS} are needed (one healing: --anomaly_codes)")
        twice = sorted({sp for sp in specs if specs.count(sp) > 1})
        if twice:
            raise ValueError(f"{flag}: {twice[0]} is given twice (every member needs its own healing outputs)")
        if cfg["anomaly_codes"] is not None:
            raise ValueError(f"{flag} with --anomaly_codes={cfg['anomaly_codes']}: the ensemble names every member's outputs itself; give one of the two")
    if cfg["anomaly_weight"] not in ("mask", "nll", "none"):
        raise ValueError(f"--anomaly_weight={cfg['anomaly_weight']}: choices are mask, nll and none")
    if cfg["anomaly_residual"] not in RESIDUALS:
        raise ValueError(f"--anomaly_residual={cfg['anomaly_residual']}: choices are abs, positive and negative")
    sigma = _anomaly_sigma(cfg)
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not 0 <= sigma <= MAX_SIGMA:
        raise ValueError(f"--anomaly_sigma={sigma}: a number in [0, {MAX_SIGMA:g}] or None (half the down-sampling factor) is needed")
    t = cfg["anomaly_threshold"]
    if t is not None and (isinstance(t, bool) or not isinstance(t, (int, float)) or t != t or abs(t) == float("inf")):
        raise ValueError(f"--anomaly_threshold={t}: a finite number or None is needed")
    hm = cfg["anomaly_hist_max"]
    if isinstance(hm, bool) or not isinstance(hm, (int, float)) or not 0 < hm < float("inf"):
        raise ValueError(f"--anomaly_hist_max={hm}: a finite number > 0 is needed")
    if cfg["anomaly_codes"] is not None and not isinstance(cfg["anomaly_codes"], str):
        raise ValueError(f"--anomaly_codes={cfg['anomaly_codes']}: a directory or a glob is needed")
    if int(cfg["no_augmented_extractions"] or 0) > 0:
        raise ValueError(f"--no_augmented_extractions={cfg['no_augmented_extractions']}: --mode=anomaly compares every scan with its own healed codes")


MEDIAN_FLAGS = ("anomaly_median", "anomaly_mask", "anomaly_mask_threshold", "anomaly_mask_erosion")


def _median_flags_given(cfg):
    return [name for name in MEDIAN_FLAGS if cfg[name] is not None and (isinstance(cfg[name], bool) or cfg[name] != DEFAULTS[name])]


def _check_median_flags(cfg):
    """--anomaly_median / --anomaly_mask / --anomaly_mask_threshold / --anomaly_mask_erosion act or refuse, each by its name"""
    from synthanatomy_amd.metrics.median import MAX_EROSION, SIZES
    for name in _median_flags_given(cfg):
        if cfg["mode"] != "anomaly":
            raise ValueError(f"--{name}={cfg[name]}: the flag belongs to --mode=anomaly, not --mode={cfg['mode']}")
    k = cfg["anomaly_median"]
    if k is not None and (isinstance(k, bool) or not isinstance(k, int) or k not in SIZES):
        raise ValueError(f"--anomaly_median={k}: choices are 1, 3 and 5 (the window's side) or None")
    mask = cfg["anomaly_mask"]
    if mask is not None and (not isinstance(mask, str) or not mask.strip()):
        raise ValueError(f"--anomaly_mask={mask}: scan, a directory or a glob is needed")
    mt = cfg["anomaly_mask_threshold"]
    if isinstance(mt, bool) or not isinstance(mt, (int, float)) or mt != mt or abs(mt) == float("inf"):
        raise ValueError(f"--anomaly_mask_threshold={mt}: a finite number is needed")
    if mt != DEFAULTS["anomaly_mask_threshold"] and mask != "scan":
        raise ValueError(f"--anomaly_mask_threshold={mt}: the flag thresholds the scan and needs --anomaly_mask=scan (given: {mask})")
    e = cfg["anomaly_mask_erosion"]
    if isinstance(e, bool) or not isinstance(e, int) or not 0 <= e <= MAX_EROSION:
        raise ValueError(f"--anomaly_mask_erosion={e}: an integer in 0..{MAX_EROSION} is needed")
    if e > 0 and mask is None:
        raise ValueError(f"--anomaly_mask_erosion={e}: there is nothing to erode without --anomaly_mask")


def find_healing_outputs(subjects, spec, weight="mask"):
    """For every subject the files ``run_transformer.save_healing`` wrote for its codes, found by stem under ``spec`` (a directory, searched recursively,
    or a glob): ``<stem>_quantization_0_healed_sample.npy`` and next to it ``..._resampled.npy`` / ``..._nll.npy`` (``weight`` = mask / nll says which
    one is needed).  One dict per subject (keys healed, resampled, nll); a subject with no match, or with more than one, is refused by name."""
    import glob
    found = set()
    for hit in ([spec] if os.path.isdir(spec) else glob.glob(spec, recursive=True)):      # a directory the glob matches is searched like one given
        if os.path.isdir(hit):
            found.update(glob.glob(os.path.join(hit, "**", "*_healed_sample.npy"), recursive=True))
        elif hit.endswith("_healed_sample.npy"):
            found.add(hit)
    found = sorted(found)
    out = []
    for s in subjects:
        want = f"{_stem(s)}_quantization_0_healed_sample.npy"
        hits = [f for f in found if os.path.basename(f) == want]
        if not hits:
            raise ValueError(f"{s}: no healing output {want} under {spec} (run_transformer.py --mode=healing writes it; see --anomaly_codes)")
        if len(hits) > 1:
            raise ValueError(f"{s}: {len(hits)} healing outputs named {want} under {spec} ({', '.join(hits)}): narrow --anomaly_codes")
        base = hits[0][:-len("healed_sample.npy")]
        rec = {"healed": hits[0], "resampled": base + "resampled.npy", "nll": base + "nll.npy"}
        need = {"mask": "resampled", "nll": "nll"}.get(weight)
        if need and not os.path.exists(rec[need]):
            raise ValueError(f"{s}: {os.path.basename(rec[need])} is missing next to {hits[0]} (--anomaly_weight={weight} needs it)")
        out.append(rec)
    return out


def find_ensemble_outputs(subjects, specs, weight="mask"):
    """``find_healing_outputs`` once per member spec: a list over the members of lists over the subjects.  A subject whose two members resolve to the
    same healed file, and a member whose code grid differs in shape from member 0's, are refused by name (host only: the ``.npy`` headers are read)."""
    members = [find_healing_outputs(subjects, spec, weight) for spec in specs]
    for j, s in enumerate(subjects):
        seen = {}
        for k, recs in enumerate(members):
            real = os.path.realpath(recs[j]["healed"])
            if real in seen:
                raise ValueError(f"{s}: members {seen[real]} ({specs[seen[real]]}) and {k} ({specs[k]}) of --anomaly_ensemble resolve to the same "
                                 f"healed file {recs[j]['healed']}")
            seen[real] = k
        shapes = [np.load(recs[j]["healed"], mmap_mode="r").shape for recs in members]
        for k, shp in enumerate(shapes):
            if shp != shapes[0]:
                raise ValueError(f"{s}: member {k} ({specs[k]}) of --anomaly_ensemble has a code grid of shape {shp}, member 0 ({specs[0]}) has "
                                 f"{shapes[0]}")
    return members


def match_labels(subjects, spec, flag="anomaly_labels", what="label"):
    """the label volume of every subject, matched by stem among ``list_inputs(spec)``; a subject without exactly one is refused by name
    (``--anomaly_mask=<dir|glob>`` finds its mask volumes the same way)"""
    found = list_inputs(spec)
    out = []
    for s in subjects:
        hits = [f for f in found if _stem(f) == _stem(s)]
        if len(hits) != 1:
            raise ValueError(f"{s}: {len(hits)} {what} volumes with the stem {_stem(s)} in --{flag}={spec} (exactly one is needed)")
        out.append(hits[0])
    return out


def anomaly(cfg, rank, local, world, dev):
    """--mode=anomaly: every validation subject against the decoding of its healed codes, on the device from the scan to the scores."""
    import csv
    from synthanatomy_amd.metrics.anomaly import anomaly_map, anomaly_map_ensemble, average_precision, best_dice, dice_from_counts
    from synthanatomy_amd.metrics.components import connected_components, lesion_scores
    from synthanatomy_amd.metrics.median import median_filter_map
    min_component = cfg["anomaly_min_component"]
    filtered = cfg["anomaly_median"] is not None or cfg["anomaly_mask"] is not None      # DESIGN 7.18; a mask alone is size 1
    files = list_inputs(cfg["validation_subjects"])
    specs = _ensemble_specs(cfg)      # K healings per subject, one fused map; None: the single healing of 7.11
    if specs is None:
        members = [find_healing_outputs(files, cfg["anomaly_codes"] or cfg["outputs_directory"], cfg["anomaly_weight"])]      # host only: refusals come first
    else:
        members = find_ensemble_outputs(files, specs, cfg["anomaly_weight"])
    label_files = match_labels(files, cfg["anomaly_labels"]) if cfg["anomaly_labels"] is not None else None
    mask_files = None
    if cfg["anomaly_mask"] not in (None, "scan"):
        mask_files = match_labels(files, cfg["anomaly_mask"], "anomaly_mask", "mask")
    sigma = _anomaly_sigma(cfg)
    net = build_network(cfg, dev).eval()
    path = check_for_checkpoints(cfg)
    if path:
        load_network_state(net, path)
        log(rank, f"loaded {path}")
    gen = torch.Generator(device=dev).manual_seed(cfg["seed"] + rank)
    saver = None
    if cfg["output_ext"] != ".npy":
        from synthanatomy_amd.utils.vqvae import NiftiSaver, nifti_output_geometry
        saver = NiftiSaver(cfg["output_ext"], cfg["output_dtype"], min(int(cfg.get("num_workers") or 0), 8))
        canonical = bool(cfg.get("load_nii_canonical", True))
    index = {f: k for k, f in enumerate(files)}
    order = shard_for_rank(len(files), rank, world, shuffle=False, pad=False)
    raw_cfg = dict(cfg, normalize=False)      # label volumes: the scans' reorientation and ROI, never their normalisation
    rows = []
    try:
        with torch.no_grad():
            for names, x, headers in _batches(files, order, cfg["eval_batch_size"], cfg, gen, dev):
                recs, wgts = [], []      # per member: the decoding [B, 1, D, H, W] and the weight grids [B, d, h, w]
                for healed in members:      # member by member: each decode_samples call is the one a single-healing run makes for this batch
                    grids, weights = [], []
                    for n in names:
                        h = healed[index[n]]
                        codes = np.load(h["healed"]).astype(np.int64)
                        if codes.min() < 0 or codes.max() >= net.n_embed:      # the check of --mode=decoding
                            raise ValueError(f"{h['healed']}: code {int(codes.max())} is not a codebook entry (num_embeddings={net.n_embed})")
                        grids.append(torch.from_numpy(codes))
                        if cfg["anomaly_weight"] != "none":
                            wgt = np.load(h["resampled" if cfg["anomaly_weight"] == "mask" else "nll"]).astype(np.float32)
                            if wgt.shape != codes.shape:
                                raise ValueError(f"{n}: the weight grid {wgt.shape} and the healed codes {codes.shape} differ in shape")
                            weights.append(torch.from_numpy(wgt))
                    rec = net.decode_samples([torch.stack(grids).to(dev)]).float()
                    if rec.shape != x.shape:
                        raise ValueError(f"{names[0]}: the healed codes decode to {tuple(rec.shape[2:])}, the scan is {tuple(x.shape[2:])} (--roi?)")
                    if specs is not None:
                        if not recs:
                            block = torch.empty((len(members),) + tuple(x.shape), dtype=torch.float32, device=dev)
                        block[len(recs)].copy_(rec)
                        rec = block[len(recs)]
                    recs.append(rec)
                    wgts.append(torch.stack(weights).to(dev) if weights else None)
                labels = None
                if label_files is not None:
                    labels = torch.stack([_load_volume(label_files[index[n]], raw_cfg, gen, dev).reshape(x.shape[1:]) for n in names])
                if specs is None:
                    amap, summ = anomaly_map(x, recs[0], wgts[0], sigma=sigma, residual=cfg["anomaly_residual"],
                                             labels=labels, threshold=cfg["anomaly_threshold"], hist_max=cfg["anomaly_hist_max"])
                else:
                    amap, summ = anomaly_map_ensemble(x, block, torch.stack(wgts) if wgts[0] is not None else None, sigma=sigma,
                                                      residual=cfg["anomaly_residual"], labels=labels, threshold=cfg["anomaly_threshold"],
                                                      hist_max=cfg["anomaly_hist_max"])
                fmap = fsumm = None
                if filtered:      # mask, median, mask again on the device; the components below take the filtered map
                    mask = None
                    if cfg["anomaly_mask"] == "scan":
                        mask = x > float(cfg["anomaly_mask_threshold"])
                    elif mask_files is not None:
                        mask = torch.stack([_load_volume(mask_files[index[n]], raw_cfg, gen, dev).reshape(x.shape[1:]) for n in names])
                    fmap, fsumm = median_filter_map(amap, size=cfg["anomaly_median"] or 1, mask=mask, erosion=cfg["anomaly_mask_erosion"], labels=labels,
                                                    threshold=cfg["anomaly_threshold"], hist_max=cfg["anomaly_hist_max"])
                seg = comp = None
                if min_component is not None:      # the map, single or ensemble, is still on the device
                    ids, comp = connected_components(fmap if filtered else amap, threshold=cfg["anomaly_threshold"], connectivity=int(cfg["anomaly_connectivity"]),
                                                     min_size=min_component, labels=labels)
                    seg = (ids > 0).float()
                posts = ["healed_reconstruction"] if specs is None else [f"healed_reconstruction_m{k}" for k in range(len(members))]
                if saver is None:
                    host = [rec.cpu().numpy() for rec in recs]
                    seg_host = seg.cpu().numpy() if seg is not None else None
                    f_host = fmap.cpu().numpy() if filtered else None
                    for j, (n, a_) in enumerate(zip(names, amap.cpu().numpy())):
                        save_npy(a_[0], cfg["outputs_directory"], n, "anomaly_map", np.float32)
                        if filtered:
                            save_npy(f_host[j, 0], cfg["outputs_directory"], n, "anomaly_map_filtered", np.float32)
                        if seg_host is not None:
                            save_npy(seg_host[j, 0], cfg["outputs_directory"], n, "anomaly_segmentation", np.float32)
                        for post, r_ in zip(posts, host):
                            save_npy(r_[j, 0], cfg["outputs_directory"], n, post, np.float32)
                else:
                    saver.batch()
                    for j, (n, a_, h) in enumerate(zip(names, amap, headers)):
                        geom = nifti_output_geometry(h, cfg["roi"], canonical, a_.shape[-3:])
                        saver.save(a_[0], _output_path(cfg, n, "anomaly_map"), *geom)
                        if filtered:
                            saver.save(fmap[j, 0], _output_path(cfg, n, "anomaly_map_filtered"), *geom)
                        if seg is not None:
                            saver.save(seg[j, 0], _output_path(cfg, n, "anomaly_segmentation"), *geom)
                        for post, rec in zip(posts, recs):
                            saver.save(rec[j, 0], _output_path(cfg, n, post), *geom)
                if comp is not None:
                    comp = {k: v.cpu().numpy() for k, v in comp.items() if v is not None}
                sums, maxs, hist = summ["sum"].cpu().numpy(), summ["max"].cpu().numpy(), summ["hist"].cpu().numpy()
                counts = [summ[k].cpu().numpy() for k in ("tp", "fp", "fn")] if summ["tp"] is not None else None
                if filtered:
                    fsums, fmaxs, fhist = fsumm["sum"].cpu().numpy(), fsumm["max"].cpu().numpy(), fsumm["hist"].cpu().numpy()
                    fcounts = [fsumm[k].cpu().numpy() for k in ("tp", "fp", "fn")] if fsumm["tp"] is not None else None
                for j, n in enumerate(names):
                    row = {"subject": _stem(n), "sum": repr(float(sums[j])), "max": repr(float(maxs[j]))}
                    if labels is not None:
                        bd, bt = best_dice(hist[j, 0], hist[j, 1], summ["inv_bin"])
                        row.update(dice="" if counts is None else repr(dice_from_counts(counts[0][j], counts[1][j], counts[2][j])),
                                   best_dice=repr(bd), best_dice_threshold=repr(bt), average_precision=repr(average_precision(hist[j, 0], hist[j, 1])))
                    if filtered:
                        row.update(filtered_sum=repr(float(fsums[j])), filtered_max=repr(float(fmaxs[j])))
                        if labels is not None:
                            bd, bt = best_dice(fhist[j, 0], fhist[j, 1], fsumm["inv_bin"])
                            row.update(filtered_dice="" if fcounts is None else repr(dice_from_counts(fcounts[0][j], fcounts[1][j], fcounts[2][j])),
                                       filtered_best_dice=repr(bd), filtered_best_dice_threshold=repr(bt),
                                       filtered_average_precision=repr(average_precision(fhist[j, 0], fhist[j, 1])))
                    if comp is not None:
                        row.update(components=str(int(comp["components"][j])), components_kept=str(int(comp["components_kept"][j])),
                                   voxels_kept=str(int(comp["voxels_kept"][j])), largest_component=str(int(comp["largest_component"][j])))
                        if labels is not None:
                            rc, pr, f1 = lesion_scores(comp["lesions"][j], comp["lesions_detected"][j], comp["components_kept"][j], comp["kept_true"][j])
                            row.update(dice_cleaned=repr(dice_from_counts(comp["tp"][j], comp["fp"][j], comp["fn"][j])),
                                       lesions=str(int(comp["lesions"][j])), lesions_detected=str(int(comp["lesions_detected"][j])),
                                       lesion_recall=repr(rc), lesion_precision=repr(pr), lesion_f1=repr(f1))
                    if specs is not None:
                        row["members"] = str(summ["members"])
                    rows.append(row)
    finally:
        if saver is not None:
            saver.close()
    fields = ["subject", "sum", "max"] + (["dice", "best_dice", "best_dice_threshold", "average_precision"] if label_files is not None else [])
    if filtered:
        fields += ["filtered_sum", "filtered_max"]
        fields += ["filtered_dice", "filtered_best_dice", "filtered_best_dice_threshold", "filtered_average_precision"] if label_files is not None else []
    if min_component is not None:
        fields += ["components", "components_kept", "voxels_kept", "largest_component"]
        fields += ["dice_cleaned", "lesions", "lesions_detected", "lesion_recall", "lesion_precision", "lesion_f1"] if label_files is not None else []
    fields += ["members"] if specs is not None else []
    with open(os.path.join(cfg["outputs_directory"], f"anomaly_scores_rank{rank}.csv"), "w", newline="") as f:
        wr = csv.DictWriter(f, fieldnames=fields)
        wr.writeheader()
        wr.writerows(rows)
    log(rank, f"anomaly done: {len(order)} subjects -> {cfg['outputs_directory']}")


def run(argv):
    from synthanatomy_amd.runtime.ddp import init_distributed
    cfg = parse_flags(argv, DEFAULTS)
    if cfg["mode"] not in MODES:
        raise ValueError(f"VQVAE mode unknown. Was given {cfg['mode']} but choices are {MODES}.")
    _check_output_flags(cfg)
    _check_codebook_flags(cfg)
    if (cfg["mode"] == "anomaly" or cfg["anomaly_ensemble"] is not None or cfg["anomaly_min_component"] is not None
            or cfg["anomaly_connectivity"] != DEFAULTS["anomaly_connectivity"] or _median_flags_given(cfg)):
        _check_anomaly_flags(cfg)
    cfg["perceptual_state"] = _check_perceptual_flags(cfg) if cfg["mode"] == "training" else None
    rank, local, world = init_distributed()
    cfg.update(rank=rank, local_rank=local, world_size=world)
    torch.manual_seed(cfg["seed"])
    np.random.seed(cfg["seed"])
    if cfg.get("deterministic"):
        # upstream: torch.backends.cudnn.deterministic (src/utils/general.py:336-338).  Here: fixed-order reductions instead of fp32 atomics (quantizer
        # statistics, bias gradients, BatchNorm sums) and the unfused first / last layer routes -- bit-identical runs (tests/test_deterministic_gpu.py)
        from synthanatomy_amd import debug
        debug.set_deterministic(True)
        log(rank, "--deterministic: fixed-order reductions (csrc/deterministic.hip); slower than the default path")
    create_folder_structure(cfg)
    dev = torch.device("cuda", local)
    {"training": training, "anomaly": anomaly}.get(cfg["mode"], inference)(cfg, rank, local, world, dev)


if __name__ == "__main__":
    run(sys.argv[1:])
