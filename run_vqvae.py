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
Inputs: ``.npy`` or NIfTI-1 volumes -- any of dir / glob / csv listing -- or ``synthetic:<n>`` (synthanatomy_amd/utils/volumes.py).
Multi-GPU: launch with torchrun; one process per GPU, RCCL.

MI355X-only features (all off by default) and where each is documented:
``--augmentation``, ``--patch_size``, ``--no_augmented_extractions``: DESIGN 7.5, synthanatomy_amd/utils/vqvae.py (``draw_augmentation``, ``hip_augment``).
``--output_ext`` / ``--output_dtype`` (NIfTI-1 outputs): DESIGN 7.8, INTEGRATION.md, synthanatomy_amd/utils/volumes.py (``VolumeWriter``).
``--codebook_restart_patience`` / ``--codebook_restart_max``, ``--decay_warmup`` / ``--max_decay_epochs``: DESIGN 7.14, ``_check_codebook_flags`` below.
``--mode=anomaly``, ``--anomaly_ensemble`` (7.15), ``--anomaly_min_component`` / ``--anomaly_connectivity`` (7.17), ``--anomaly_median`` /
``--anomaly_mask=scan|<dir|glob>`` / ``--anomaly_mask_threshold`` / ``--anomaly_mask_erosion`` (7.18: ``_anomaly_map_filtered``, ``filtered_sum`` ...): engines/anomaly.py.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from synthanatomy_amd.engines.anomaly import (ANOMALY_FLAGS, _anomaly_sigma, _check_anomaly_flags, _ensemble_specs, anomaly,  # noqa: E402,F401
                                              anomaly_only_flags_given, find_ensemble_outputs, find_healing_outputs, match_labels)
from synthanatomy_amd.utils.general import (REQUIRED, check_for_checkpoints, create_folder_structure, list_inputs, load_checkpoint,  # noqa: E402
                                            load_network_state, log, parse_flags, save_checkpoint, save_npy, shard_for_rank)
from synthanatomy_amd.utils.volumes import (VolumeWriter, _augmented_batches, _augmented_name, _batches, _load_input, _load_volume,  # noqa: E402,F401
                                            _noise_seed, _output_path, _read_volume, _with_nifti_blocks)

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
    **ANOMALY_FLAGS,
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
    writer = VolumeWriter(cfg)      # NIfTI volumes leave through sa_volume_egress and writer threads; the codes stay uint16 .npy
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
                for names, x, headers in batches:
                    idx = net.index_quantize(x)[0]
                    rec = net.decode_samples([idx])
                    writer.batch()      # a NIfTI volume goes back into its source file's own axes; the writers work while the next batch runs
                    writer.save(names, {"reconstruction": rec}, None if n_aug > 0 else headers)      # (augmented batches carry their noise seed there)
                    for n, i_ in zip(names, idx.cpu().numpy()):
                        save_npy(i_, cfg["outputs_directory"], n, "quantization_0", np.uint16)
            else:  # decoding: .npy uint16 code grids -> reconstructions (prepare_decoding_batch: .long())
                files = list_inputs(cfg["training_subjects"], postfix="sample")[rank::world]
                group = max(min(int(cfg.get("num_workers") or 0), 8), 1)      # decoded volumes per batch of the writer: one per writer thread
                for k, f in enumerate(files):
                    codes = np.load(f).astype(np.int64)
                    if codes.min() < 0 or codes.max() >= net.n_embed:   # e.g. a sampled BOS id (== vocab_size): torch's embedding lookup raises upstream too
                        raise ValueError(f"{f}: code {int(codes.max())} is not a codebook entry (num_embeddings={net.n_embed})")
                    idx = torch.from_numpy(codes)[None].to(dev)
                    if k % group == 0:
                        writer.batch()
                    writer.save([f], {"sample": net.decode_samples([idx])})      # no source metadata (upstream has none here either): the identity geometry
    finally:
        writer.close()      # every writer is joined (and its exception re-raised here) before "done"
    log(rank, f"{cfg['mode']} done: {len(files)} inputs -> {cfg['outputs_directory']}")


def run(argv):
    from synthanatomy_amd.runtime.ddp import init_distributed
    cfg = parse_flags(argv, DEFAULTS)
    if cfg["mode"] not in MODES:
        raise ValueError(f"VQVAE mode unknown. Was given {cfg['mode']} but choices are {MODES}.")
    _check_output_flags(cfg)
    _check_codebook_flags(cfg)
    if cfg["mode"] == "anomaly" or anomaly_only_flags_given(cfg):
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
    stages = {"training": training, "anomaly": lambda *args: anomaly(*args, build_network)}      # (the stage's module does not import this script)
    stages.get(cfg["mode"], inference)(cfg, rank, local, world, dev)


if __name__ == "__main__":
    run(sys.argv[1:])
