"""Network factory keyed on ``config["network"]`` -- mirror of reference src/networks/vqvae/configure.py:14-39.

The EMA-decay warm-up of the reference (``add_vqvae_network_handlers``, configure.py:42-86: a ``ParamSchedulerHandler`` on ``set_ema_decay`` at every finished
epoch) is :func:`decay_schedule` here, applied by ``run_vqvae.py``'s loop.  Upstream subtracts from the ``decay`` TUPLE at :47 and hands the tuple to
``_linear`` at :75, so neither kind can run there; the rule below is restated from that code read on ``decay[0]``, which is what
the docstring at the reference's run_vqvae.py:802-804 describes -- unpinned: there is no upstream run to compare with.
"""
from __future__ import annotations

from enum import Enum
from math import ceil

import torch

from .baseline import BaselineVQVAE
from .vqvae import VQVAEBase


class VQVAENetworks(Enum):
    BASELINE_VQVAE = "baseline_vqvae"


class DecayWarmups(Enum):
    STEP = "step"
    LINEAR = "linear"


def get_max_decay_epochs(config: dict) -> int:
    """``--max_decay_epochs``, ``"auto"`` resolved by the reference's rule of thumb (src/utils/general.py:51-72): the EMA sees 200 epochs of 437 iterations of
    32 samples before the decay reaches 0.99."""
    m = config["max_decay_epochs"]
    if m == "auto":
        return ceil(200 * 437 * 32 / (config["epoch_length"] * config["batch_size"]))
    return m


def check_decay_warmup(config: dict) -> None:
    """``--decay_warmup`` / ``--max_decay_epochs`` act or refuse (host only)."""
    kinds = [None] + [w.value for w in DecayWarmups]
    if config["decay_warmup"] not in kinds:
        raise ValueError(f"--decay_warmup={config['decay_warmup']}: choices are step, linear and None")
    m = config["max_decay_epochs"]
    if m != "auto" and (isinstance(m, bool) or not isinstance(m, int) or m < 1):
        raise ValueError(f"--max_decay_epochs={m}: an int >= 1 or auto is needed")


def decay_schedule(config: dict, finished_epochs: int) -> float:
    """The quantizer's EMA decay after ``finished_epochs`` epochs (ignite's ``state.epoch`` at EPOCH_COMPLETED), starting from ``decay[0]``:
    ``step``: four stairs at ``linspace(0, max_decay_epochs, 5)[1:]``, reached when ``finished_epochs + 1`` gets there, each a quarter of ``0.99 - decay``
    (configure.py:46-59); ``linear``: ``ParamSchedulerHandler._linear`` (src/handlers/general.py:92-120) with ``step_constant=0``, ``max_value=0.99``,
    ``step_max_value=max_decay_epochs``; None: the constant ``decay[0]``."""
    base, kind, s = config["decay"][0], config["decay_warmup"], finished_epochs
    if kind is None:
        return base
    top = get_max_decay_epochs(config)
    if kind == DecayWarmups.STEP.value:
        delta_step = (0.99 - base) / 4
        stairs = [top * i / 4 for i in (1, 2, 3, 4)]
        return base + sum(1 for t in stairs if s + 1 >= t) * delta_step
    if kind == DecayWarmups.LINEAR.value:
        delta = (0.99 - base) if s > top else (0.99 - base) * (s / top)
        return base + delta
    raise ValueError(f"--decay_warmup={kind}: choices are step, linear and None")


def get_vqvae_network(config: dict) -> VQVAEBase:
    if config["network"] == VQVAENetworks.BASELINE_VQVAE.value:
        return BaselineVQVAE(
            n_levels=config["no_levels"],
            downsample_parameters=config["downsample_parameters"],
            upsample_parameters=config["upsample_parameters"],
            n_embed=config["num_embeddings"][0],
            embed_dim=config["embedding_dim"][0],
            commitment_cost=config["commitment_cost"][0],
            n_channels=config["no_channels"],
            n_res_channels=config["no_channels"],
            n_res_layers=config["no_res_layers"],
            p_dropout=config["dropout"],
            vq_decay=config["decay"][0],
            use_subpixel_conv=config["use_subpixel_conv"],
            # MI355X-only knob (not in the reference): bf16 MFMA throughput mode or exact-fp32 MFMA parity mode
            compute_dtype=config.get("compute_dtype", torch.bfloat16),
        )
    raise ValueError(f"VQVAE unknown. Was given {config['network']} but choices are {[v.value for v in VQVAENetworks]}.")
