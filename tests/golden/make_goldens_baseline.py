#!/usr/bin/env python3
"""Generate ``losses_baseline.npz`` by importing the REFERENCE's ``BaselineLoss`` (build container only; the reference tree is absent on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_goldens_baseline.py

* ``src.losses.vqvae.vqvae.BaselineLoss`` (vqvae.py:1648-1780) with its defaults: loss value, every tensor-valued summary and d loss / d reconstruction
  under ``case/<shape>/``, for two inputs under ``input/<shape>/``: ``small`` [2, 1, 17, 21, 26] and ``background`` [2, 1, 19, 22, 25] with a zero
  block in both volumes.  Both have B n <= 512 = ``n_slices`` in every view, so upstream's ``torch.randperm(...)[:512]`` keeps every slice and the mean
  does not depend on the permutation: the reference is deterministic.  B = 2 so that the batch-axis transform of the frequency term (``fftn`` without
  ``dim``) is actually exercised.  As in make_goldens_perceptual.py the inputs lie on the grid k / 255 and are stored as uint8, and the float64 gradient
  is stored at every 8th voxel of the flattened volume (``dpred_strided``).
* Import recipe as in make_goldens_perceptual.py; the ``lpips.LPIPS`` placeholder is the restatement of tests/squeeze_ref.py with the seeded weights of
  ``seed`` (stored; the weights are NOT stored -- the tests re-draw them).  The fixture therefore pins the WRAPPER -- the three permutes, the means, the
  factors, the five-axis frequency term, the L1 term, the summary keys -- while the inner LPIPS-squeeze arithmetic stays UNPINNED.
* The class runs in float64 (its ``.float()`` casts keep float64 while it runs).  Nothing from the reference is copied: tensors only.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import squeeze_ref  # noqa: E402
from make_goldens_perceptual import GRAD_STRIDE, _float_keeps_float64, _placeholders, volumes  # noqa: E402

SEED = 7
SHAPES = {"small": (2, 1, 17, 21, 26), "background": (2, 1, 19, 22, 25)}


def _inputs(name, shape, g):
    """volumes on the grid k / 255 (stored as uint8: the fixture stays small)"""
    y = torch.randint(0, 256, shape, generator=g)
    pred = (y + torch.round(25 * torch.randn(shape, generator=g)).long()).clamp(0, 255)
    if name == "background":
        y[:, :, :8, :, :10] = 0
        pred[:, :, :8, :, :10] = 0
    return y.to(torch.uint8), pred.to(torch.uint8), torch.tensor([0.0123])


def main():
    assert os.path.isdir(REF), "reference tree not present: goldens can only be regenerated in the build container"
    sys.path.insert(0, REF)
    _placeholders()
    squeeze_ref.LPIPS.seed = SEED
    sys.modules["lpips"].LPIPS = squeeze_ref.LPIPS
    from src.losses.vqvae.vqvae import BaselineLoss

    out = {"seed": np.int64(SEED)}
    g = torch.Generator().manual_seed(91)
    for sname, shape in SHAPES.items():
        y8, pred8, q = _inputs(sname, shape, g)
        out[f"input/{sname}/y_u8"], out[f"input/{sname}/pred_u8"], out[f"input/{sname}/qloss"] = y8.numpy(), pred8.numpy(), q.numpy()
        y, pred = volumes(y8), volumes(pred8)
        fn = BaselineLoss()
        assert all(shape[0] * n <= fn.n_slices for n in shape[2:])
        p = pred.double().requires_grad_(True)
        with _float_keeps_float64():
            loss = fn({"reconstruction": [p], "quantization_losses": [q[0].double()]}, y.double())
        loss.backward()
        c = f"case/{sname}/"
        out[c + "loss"], out[c + "dpred_strided"] = loss.detach().numpy(), p.grad.reshape(-1)[::GRAD_STRIDE].numpy()
        summ = fn.get_summaries()[list(fn.get_summaries())[0]]
        for k, v in summ.items():
            if torch.is_tensor(v) and "Commitment" not in k:
                out[c + k] = v.detach().numpy()
    np.savez_compressed(os.path.join(HERE, "losses_baseline.npz"), **out)
    print("losses_baseline ok:", {k: float(v) for k, v in out.items() if k.endswith("/loss")})


if __name__ == "__main__":
    main()
