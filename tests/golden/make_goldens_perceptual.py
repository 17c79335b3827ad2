#!/usr/bin/env python3
"""Generate ``losses_perceptual.npz`` by importing the REFERENCE's ``PerceptualLoss``, ``JukeboxPerceptualLoss`` and ``HartleyPerceptualLoss``
(build container only; the reference tree is absent on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_goldens_perceptual.py

* ``src.losses.vqvae.vqvae.PerceptualLoss`` (vqvae.py:774-1000), ``JukeboxPerceptualLoss`` (:1003-1285) and ``HartleyPerceptualLoss`` (:1288-1645),
  all ``dimensions=3`` with their defaults and ``drop_ratio=0`` (so the device ``randperm`` cannot matter): loss value, every tensor-valued summary and
  d loss / d reconstruction under ``case/<loss>/<shape>/``, for two inputs under ``input/<shape>/``: ``small`` [1, 1, 31, 33, 35] and ``background``
  [2, 1, 31, 34, 37] with a zero block in both volumes.  To keep the fixture under the size limit for committed files the inputs lie on the grid
  k / 255 and are stored as uint8 (``volumes()`` turns them back), and the float64 gradient is stored at every 8th voxel of the flattened volume
  (``dpred_strided``): a wrapper defect -- a wrong view, mean or factor -- moves every voxel, so the sample loses nothing the fixture is for.
* Import recipe as in make_goldens_fourier.py, but the ``lpips.LPIPS`` placeholder is the restatement of tests/lpips_ref.py with the seeded weights
  of ``seed`` (stored; the weights are NOT stored -- the tests re-draw them).  The fixture therefore pins the WRAPPER -- the views, the means, the
  factors, the spectral and pixel terms, the summary keys -- while the inner LPIPS arithmetic stays unpinned.
* The classes run in float64 (their ``.float()`` casts keep float64 while they run).  Nothing from the reference is copied: tensors only.
"""
import contextlib
import enum
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lpips_ref  # noqa: E402

SEED = 5
SHAPES = {"small": (1, 1, 31, 33, 35), "background": (2, 1, 31, 34, 37)}
LOSSES = ("perceptual", "jukebox_perceptual", "hartley_perceptual")


def _placeholders():
    handlers = types.ModuleType("src.handlers.general")

    class TBSummaryTypes(enum.Enum):   # only ever used as a dict key
        SCALAR = "scalar"

    handlers.TBSummaryTypes = TBSummaryTypes
    sys.modules["src.handlers.general"] = handlers
    lp = types.ModuleType("lpips")
    lpips_ref.LPIPS.seed = SEED
    lp.LPIPS = lpips_ref.LPIPS
    sys.modules["lpips"] = lp


@contextlib.contextmanager
def _float_keeps_float64():
    orig = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self if self.dtype == torch.float64 else orig(self, *a, **k)
    try:
        yield
    finally:
        torch.Tensor.float = orig


GRAD_STRIDE = 8     # d loss / d reconstruction is stored at every 8th voxel of the flattened volume (W is odd in both inputs: every column is visited)


def _inputs(name, shape, g):
    """volumes on the grid k / 255 (stored as uint8: the fixture stays small)"""
    y = torch.randint(0, 256, shape, generator=g)
    pred = (y + torch.round(25 * torch.randn(shape, generator=g)).long()).clamp(0, 255)
    if name == "background":
        y[:, :, :12, :, :15] = 0
        pred[:, :, :12, :, :15] = 0
    return y.to(torch.uint8), pred.to(torch.uint8), torch.tensor([0.0123])


def volumes(u8):
    return torch.as_tensor(u8).float() / 255


def main():
    assert os.path.isdir(REF), "reference tree not present: goldens can only be regenerated in the build container"
    sys.path.insert(0, REF)
    _placeholders()
    from src.losses.vqvae.vqvae import HartleyPerceptualLoss, JukeboxPerceptualLoss, PerceptualLoss

    make = {"perceptual": PerceptualLoss, "jukebox_perceptual": JukeboxPerceptualLoss, "hartley_perceptual": HartleyPerceptualLoss}
    out = {"seed": np.int64(SEED)}
    g = torch.Generator().manual_seed(83)
    for sname, shape in SHAPES.items():
        y8, pred8, q = _inputs(sname, shape, g)
        out[f"input/{sname}/y_u8"], out[f"input/{sname}/pred_u8"], out[f"input/{sname}/qloss"] = y8.numpy(), pred8.numpy(), q.numpy()
        y, pred = volumes(y8), volumes(pred8)
        for lname in LOSSES:
            fn = make[lname](dimensions=3, drop_ratio=0.0)
            p = pred.double().requires_grad_(True)
            with _float_keeps_float64():
                loss = fn({"reconstruction": [p], "quantization_losses": [q[0].double()]}, y.double())
            loss.backward()
            c = f"case/{lname}/{sname}/"
            out[c + "loss"], out[c + "dpred_strided"] = loss.detach().numpy(), p.grad.reshape(-1)[::GRAD_STRIDE].numpy()
            summ = fn.get_summaries()[list(fn.get_summaries())[0]]
            for k, v in summ.items():
                if torch.is_tensor(v) and "Commitment" not in k:
                    out[c + k] = v.detach().numpy()
    np.savez_compressed(os.path.join(HERE, "losses_perceptual.npz"), **out)
    print("losses_perceptual ok:", {k: float(v) for k, v in out.items() if k.endswith("/loss")})


if __name__ == "__main__":
    main()
