#!/usr/bin/env python3
"""Generate ``losses_fourier.npz`` by importing the REFERENCE's ``SpectralLoss``, ``HartleyLoss`` and ``WaveGANLoss`` (build container only; the
reference tree is absent on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_goldens_fourier.py

* ``src.losses.vqvae.vqvae.SpectralLoss`` (vqvae.py:188-323), ``HartleyLoss`` (:326-519) with ``prioritise_high_frequency`` True and False, and
  ``WaveGANLoss`` (:641-771), all ``dimensions=3`` with the default ``fft_kwargs`` and the pixel term: loss value, every tensor-valued summary and
  d loss / d reconstruction, under ``case/<loss>/<shape>/``, for three inputs under ``input/<shape>/``: ``even_w`` [2, 1, 5, 6, 8] (even W, odd D),
  ``odd_w`` [1, 2, 4, 6, 7] (odd W, two channels) and ``background`` [2, 1, 8, 8, 8] (a zero block in both volumes, as in a cropped MRI).
* The classes run in **float64**: their ``.float()`` casts are made to keep float64 while they run, so the fixture is exact to ~1e-15 and
  ``tests/fourier_ref.py`` can be held to 1e-10.  The inputs themselves are float32 values (what the GPU path receives).

Import recipe as in make_goldens_losses.py: ``src.handlers.general`` (needs ignite / MONAI) is replaced by its ``TBSummaryTypes`` enum, used only as
a dictionary key, and ``lpips.LPIPS``, which none of these classes constructs, by a placeholder.  Nothing from the reference is copied: the fixture
holds tensors only.
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

SHAPES = {"even_w": (2, 1, 5, 6, 8), "odd_w": (1, 2, 4, 6, 7), "background": (2, 1, 8, 8, 8)}
LOSSES = ("spectral", "hartley", "hartley_flat", "wavegan")


def _placeholders():
    handlers = types.ModuleType("src.handlers.general")

    class TBSummaryTypes(enum.Enum):   # only ever used as a dict key
        SCALAR = "scalar"

    handlers.TBSummaryTypes = TBSummaryTypes
    sys.modules["src.handlers.general"] = handlers
    lp = types.ModuleType("lpips")

    class LPIPS:  # placeholder, never constructed by these classes
        pass

    lp.LPIPS = LPIPS
    sys.modules["lpips"] = lp


@contextlib.contextmanager
def _float_keeps_float64():
    orig = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self if self.dtype == torch.float64 else orig(self, *a, **k)
    try:
        yield
    finally:
        torch.Tensor.float = orig


def _inputs(name, shape, g):
    y = torch.rand(shape, generator=g)
    pred = y + 0.1 * torch.randn(shape, generator=g)
    if name == "background":
        y[:, :, :3, :, :5] = 0
        pred[:, :, :3, :, :5] = 0.01 * torch.randn(shape, generator=g)[:, :, :3, :, :5]
    return y, pred, torch.tensor([0.0123, 0.0456])


def main():
    assert os.path.isdir(REF), "reference tree not present: goldens can only be regenerated in the build container"
    sys.path.insert(0, REF)
    _placeholders()
    from src.losses.vqvae.vqvae import HartleyLoss, SpectralLoss, WaveGANLoss

    make = {"spectral": lambda: SpectralLoss(dimensions=3), "hartley": lambda: HartleyLoss(dimensions=3),
            "hartley_flat": lambda: HartleyLoss(dimensions=3, prioritise_high_frequency=False), "wavegan": lambda: WaveGANLoss(dimensions=3)}
    out = {}
    g = torch.Generator().manual_seed(71)
    for sname, shape in SHAPES.items():
        y, pred, q = _inputs(sname, shape, g)
        out[f"input/{sname}/y"], out[f"input/{sname}/pred"], out[f"input/{sname}/qloss"] = y.numpy(), pred.numpy(), q.numpy()
        for lname in LOSSES:
            fn = make[lname]()
            p = pred.double().requires_grad_(True)
            with _float_keeps_float64():
                loss = fn({"reconstruction": [p], "quantization_losses": [q[0].double(), q[1].double()]}, y.double())
            loss.backward()
            c = f"case/{lname}/{sname}/"
            out[c + "loss"], out[c + "dpred"] = loss.detach().numpy(), p.grad.numpy()
            summ = fn.get_summaries()[list(fn.get_summaries())[0]]
            for k, v in summ.items():
                if torch.is_tensor(v) and "Commitment" not in k:
                    out[c + k] = v.detach().numpy()
    np.savez_compressed(os.path.join(HERE, "losses_fourier.npz"), **out)
    print("losses_fourier ok:", {k: float(v) for k, v in out.items() if k.endswith("/loss")})


if __name__ == "__main__":
    main()
