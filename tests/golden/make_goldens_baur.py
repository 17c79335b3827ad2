#!/usr/bin/env python3
"""Generate ``losses_baur.npz`` by importing the REFERENCE's ``BaurLoss`` and its factor schedule (build container only; the reference tree is
absent on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_goldens_baur.py

* ``src.losses.vqvae.vqvae.BaurLoss`` (vqvae.py:74-186): loss value, the three reconstruction summaries and d loss / d reconstruction for
  ``case/<name>/...``, whose inputs are under ``input/<case/<name>/input>/``: random volumes at gdl_factor 0.0 and 1.7, reduction "mean" and
  "sum", two quantization losses; a tie-heavy case on a 1/4 grid (p == y, gp == 0 and |gy| == |gp| all occur); a two-channel case with the
  smallest D (3).
* ``ParamSchedulerHandler._linear`` (src/handlers/general.py:92-118) at a table of (initial_value, step_constant, step_max_value, max_value,
  current_step) rows: ``schedule/args`` [R, 5] and ``schedule/values`` [R].

Import recipe as in make_goldens_losses.py: ``src.handlers.general`` imports ignite, MONAI and tensorboard (absent here) only for names used in
annotations and handler bodies never run here, and ``vqvae.py`` imports ``lpips.LPIPS`` which ``BaurLoss`` never constructs -> ``sys.modules`` is
pre-seeded with placeholders for exactly those names, and the reference's own ``general.py`` is then imported.  Nothing from the reference is
copied: the fixture holds tensors only.
"""
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


def _placeholders():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    class _Placeholder:  # only ever named in annotations / bodies that are not run
        pass

    mod("ignite")
    mod("ignite.engine", Engine=_Placeholder, Events=_Placeholder)
    mod("monai")
    mod("monai.engines", Trainer=_Placeholder)
    mod("monai.data")
    mod("monai.data.utils", create_file_basename=lambda *a, **k: None)
    if "torch.utils.tensorboard" not in sys.modules:
        try:
            import torch.utils.tensorboard  # noqa: F401
        except ImportError:
            mod("torch.utils.tensorboard", SummaryWriter=_Placeholder)
    mod("lpips", LPIPS=_Placeholder)


SCHEDULE = [(0, 25, 50, 5, s) for s in (0, 1, 24, 25, 26, 49, 50, 51, 100)] + \
           [(0.5, 1, 2, 3, s) for s in (0, 1, 2, 3, 4)] + \
           [(1.0, 3, 10, 4.0, s) for s in (0, 2, 3, 5, 10, 11)] + \
           [(0.2, 0, 4, 1.0, s) for s in (0, 1, 4, 5)]


def main():
    assert os.path.isdir(REF), "reference tree not present: goldens can only be regenerated in the build container"
    sys.path.insert(0, REF)
    _placeholders()
    from src.handlers.general import ParamSchedulerHandler
    from src.losses.vqvae.vqvae import BaurLoss

    out = {}
    g = torch.Generator().manual_seed(53)
    y0 = torch.rand(2, 1, 7, 9, 11, generator=g)
    p0 = y0 + 0.1 * torch.randn(2, 1, 7, 9, 11, generator=g)
    q0 = torch.tensor([0.0123, 0.0456])
    cases = {}
    for factor in (0.0, 1.7):
        for red in ("mean", "sum"):
            cases[f"random_f{factor}_{red}"] = ("random", y0, p0, q0, factor, red)
    y1 = torch.randint(0, 5, (2, 1, 6, 7, 9), generator=g).float() / 4
    p1 = torch.where(torch.rand(2, 1, 6, 7, 9, generator=g) < 0.4, y1, torch.randint(0, 5, (2, 1, 6, 7, 9), generator=g).float() / 4)
    cases["ties"] = ("ties", y1, p1, torch.tensor([0.25, 0.5]), 1.3, "mean")
    y2 = torch.rand(1, 2, 3, 5, 6, generator=g)
    p2 = y2 + 0.2 * torch.randn(1, 2, 3, 5, 6, generator=g)
    cases["small_d"] = ("small_d", y2, p2, torch.tensor([0.01, 0.02]), 0.9, "mean")
    for name, (inp, y, p, q, factor, red) in cases.items():
        pred = p.clone().requires_grad_(True)
        fn = BaurLoss(reduction=red)
        fn.set_gdl_factor(factor)
        loss = fn({"reconstruction": [pred], "quantization_losses": [q[0], q[1]]}, y)
        loss.backward()
        summ = fn.get_summaries()[list(fn.get_summaries())[0]]
        c = f"case/{name}/"
        out[f"input/{inp}/y"], out[f"input/{inp}/pred"], out[f"input/{inp}/qloss"] = y.numpy(), p.numpy(), q.numpy()   # (shared by the random cases)
        out[c + "input"] = np.array(inp)
        out[c + "factor"], out[c + "reduction_sum"] = np.float32(factor), np.int32(red == "sum")
        out[c + "loss"], out[c + "dpred"] = loss.detach().numpy(), pred.grad.numpy()
        for key in ("Loss-MAE-Reconstruction", "Loss-MSE-Reconstruction", "Loss-GDL-Reconstruction"):
            out[c + key] = torch.as_tensor(summ[key]).detach().numpy()
    out["schedule/args"] = np.array(SCHEDULE, dtype=np.float64)
    out["schedule/values"] = np.array([ParamSchedulerHandler._linear(*r) for r in SCHEDULE], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "losses_baur.npz"), **out)
    print("losses_baur ok:", {k: float(v) for k, v in out.items() if v.ndim == 0 and k.endswith("/loss")})
    print("schedule:", list(zip(SCHEDULE, out["schedule/values"].tolist())))


if __name__ == "__main__":
    main()
