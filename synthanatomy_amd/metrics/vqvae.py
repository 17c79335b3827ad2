"""The VQ-VAE evaluator's metrics (reference ``src/metrics/vqvae.py``): ``MultiScaleSSIM`` (the key metric), ``MAE`` and ``MSE``, with ignite's
``reset`` / ``update((y_pred, y))`` / ``compute`` protocol and its ``sync_all_reduce`` of ``(_accumulator, _count)`` over an initialised process group.
MS-SSIM is ``sa_ms_ssim`` (csrc/metrics.hip); MAE and MSE are the L1 / L2 sums of ``sa_baur_loss`` with ``gdl_factor = 0`` (csrc/losses.hip, one
stencil-free pass)."""
from __future__ import annotations

from typing import Sequence

import torch

from .. import _ffi
from . import ms_ssim


class NotComputableError(RuntimeError):
    """ignite.exceptions.NotComputableError: ``compute()`` before any example."""


def abs_sq_sums(y_pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """[sum |p - y|, sum (p - y)^2] (fp32 device tensor, summed in fp64 in a fixed order) by ``sa_baur_loss`` with gdl_factor = 0 and no gradient."""
    _ffi.require_gpu()
    a = y_pred.float().contiguous()
    b = y.float().contiguous().to(a.device)
    if a.dim() != 5 or min(a.shape[2:]) < 3:
        raise ValueError(f"MAE / MSE take [B, C, D, H, W] volumes with sides >= 3, got {tuple(a.shape)}")
    B, C, D, H, W = a.shape
    lib = _ffi.lib()
    nbytes = lib.sa_baur_loss_workspace_bytes(B * C, D, H, W)
    _ffi.check(nbytes if nbytes < 0 else 0, "sa_baur_loss_workspace_bytes")
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=a.device)
    sums = torch.empty(3, dtype=torch.float32, device=a.device)
    _ffi.check(lib.sa_baur_loss(_ffi.ptr(a), _ffi.ptr(b), B * C, D, H, W, 0.0, 1, 1.0, _ffi.ptr(sums), None, _ffi.ptr(ws), _ffi.stream()),
               "sa_baur_loss")
    return sums[:2]


def _sync_all_reduce(acc: float, count: int):
    """ignite's ``sync_all_reduce("_accumulator", "_count")``: summed over ranks when a process group of more than one rank is initialised."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() < 2:
        return acc, count
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    t = torch.tensor([float(acc), float(count)], dtype=torch.float64, device=dev)
    dist.all_reduce(t)
    return float(t[0]), int(round(float(t[1])))


class _Metric:
    _name = ""

    def __init__(self, output_transform=lambda x: x):
        self._output_transform = output_transform
        self._accumulator = None
        self._count = None
        self.reset()

    def reset(self):
        self._accumulator = 0
        self._count = 0

    def _value(self, y_pred: torch.Tensor, y: torch.Tensor) -> float:
        raise NotImplementedError

    def update(self, output: Sequence[torch.Tensor]):
        y_pred, y = output
        y = y.float()
        y_pred = y_pred.float()
        if y.shape != y_pred.shape:
            raise ValueError("y_pred and y should have same shapes.")
        self._accumulator += self._value(y_pred, y)
        self._count += y.shape[0]

    def compute(self):
        acc, count = _sync_all_reduce(self._accumulator, self._count)
        if count == 0:
            raise NotComputableError(f"{self._name} must have at least one example before it can be computed.")
        return acc / count


class MultiScaleSSIM(_Metric):
    """Sum of the per-element MS-SSIM values over the examples seen, divided by their number.  Defaults: data_range 1, win_size 11,
    win_sigma 1.5, size_average False, weights None, K (0.01, 0.03), updated from ``ms_ssim_kwargs``."""
    _name = "MultiScaleSSIM"

    def __init__(self, output_transform=lambda x: x, ms_ssim_kwargs=None):
        self._ms_ssim_kwargs = {"data_range": 1, "win_size": 11, "win_sigma": 1.5, "size_average": False, "weights": None, "K": (0.01, 0.03)}
        if ms_ssim_kwargs:
            self._ms_ssim_kwargs.update(ms_ssim_kwargs)
        super().__init__(output_transform=output_transform)

    def _value(self, y_pred, y):
        return torch.sum(ms_ssim(X=y, Y=y_pred, **self._ms_ssim_kwargs)).item()


class MAE(_Metric):
    """``F.l1_loss(y_pred, y, "mean") * batch`` per update."""
    _name = "MAE"

    def _value(self, y_pred, y):
        return (abs_sq_sums(y_pred, y)[0].double() / y.numel()).item() * y.shape[0]


class MSE(_Metric):
    """``F.mse_loss(y_pred, y, "mean") * batch`` per update."""
    _name = "MSE"

    def _value(self, y_pred, y):
        return (abs_sq_sums(y_pred, y)[1].double() / y.numel()).item() * y.shape[0]
