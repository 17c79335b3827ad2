"""``MSELoss`` -- the minimal reconstruction loss of the reference (src/losses/vqvae/vqvae.py:14-71):
``mse(reconstruction[0], y) + sum(quantization_losses)``, with the same ``summaries`` side-channel.  The squared-error
reduction and its gradient are one fused HIP kernel (csrc/elementwise.hip: mse_kernel)."""
from __future__ import annotations

from typing import Dict, List

import torch

from .. import _ffi, debug


class _MSEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        _ffi.require_gpu()
        a = pred.float().contiguous()
        b = target.float().contiguous().to(a.device)
        n = a.numel()
        acc = torch.zeros(1, dtype=torch.float32, device=a.device)
        grad = torch.empty_like(a) if pred.requires_grad else None
        if debug.deterministic():   # --deterministic: the squared errors are summed in a fixed order (the loss value decides the key-metric checkpoint)
            ws = torch.empty(2048, dtype=torch.float32, device=a.device)
            _ffi.check(_ffi.lib().sa_mse_det(_ffi.ptr(a), _ffi.ptr(b), n, _ffi.ptr(acc), _ffi.ptr(grad), 1.0, _ffi.ptr(ws), _ffi.stream()), "sa_mse_det")
        else:
            _ffi.check(_ffi.lib().sa_mse(_ffi.ptr(a), _ffi.ptr(b), n, _ffi.ptr(acc), _ffi.ptr(grad), 1.0, _ffi.stream()), "sa_mse")
        ctx.grad = grad
        return (acc / n).reshape(())

    @staticmethod
    def backward(ctx, g):
        # re-entrant (the adaptive adversarial weight differentiates the reconstruction loss twice, engines/trainer.py): the stored
        # d mse / d pred is neither consumed nor scaled in place
        grad = ctx.grad
        return (grad * g if grad is not None else None), None


def hip_mse(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    return _MSEFn.apply(pred, target)


class MSELoss(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.summaries: Dict = {"scalar": {}}

    def forward(self, network_output: Dict[str, List[torch.Tensor]], y: torch.Tensor) -> torch.Tensor:
        rec = hip_mse(network_output["reconstruction"][0], y)
        q = network_output["quantization_losses"]
        loss = rec
        for ql in q:
            loss = loss + ql
        self.summaries["scalar"]["Loss-MSE-Reconstruction"] = rec.detach()
        for i, ql in enumerate(q):
            self.summaries["scalar"][f"Loss-MSE-Quantization_{i}"] = ql.detach()
        return loss

    def get_summaries(self):
        return self.summaries


class JukeboxLoss(torch.nn.Module):
    """``JukeboxLoss(dimensions=3)`` of the reference (src/losses/vqvae/vqvae.py:522-638, selected by ``--loss=jukebox``):
    ``mse(|fftn(pred)|, |fftn(y)|) * fft_factor + mse(pred, y) + sum(quantization_losses)`` with the orthonormal FFT over dims (1, 2, 3, 4).
    The transforms run in rocFFT through ``torch.fft.fftn`` on the device the volumes live on (a [8, 1, 160, 224, 160] batch is 367 MB of
    complex64 per transform; the amplitude / difference passes are a few HBM sweeps, ~1 % of a training step); the pixel term is the fused
    ``sa_mse`` kernel.  Same ``summaries`` keys and ``get/set_fft_factor`` as upstream."""

    def __init__(self, dimensions: int = 3, include_pixel_loss: bool = True, fft_kwargs: Dict = None, reduction: str = "mean"):
        super().__init__()
        self.dimensions, self.include_pixel_loss, self.reduction = dimensions, include_pixel_loss, reduction
        self.fft_factor: float = 1.0
        self.fft_kwargs = {"s": None, "dim": tuple(range(1, dimensions + 2)), "norm": "ortho"} if fft_kwargs is None else fft_kwargs
        self.summaries: Dict = {"scalar": {}}

    def _get_fft_amplitude(self, images: torch.Tensor) -> torch.Tensor:
        f = torch.fft.fftn(images, **self.fft_kwargs)
        return torch.sqrt(f.real ** 2 + f.imag ** 2)

    def forward(self, network_output: Dict[str, List[torch.Tensor]], y: torch.Tensor) -> torch.Tensor:
        y = y.float()
        y_pred = network_output["reconstruction"][0].float()
        with torch.no_grad():
            y_amp = self._get_fft_amplitude(y)
        loss = torch.nn.functional.mse_loss(self._get_fft_amplitude(y_pred), y_amp) * self.fft_factor
        self.summaries["scalar"]["Loss-Spectral-Reconstruction"] = loss.detach()
        self.summaries["scalar"]["Auxiliary-FFT_Factor"] = self.fft_factor
        if self.include_pixel_loss:
            l2 = hip_mse(y_pred, y)
            self.summaries["scalar"]["Loss-MSE-Reconstruction"] = l2.detach()
            loss = loss + l2
        for i, ql in enumerate(network_output["quantization_losses"]):
            ql = ql.float()
            self.summaries["scalar"][f"Loss-MSE-VQ{i}_Commitment_Cost"] = ql.detach()
            loss = loss + ql
        return loss

    def get_summaries(self):
        return self.summaries

    def get_fft_factor(self) -> float:
        return self.fft_factor

    def set_fft_factor(self, fft_factor: float) -> float:
        self.fft_factor = fft_factor
        return self.get_fft_factor()


class _BaurFn(torch.autograd.Function):
    """``l1 + l2 + gdl_factor * gdl`` and its gradient in one ``sa_baur_loss`` launch pair (csrc/losses.hip).  Returns the differentiable sum and the
    three terms as non-differentiable side outputs (the summaries)."""

    @staticmethod
    def forward(ctx, pred, target, gdl_factor, reduction_sum):
        _ffi.require_gpu()
        a = pred.contiguous()
        b = target.contiguous().to(a.device)
        B, C, D, H, W = a.shape
        lib = _ffi.lib()
        ws_bytes = lib.sa_baur_loss_workspace_bytes(B * C, D, H, W)
        _ffi.check(ws_bytes if ws_bytes < 0 else 0, "sa_baur_loss_workspace_bytes")
        ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=a.device)
        sums = torch.empty(3, dtype=torch.float32, device=a.device)
        grad = torch.empty_like(a) if pred.requires_grad else None
        _ffi.check(lib.sa_baur_loss(_ffi.ptr(a), _ffi.ptr(b), B * C, D, H, W, float(gdl_factor), int(reduction_sum), 1.0, _ffi.ptr(sums), _ffi.ptr(grad),
                                    _ffi.ptr(ws), _ffi.stream()), "sa_baur_loss")
        if reduction_sum:
            l1, l2, gdl = sums[0], sums[1], sums[2] * gdl_factor
        else:
            l1, l2, gdl = sums[0] / a.numel(), sums[1] / a.numel(), sums[2] / (B * C * (D - 2) * (H - 2) * (W - 2)) * gdl_factor
        rec = l1 + l2 + gdl
        ctx.grad = grad
        ctx.mark_non_differentiable(l1, l2, gdl)
        return rec, l1, l2, gdl

    @staticmethod
    def backward(ctx, g, *_):
        # re-entrant like _MSEFn: the stored d loss / d pred is neither consumed nor scaled in place
        grad = ctx.grad
        return (grad * g if grad is not None else None), None, None, None


class BaurLoss(torch.nn.Module):
    """``BaurLoss`` of the reference (src/losses/vqvae/vqvae.py:74-186, selected by ``--loss=baur``): ``l1(pred, y) + mse(pred, y) +
    gdl * gdl_factor + sum(quantization_losses)``, where ``gdl`` reduces ``| |y(i - e_a) - y(i)| - |pred(i - e_a) - pred(i)| |`` summed over the
    three axes on the interior voxels (the reference's ConstantPad3d shifts cropped by ``[1:-1]`` on D, H and W).  The three reductions and
    d loss / d pred are one fused HIP pass (``sa_baur_loss``, csrc/losses.hip).  ``gdl_factor`` starts at 0.0; ``run_vqvae.py`` schedules it once per
    epoch with :func:`gdl_factor_schedule`.  Same constructor, ``summaries`` keys and ``get/set_gdl_factor`` as upstream."""

    def __init__(self, size_average: bool = None, reduce: bool = None, reduction: str = "mean"):
        super().__init__()
        if reduction not in ("sum", "mean"):
            raise ValueError("Reduction must be either 'sum' or 'mean'")
        self.reduction = reduction
        self.gdl_factor: float = 0.0
        self.summaries: Dict = {"scalar": {}}

    def forward(self, network_output: Dict[str, List[torch.Tensor]], y: torch.Tensor) -> torch.Tensor:
        y = y.float()
        y_pred = network_output["reconstruction"][0].float()
        if y_pred.dim() != 5 or min(y_pred.shape[2:]) < 3:
            raise ValueError(f"BaurLoss needs [B, C, D, H, W] volumes with D, H, W >= 3 (the image-gradient term crops one voxel per side); "
                             f"got {tuple(y_pred.shape)}")
        if tuple(y.shape) != tuple(y_pred.shape):
            raise ValueError(f"BaurLoss: target shape {tuple(y.shape)} differs from the reconstruction's {tuple(y_pred.shape)}")
        loss, l1, l2, gdl = _BaurFn.apply(y_pred, y, float(self.gdl_factor), self.reduction == "sum")
        self.summaries["scalar"]["Loss-MAE-Reconstruction"] = l1.detach()
        self.summaries["scalar"]["Loss-MSE-Reconstruction"] = l2.detach()
        self.summaries["scalar"]["Loss-GDL-Reconstruction"] = gdl.detach()
        self.summaries["scalar"]["Auxiliary-GDL_Factor"] = self.gdl_factor
        for idx, ql in enumerate(network_output["quantization_losses"]):
            ql = ql.float()
            self.summaries["scalar"][f"Loss-MSE-VQ{idx}_Commitment_Cost"] = ql.detach()
            loss = loss + ql
        return loss

    def get_summaries(self):
        return self.summaries

    def get_gdl_factor(self) -> float:
        return self.gdl_factor

    def set_gdl_factor(self, gdl_factor: float) -> float:
        self.gdl_factor = gdl_factor
        return self.get_gdl_factor()


def gdl_factor_schedule(config: dict, finished_epochs: int) -> float:
    """The ``gdl_factor`` of ``--loss=baur`` after ``finished_epochs`` epochs: ``ParamSchedulerHandler._linear`` (reference src/handlers/general.py:92-118)
    with the four ``--*_factor_*`` flags (src/losses/vqvae/configure.py:56-76), called at EPOCH_COMPLETED with ignite's ``state.epoch``.  Kept as
    upstream writes it, quirks included: before ``initial_factor_steps`` it returns ``2 * initial_factor_value`` (``delta = initial_value`` is added to
    ``initial_value``), and the ramp divides by ``max_factor_steps``, not by its length."""
    init, const = config["initial_factor_value"], config["initial_factor_steps"]
    steps, top = config["max_factor_steps"], config["max_factor_value"]
    s = finished_epochs
    if s < const:
        delta = init
    elif s > steps:
        delta = top - init
    else:
        delta = (top - init) * ((s - const) / steps)
    return init + delta


_FOURIER_KIND = {"spectral": 0, "hartley": 1, "wavegan": 2}   # include/synthanatomy_hip.h: SA_FOURIER_*
_FFT_DIMS = (1, 2, 3, 4)


class _FourierFn(torch.autograd.Function):
    """The spectral term of ``SpectralLoss`` / ``HartleyLoss`` / ``WaveGANLoss`` and its gradient: unnormalised rocFFT ``rfftn`` of both volumes over
    (C, D, H, W), one fused ``sa_fourier_loss`` pass over the two half spectra (csrc/spectral.hip) that writes the fp64 sums and, in place of the
    prediction's spectrum, the spectrum-domain gradient, then ``irfftn(norm="forward")`` of that gradient.  Returns the differentiable spectral term
    (factor applied) and the two unscaled summary terms as non-differentiable side outputs."""

    @staticmethod
    def forward(ctx, pred, target, kind, factor, prioritise_hf):
        _ffi.require_gpu()
        a = pred.contiguous()
        B, C, D, H, W = a.shape
        lib = _ffi.lib()
        ws_bytes = lib.sa_fourier_loss_workspace_bytes(B, C, D, H, W)
        _ffi.check(ws_bytes if ws_bytes < 0 else 0, "sa_fourier_loss_workspace_bytes")
        # (the kernel indexes bins as [B, C, D, H, W/2 + 1]; a multi-pass rocFFT transform leaves its output re-strided, k_W not innermost)
        xp = torch.fft.rfftn(a, dim=_FFT_DIMS, norm="backward").contiguous()
        xy = torch.fft.rfftn(target.contiguous().to(a.device), dim=_FFT_DIMS, norm="backward").contiguous()
        ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=a.device)
        sums = torch.empty(3, dtype=torch.float64, device=a.device)
        want = pred.requires_grad
        _ffi.check(lib.sa_fourier_loss(_FOURIER_KIND[kind], _ffi.ptr(xp), _ffi.ptr(xy), B, C, D, H, W, int(prioritise_hf), float(factor), _ffi.ptr(sums),
                                       _ffi.ptr(xp) if want else None, _ffi.ptr(ws), _ffi.stream()), "sa_fourier_loss")
        ctx.grad = torch.fft.irfftn(xp, s=(C, D, H, W), dim=_FFT_DIMS, norm="forward") if want else None
        n = a.numel()
        if kind == "spectral":
            t1, t2 = sums[0] * (0.5 / n), sums[1] * (0.5 / n)          # amplitude, phase
            spec = (t1 + t2) * factor
        elif kind == "hartley":
            spec = sums[0] * (0.5 / n) * factor
            t1, t2 = spec.clone(), torch.zeros_like(spec)               # (the reference's Hartley summary is the scaled term; distinct tensors, since
                                                                        # the side outputs are marked non-differentiable)
        else:
            t1, t2 = torch.sqrt(sums[0]) / torch.sqrt(sums[1]), sums[2] / n     # spectral convergence, log magnitude
            spec = (t1 + t2) * factor
        dt = torch.float64 if kind == "hartley" and prioritise_hf else torch.float32   # (the reference's Hartley weight is float64)
        spec, t1, t2 = spec.to(dt), t1.to(dt), t2.to(dt)
        ctx.mark_non_differentiable(t1, t2)
        return spec, t1, t2

    @staticmethod
    def backward(ctx, g, *_):
        # re-entrant like _MSEFn: the stored d loss / d pred is neither consumed nor scaled in place
        grad = ctx.grad
        return (grad * g.float() if grad is not None else None), None, None, None, None


class _FourierLoss(torch.nn.Module):
    _KIND = ""
    _FACTOR_ATTR, _FACTOR_KEY = "fft_factor", "Auxiliary-FFT_Factor"      # the factor's attribute and summary key, as upstream names them

    def __init__(self, dimensions: int, include_pixel_loss: bool = True, fft_kwargs: Dict = None, size_average: bool = None, reduce: bool = None,
                 reduction: str = "mean"):
        super().__init__()
        name = type(self).__name__
        if dimensions != 3:
            raise NotImplementedError(f"{name}: only dimensions=3 ([B, C, D, H, W] volumes) has a HIP path; got dimensions={dimensions}")
        default = {"s": None, "dim": tuple(range(1, dimensions + 2)), "norm": "ortho"}
        if fft_kwargs is not None and dict(fft_kwargs) != default:
            raise NotImplementedError(f"{name}: only the default fft_kwargs {default} have a HIP path; got {fft_kwargs}")
        if reduction not in ("mean", "sum"):
            raise NotImplementedError(f"{name}: reduction must be 'mean' or 'sum' (it applies to the pixel term); got {reduction!r}")
        self.dimensions, self.include_pixel_loss, self.reduction = dimensions, include_pixel_loss, reduction
        self.fft_kwargs = default
        self.summaries: Dict = {"scalar": {}}
        setattr(self, self._FACTOR_ATTR, 1.0)

    def _spectral_summaries(self, spec, t1, t2):
        raise NotImplementedError

    def _prioritise_hf(self) -> bool:
        return False

    def forward(self, network_output: Dict[str, List[torch.Tensor]], y: torch.Tensor) -> torch.Tensor:
        y = y.float()
        y_pred = network_output["reconstruction"][0].float()
        name = type(self).__name__
        if y_pred.dim() != 5 or min(y_pred.shape[2:]) < 2:
            raise ValueError(f"{name} needs [B, C, D, H, W] volumes with D, H, W >= 2; got {tuple(y_pred.shape)}")
        if tuple(y.shape) != tuple(y_pred.shape):
            raise ValueError(f"{name}: target shape {tuple(y.shape)} differs from the reconstruction's {tuple(y_pred.shape)}")
        factor = getattr(self, self._FACTOR_ATTR)
        loss, t1, t2 = _FourierFn.apply(y_pred, y, self._KIND, float(factor), self._prioritise_hf())
        self._spectral_summaries(loss.detach(), t1.detach(), t2.detach())
        self.summaries["scalar"][self._FACTOR_KEY] = factor
        if self.include_pixel_loss:
            l2 = hip_mse(y_pred, y)
            if self.reduction == "sum":
                l2 = l2 * y_pred.numel()
            self.summaries["scalar"]["Loss-MSE-Reconstruction"] = l2.detach()
            loss = loss + l2
        for idx, ql in enumerate(network_output["quantization_losses"]):
            ql = ql.float()
            self.summaries["scalar"][f"Loss-MSE-VQ{idx}_Commitment_Cost"] = ql.detach()
            loss = loss + ql
        return loss

    def get_summaries(self):
        return self.summaries


class SpectralLoss(_FourierLoss):
    """``SpectralLoss(dimensions=3)`` of the reference (src/losses/vqvae/vqvae.py:188-323, ``--loss=spectral``): ``fft_factor * (0.5 mse(|Y_pred|, |Y|)
    + mean 0.5 (1 - exp|angle Y_pred - angle Y|)^2) + mse(pred, y) + sum(quantization_losses)``, Y the ortho ``fftn`` over dims (1, 2, 3, 4).  The
    spectral term and its gradient are :class:`_FourierFn` (half spectra, one fused HIP pass).  Same constructor, ``summaries`` keys and
    ``get/set_fft_factor`` as upstream; a non-default ``fft_kwargs`` or ``dimensions`` raises ``NotImplementedError``."""
    _KIND = "spectral"

    def _spectral_summaries(self, spec, amp, phase):
        self.summaries["scalar"]["Loss-Amplitude-Reconstruction"] = amp
        self.summaries["scalar"]["Loss-Phase-Reconstruction"] = phase
        self.summaries["scalar"]["Loss-Spectral-Reconstruction"] = spec

    def get_fft_factor(self) -> float:
        return self.fft_factor

    def set_fft_factor(self, fft_factor: float) -> float:
        self.fft_factor = fft_factor
        return self.get_fft_factor()


class HartleyLoss(_FourierLoss):
    """``HartleyLoss(dimensions=3)`` of the reference (src/losses/vqvae/vqvae.py:326-519, ``--loss=hartley``): ``fht_factor * 0.5 mse(w H_pred, w H)
    + mse(pred, y) + sum(quantization_losses)``, H = Re - Im of the ortho ``fftn`` and w the reference's high-frequency weight (1 with
    ``prioritise_high_frequency=False``).  Because w is symmetric under k -> -k this is a weighted complex MSE, computed on half spectra by
    :class:`_FourierFn`.  As upstream, the loss is float64 when the weight applies (the reference builds it in float64).  Same constructor,
    ``summaries`` keys and ``get/set_fht_factor`` as upstream."""
    _KIND = "hartley"
    _FACTOR_ATTR, _FACTOR_KEY = "fht_factor", "Auxiliary-Hartley_Factor"

    def __init__(self, dimensions: int, include_pixel_loss: bool = True, fft_kwargs: Dict = None, prioritise_high_frequency: bool = True,
                 size_average: bool = None, reduce: bool = None, reduction: str = "mean"):
        super().__init__(dimensions, include_pixel_loss, fft_kwargs, size_average, reduce, reduction)
        self.prioritise_high_frequency = prioritise_high_frequency

    def _prioritise_hf(self) -> bool:
        return bool(self.prioritise_high_frequency)

    def _spectral_summaries(self, spec, *_):
        self.summaries["scalar"]["Loss-Hartley-Reconstruction"] = spec

    def get_fht_factor(self) -> float:
        return self.fht_factor

    def set_fht_factor(self, fht_factor: float) -> float:
        self.fht_factor = fht_factor
        return self.get_fht_factor()


class WaveGANLoss(_FourierLoss):
    """``WaveGANLoss(dimensions=3)`` of the reference (src/losses/vqvae/vqvae.py:641-771, ``--loss=wavegan``): ``fft_factor * (||A - A_pred||_F / ||A||_F
    + l1(log A, log A_pred)) + mse(pred, y) + sum(quantization_losses)``, A = |ortho fftn|.  The two norms are global, so the fused HIP step takes a
    second pass for the gradient, reading the finished sums on the device.  Same constructor, ``summaries`` keys and ``get/set_fft_factor`` as
    upstream."""
    _KIND = "wavegan"

    def _spectral_summaries(self, spec, l_sc, l_mag):
        self.summaries["scalar"]["Loss-Spectral_Convergence-Reconstruction"] = l_sc
        self.summaries["scalar"]["Loss-Log_Magnitude-Reconstruction"] = l_mag
        self.summaries["scalar"]["Loss-Spectral-Reconstruction"] = spec

    def get_fft_factor(self) -> float:
        return self.fft_factor

    def set_fft_factor(self, fft_factor: float) -> float:
        self.fft_factor = fft_factor
        return self.get_fft_factor()


def _lpips_network(name: str, net: str, weights: Dict, compute_dtype: torch.dtype):
    """(the frozen LPIPS network ``net`` over validated weights, its smallest slice side); weights of the other network's layout are refused by name"""
    from . import lpips, lpips_squeeze
    squeeze_file = lpips_squeeze.is_squeeze_layout(weights)
    if net == "squeeze":
        if not squeeze_file:
            raise ValueError(f"{name}: net='squeeze' needs perceptual_weights in the layout of lpips.LPIPS(net='squeeze').state_dict() (key "
                             f"'net.slice2.3.squeeze.weight' is missing): losses.lpips.load_weights(<file> | 'random:<seed>', net='squeeze')")
        return lpips_squeeze.LpipsSqueeze(weights, compute_dtype), lpips_squeeze.MIN_SIDE
    if squeeze_file:
        raise ValueError(f"{name}: perceptual_weights hold the LPIPS-squeeze layout ('net.slice2.3.squeeze.weight'); pass lpips_kwargs={{'net': 'squeeze'}} "
                         "or LPIPS-alex weights")
    return lpips.LpipsAlex(weights, compute_dtype), lpips.MIN_SIDE


_FAKE_3D_VIEW = {2: 0, 3: 1, 4: 2}      # fake_3d_axis entry -> view id of sa_lpips_unfold (the reference's permutes (0,2,1,3,4), (0,3,1,2,4), (0,4,1,2,3))


class _SliceLpipsLoss(torch.nn.Module):
    """What the losses with a 2.5D LPIPS term share: the step that keys the slice draw, the refusals every such loss makes of its volumes, the per-view
    draw and the commitment-cost tail.  Subclasses set ``seed``, ``step`` and ``summaries``."""

    def set_step(self, step: int) -> int:
        """the global training iteration: with the seed and the view it keys the slice draw, so a resumed run reproduces it"""
        self.step = int(step)
        return self.step

    def _check_volumes(self, y_pred: torch.Tensor, y: torch.Tensor):
        name = type(self).__name__
        if y_pred.dim() != 5:
            raise ValueError(f"{name} needs [B, 1, D, H, W] volumes; got {tuple(y_pred.shape)}")
        if tuple(y.shape) != tuple(y_pred.shape):
            raise ValueError(f"{name}: target shape {tuple(y.shape)} differs from the reconstruction's {tuple(y_pred.shape)}")
        if y_pred.shape[1] != 1:
            raise NotImplementedError(f"{name}: C = 1 only (the single channel broadcasts to LPIPS' three); got C={y_pred.shape[1]}")

    def _draw_ids(self, y_pred: torch.Tensor, views, n_keep) -> List[torch.Tensor]:
        """per view the kept slice ids (``n_keep(n)`` of its n = B * extent slices) on the prediction's device: small int32 uploads"""
        from . import lpips
        B, _, D, H, W = y_pred.shape
        return [torch.from_numpy(lpips.draw_slices(self.seed, self.step, v, B * (D, H, W)[v], n_keep(B * (D, H, W)[v]))).to(y_pred.device) for v in views]

    def _add_commitment(self, loss: torch.Tensor, network_output) -> torch.Tensor:
        for idx, ql in enumerate(network_output["quantization_losses"]):
            ql = ql.float()
            self.summaries["scalar"][f"Loss-MSE-VQ{idx}_Commitment_Cost"] = ql.detach()
            loss = loss + ql
        return loss

    def get_summaries(self):
        return self.summaries


class _PerceptualLoss(_SliceLpipsLoss):
    """What ``PerceptualLoss``, ``JukeboxPerceptualLoss`` and ``HartleyPerceptualLoss`` share: the 2.5D LPIPS term -- alex by default (losses/lpips.py,
    csrc/lpips.hip), squeeze with ``lpips_kwargs={"net": "squeeze"}`` (losses/lpips_squeeze.py; section 7.13) --, the pixel term and
    the commitment terms.  Beyond upstream's constructor arguments: ``perceptual_weights`` (a validated state dict in the layout of that network,
    losses.lpips.load_weights), ``compute_dtype`` (float32 = parity mode, bfloat16 = throughput mode) and ``seed`` (the slice
    draw is keyed on (seed, step, view); the training loop calls :meth:`set_step` with the global iteration)."""

    def __init__(self, dimensions: int, include_pixel_loss: bool = True, is_fake_3d: bool = True, drop_ratio: float = 0.0,
                 fake_3d_axis=(2, 3, 4), lpips_kwargs: Dict = None, lpips_normalize: bool = True, *, perceptual_weights: Dict = None,
                 compute_dtype: torch.dtype = torch.float32, seed: int = 0):
        super().__init__()
        from . import lpips
        name = type(self).__name__
        if dimensions != 3:
            raise NotImplementedError(f"{name}: only dimensions=3 ([B, 1, D, H, W] volumes, the 2.5D approach) has a HIP path; got dimensions={dimensions}")
        if not is_fake_3d:
            raise NotImplementedError(f"{name}: is_fake_3d=False (a true 3D perceptual loss) is not implemented, as upstream")
        net = "alex"
        if lpips_kwargs is not None:
            want = {k: v for k, v in lpips.DEFAULT_LPIPS_KWARGS.items() if k != "verbose"}
            net = dict(lpips_kwargs).get("net", "alex")
            if any(k not in want or (want[k] != v and not (k == "net" and v == "squeeze")) for k, v in dict(lpips_kwargs).items() if k != "verbose"):
                raise NotImplementedError(f"{name}: only the default lpips_kwargs (net='alex' or 'squeeze', version='0.1', lpips=True, spatial=False, "
                                          f"pnet_tune=False) have a HIP path; got lpips_kwargs={lpips_kwargs}")
        if isinstance(drop_ratio, bool) or not isinstance(drop_ratio, (int, float)) or not 0 <= drop_ratio < 1:
            raise ValueError(f"{name}: drop_ratio must lie in [0, 1); got drop_ratio={drop_ratio}")
        axes = tuple(fake_3d_axis)
        if not axes or any(a not in _FAKE_3D_VIEW for a in axes):
            raise ValueError(f"{name}: fake_3d_axis must name axes among (2, 3, 4); got fake_3d_axis={fake_3d_axis}")
        if perceptual_weights is None:
            raise ValueError(f"{name}: perceptual_weights is required (this build downloads nothing): losses.lpips.load_weights(<file> | 'random:<seed>')")
        self.dimensions, self.include_pixel_loss = dimensions, include_pixel_loss
        self.lpips_kwargs = dict(lpips.DEFAULT_LPIPS_KWARGS, net=net)
        self.fake_3D_views = [_FAKE_3D_VIEW[a] for a in (2, 3, 4) if a in axes]      # (upstream's order: by axis, whatever the tuple's order)
        self.keep_ratio = 1 - drop_ratio
        self.lpips_normalize = bool(lpips_normalize)
        self.perceptual_function, self._min_side = _lpips_network(name, net, perceptual_weights, compute_dtype)
        self.perceptual_factor = 0.001
        self.seed, self.step = int(seed), 0
        self.chunk_slices = None           # None: from the workspace cap (tests halve it)
        self.summaries: Dict = {"scalar": {}}

    def _n_keep(self, n_slices: int) -> int:
        return int(n_slices * self.keep_ratio)

    def _check(self, y_pred: torch.Tensor, y: torch.Tensor):
        name = type(self).__name__
        self._check_volumes(y_pred, y)
        B, _, D, H, W = y_pred.shape
        for v in self.fake_3D_views:
            n, sides = ((D, (H, W)), (H, (D, W)), (W, (D, H)))[v]
            if min(sides) < self._min_side:
                raise ValueError(f"{name}: view {v} has slices of {sides[0]} x {sides[1]}; every slice side must be >= {self._min_side} (the smallest for which "
                                 f"the network's last pool still has an output); got a volume of {D} x {H} x {W}")
            if self._n_keep(B * n) < 1:
                raise ValueError(f"{name}: drop_ratio={1 - self.keep_ratio:g} keeps 0 of the {B * n} slices of view {v}")

    def _perceptual(self, y_pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """the sum of the per-view terms (differentiable to y_pred), summaries written"""
        from . import lpips
        self._check(y_pred, y)          # every refusal comes before the first launch
        ids = self._draw_ids(y_pred, self.fake_3D_views, self._n_keep)
        total, *terms = lpips.PerceptualFn.apply(y_pred, y, self.perceptual_function, tuple(self.fake_3D_views), ids, float(self.perceptual_factor),
                                                 self.lpips_normalize, self.chunk_slices)
        for idx, t in enumerate(terms):
            self.summaries["scalar"][f"Loss-Perceptual_{idx}-Reconstruction"] = t.detach()
        self.summaries["scalar"]["Auxiliary-Perceptual_Factor"] = self.perceptual_factor
        return total

    def _tail(self, loss, y_pred, y, network_output):
        if self.include_pixel_loss:
            l2 = hip_mse(y_pred, y)
            self.summaries["scalar"]["Loss-MSE-Reconstruction"] = l2.detach()
            loss = loss + l2
        return self._add_commitment(loss, network_output)

    def _spectral(self, y_pred, y):
        return None

    def forward(self, network_output: Dict[str, List[torch.Tensor]], y: torch.Tensor) -> torch.Tensor:
        y = y.float()
        y_pred = network_output["reconstruction"][0].float()
        self._check(y_pred, y)
        spec = self._spectral(y_pred, y)
        p = self._perceptual(y_pred, y)
        return self._tail(p if spec is None else spec + p, y_pred, y, network_output)

    def get_perceptual_factor(self) -> float:
        return self.perceptual_factor

    def set_perceptual_factor(self, perceptual_factor: float) -> float:
        self.perceptual_factor = perceptual_factor
        return self.get_perceptual_factor()


class PerceptualLoss(_PerceptualLoss):
    """``PerceptualLoss(dimensions=3)`` of the reference (src/losses/vqvae/vqvae.py:774-1000, ``--loss=perceptual``): ``sum over the 2.5D views of
    perceptual_factor * mean LPIPS(y slices, pred slices) + mse(pred, y) + sum(quantization_losses)``.  Same constructor arguments, ``summaries`` keys
    and ``get/set_perceptual_factor`` as upstream."""


class JukeboxPerceptualLoss(_PerceptualLoss):
    """``JukeboxPerceptualLoss(dimensions=3)`` of the reference (src/losses/vqvae/vqvae.py:1003-1285, ``--loss=jukebox_perceptual``, the loss of the
    published training recipe): :class:`JukeboxLoss`' spectral term + the perceptual term + pixel and commitment terms."""

    def __init__(self, dimensions: int, include_pixel_loss: bool = True, is_fake_3d: bool = True, drop_ratio: float = 0.0, fake_3d_axis=(2, 3, 4),
                 lpips_kwargs: Dict = None, lpips_normalize: bool = True, fft_kwargs: Dict = None, **kw):
        super().__init__(dimensions, include_pixel_loss, is_fake_3d, drop_ratio, fake_3d_axis, lpips_kwargs, lpips_normalize, **kw)
        self._jukebox = JukeboxLoss(dimensions=dimensions, include_pixel_loss=False, fft_kwargs=fft_kwargs)
        self.fft_kwargs = self._jukebox.fft_kwargs

    @property
    def fft_factor(self) -> float:
        return self._jukebox.fft_factor

    def _spectral(self, y_pred, y):
        spec = self._jukebox({"reconstruction": [y_pred], "quantization_losses": []}, y)
        self.summaries["scalar"]["Loss-Spectral-Reconstruction"] = spec.detach()
        self.summaries["scalar"]["Auxiliary-FFT_Factor"] = self._jukebox.fft_factor
        return spec

    def get_fft_factor(self) -> float:
        return self._jukebox.get_fft_factor()

    def set_fft_factor(self, fft_factor: float) -> float:
        return self._jukebox.set_fft_factor(fft_factor)


class HartleyPerceptualLoss(_PerceptualLoss):
    """``HartleyPerceptualLoss(dimensions=3)`` of the reference (src/losses/vqvae/vqvae.py:1288-1645, ``--loss=hartley_perceptual``): :class:`HartleyLoss`'
    weighted Hartley term (:class:`_FourierFn`) + the perceptual term + pixel and commitment terms."""

    def __init__(self, dimensions: int, include_pixel_loss: bool = True, is_fake_3d: bool = True, drop_ratio: float = 0.0, fake_3d_axis=(2, 3, 4),
                 lpips_kwargs: Dict = None, lpips_normalize: bool = True, fft_kwargs: Dict = None, prioritise_high_frequency: bool = True, **kw):
        super().__init__(dimensions, include_pixel_loss, is_fake_3d, drop_ratio, fake_3d_axis, lpips_kwargs, lpips_normalize, **kw)
        self._hartley = HartleyLoss(dimensions, include_pixel_loss=False, fft_kwargs=fft_kwargs, prioritise_high_frequency=prioritise_high_frequency)
        self.fft_kwargs, self.prioritise_high_frequency = self._hartley.fft_kwargs, prioritise_high_frequency

    @property
    def fht_factor(self) -> float:
        return self._hartley.fht_factor

    def _spectral(self, y_pred, y):
        spec = self._hartley({"reconstruction": [y_pred], "quantization_losses": []}, y)
        self.summaries["scalar"]["Auxiliary-Hartley_Factor"] = self._hartley.fht_factor
        self.summaries["scalar"]["Loss-Hartley-Reconstruction"] = spec.detach()
        return spec

    def get_fht_factor(self) -> float:
        return self._hartley.get_fht_factor()

    def set_fht_factor(self, fht_factor: float) -> float:
        return self._hartley.set_fht_factor(fht_factor)


class _BaselinePerceptualFn(torch.autograd.Function):
    """``perceptual_factor * (mean LPIPS over the kept sagittal slices + axial + coronal)`` and its gradient to the prediction, computed in the forward pass;
    returns the differentiable scaled sum and the three UNSCALED per-view means (sagittal, axial, coronal) as non-differentiable side outputs."""

    VIEWS = (0, 2, 1)       # sagittal (0,2,1,3,4), axial (0,4,1,2,3), coronal (0,3,1,2,4): upstream's order of evaluation and of the sum

    @staticmethod
    def forward(ctx, pred, target, net, ids, factor: float, chunk):
        from . import lpips
        ctx.grad, sums = lpips.view_sums(pred, target, net, _BaselinePerceptualFn.VIEWS, ids, factor, False, chunk)      # (upstream calls LPIPS without normalize)
        means = [s.div(vid.numel()).float() for s, vid in zip(sums, ids)]
        total = ((means[0] + means[1]) + means[2]) * factor
        ctx.mark_non_differentiable(*means)
        return (total, *means)

    @staticmethod
    def backward(ctx, g, *_):
        # re-entrant like _MSEFn: the stored d loss / d pred is neither consumed nor scaled in place
        grad = ctx.grad
        return (grad * g if grad is not None else None), None, None, None, None, None


class BaselineLoss(_SliceLpipsLoss):
    """``BaselineLoss()`` of the reference (src/losses/vqvae/vqvae.py:1648-1780, ``--loss=baseline``): ``pixel_factor * l1(pred, y) + fft_factor *
    mse(|fftn((y + 1) / 2)|, |fftn((pred + 1) / 2)|) + perceptual_factor * (three-plane mean LPIPS-squeeze) + sum(quantization_losses)``.

    * perceptual term: losses/lpips_squeeze.py: per plane ``min(n_slices, B n)`` slices, drawn by ``lpips.draw_slices(seed, step,
      view, ...)`` -- the project's draw, standing in for upstream's ``torch.randperm`` --, LPIPS WITHOUT ``normalize`` (upstream passes the volumes as they are);
    * frequency term: upstream's ``fftn`` names no ``dim``, so it transforms ALL five axes, the batch included.  With C = 1 that is :class:`JukeboxLoss`'
      amplitude term on the volumes viewed as [1, B, D, H, W] (the batch takes the channel axis' place): rocFFT through ``torch.fft.fftn``, with
      upstream's ``torch.abs`` (zero gradient at an empty bin, so constant volumes stay finite);
    * pixel term: ``F.l1_loss``, a bandwidth-trivial pass of torch's elementwise operators (``sa_baur_loss`` cannot leave its L2 term out).

    Upstream's constructor takes no arguments; this build adds ``perceptual_weights`` (a validated LPIPS-squeeze state dict), ``compute_dtype`` and ``seed``.
    ``pixel_factor``, ``perceptual_factor``, ``n_slices`` and ``fft_factor`` are plain settable attributes and the summary keys are upstream's."""

    def __init__(self, *, perceptual_weights: Dict = None, compute_dtype: torch.dtype = torch.float32, seed: int = 0):
        super().__init__()
        if perceptual_weights is None:
            raise ValueError("BaselineLoss: perceptual_weights is required (this build downloads nothing): "
                             "losses.lpips.load_weights(<file> | 'random:<seed>', net='squeeze')")
        self.pixel_factor = 1.0
        self.perceptual_factor = 0.002
        self.n_slices = 512
        self.perceptual_function, self._min_side = _lpips_network("BaselineLoss", "squeeze", perceptual_weights, compute_dtype)
        self.fft_factor = 1.0
        self.seed, self.step = int(seed), 0
        self.chunk_slices = None           # None: from the workspace cap (tests set it)
        self.summaries: Dict = {"scalar": {}}

    def _check(self, y_pred: torch.Tensor, y: torch.Tensor):
        self._check_volumes(y_pred, y)
        if min(y_pred.shape[2:]) < self._min_side:
            raise ValueError(f"BaselineLoss: every slice side must be >= {self._min_side} (the smallest for which SqueezeNet's third ceil-mode pool still has "
                             f"an output); got a volume of {' x '.join(map(str, y_pred.shape[2:]))}")
        if int(self.n_slices) < 1:
            raise ValueError(f"BaselineLoss: n_slices must be >= 1; got {self.n_slices}")

    def _calculate_pixel_loss(self, y_pred, y):
        loss = torch.nn.functional.l1_loss(y_pred, y) * self.pixel_factor
        self.summaries["scalar"]["Loss-MAE-Reconstruction"] = loss.detach()
        return loss

    def _calculate_frequency_loss(self, y_pred, y):
        shape = (1, *y_pred.shape[:1], *y_pred.shape[2:])

        def amplitude(t):
            # the affine (t + 1) / 2 is one elementwise pass in front of the transform; torch.abs, as upstream: its gradient at an empty bin is 0, not NaN
            return torch.abs(torch.fft.fftn(((t + 1.0) * 0.5).reshape(shape), dim=_FFT_DIMS, norm="ortho"))

        with torch.no_grad():
            y_amp = amplitude(y)
        loss = torch.nn.functional.mse_loss(amplitude(y_pred), y_amp) * self.fft_factor
        self.summaries["scalar"]["Loss-Jukebox-Reconstruction"] = loss.detach()
        return loss

    def _calculate_perceptual_loss(self, y_pred, y):
        ids = self._draw_ids(y_pred, _BaselinePerceptualFn.VIEWS, lambda n: min(int(self.n_slices), n))     # (forward's refusals come first)
        loss, sag, axi, cor = _BaselinePerceptualFn.apply(y_pred, y, self.perceptual_function, ids, float(self.perceptual_factor), self.chunk_slices)
        self.summaries["scalar"]["Loss-Perceptual_Sagittal-Reconstruction"] = sag.detach()
        self.summaries["scalar"]["Loss-Perceptual_Axial-Reconstruction"] = axi.detach()
        self.summaries["scalar"]["Loss-Perceptual_Coronal-Reconstruction"] = cor.detach()
        self.summaries["scalar"]["Loss-Perceptual-Reconstruction"] = loss.detach()
        return loss

    def forward(self, network_output: Dict[str, List[torch.Tensor]], y: torch.Tensor) -> torch.Tensor:
        y = y.float()
        y_pred = network_output["reconstruction"][0].float()
        self._check(y_pred, y)
        y = y.to(y_pred.device)
        loss = self._calculate_pixel_loss(y_pred, y) + self._calculate_frequency_loss(y_pred, y) + self._calculate_perceptual_loss(y_pred, y)
        return self._add_commitment(loss, network_output)


# the reference's src/losses/vqvae/utils.py list, complete; the LPIPS family and "baseline" (LPIPS-squeeze) need --perceptual_weights (this build downloads nothing)
VQVAE_LOSSES = ("baur", "mse", "jukebox", "spectral", "hartley", "wavegan", "perceptual", "jukebox_perceptual", "hartley_perceptual", "baseline")
_PERCEPTUAL_LOSSES = {"perceptual": PerceptualLoss, "jukebox_perceptual": JukeboxPerceptualLoss, "hartley_perceptual": HartleyPerceptualLoss}


def _lpips_arguments(config: dict, net: str) -> dict:
    """what the configuration gives every loss with an LPIPS term: the validated weights of ``net``, the compute dtype and the seed of the slice draw"""
    from . import lpips
    weights = config["perceptual_weights"]
    if not isinstance(weights, dict):
        weights = lpips.load_weights(weights, net=net)
    dtype = config.get("compute_dtype") or (torch.bfloat16 if config.get("amp") else torch.float32)
    return {"perceptual_weights": weights, "compute_dtype": dtype, "seed": int(config.get("seed") or 0)}


def get_vqvae_loss(config: dict) -> torch.nn.Module:
    """src/losses/vqvae/configure.py:22-52 for the losses this build implements."""
    if config["loss"] == "baur":
        return BaurLoss()
    if config["loss"] == "mse":
        return MSELoss()
    if config["loss"] == "jukebox":
        return JukeboxLoss(dimensions=3)
    if config["loss"] == "spectral":
        return SpectralLoss(dimensions=3)
    if config["loss"] == "hartley":
        return HartleyLoss(dimensions=3)
    if config["loss"] == "wavegan":
        return WaveGANLoss(dimensions=3)
    if config["loss"] in _PERCEPTUAL_LOSSES and config.get("perceptual_weights"):
        # drop_ratio 0.5 as src/losses/vqvae/configure.py:40-45; the weights come from --perceptual_weights (host only, refused by name when wrong)
        return _PERCEPTUAL_LOSSES[config["loss"]](dimensions=3, drop_ratio=0.5, **_lpips_arguments(config, "alex"))
    if config["loss"] == "baseline" and config.get("perceptual_weights"):
        # src/losses/vqvae/configure.py builds BaselineLoss() without arguments; the LPIPS-squeeze weights come from --perceptual_weights
        return BaselineLoss(**_lpips_arguments(config, "squeeze"))
    hint = " The LPIPS family needs --perceptual_weights=<file | random:seed>." if config["loss"] in (*_PERCEPTUAL_LOSSES, "baseline") else ""
    raise ValueError(f"Loss function unknown. Was given {config['loss']} but choices are {list(VQVAE_LOSSES)}.{hint}")
