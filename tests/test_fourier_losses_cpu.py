"""CPU: the host side of ``--loss=spectral | hartley | wavegan`` (reference src/losses/vqvae/vqvae.py:188-323, 326-519, 641-771) -- the factory, the
constructors' defaults and refusals, the factor getters and setters, the fp64 half-spectrum restatement (tests/fourier_ref.py) against the values the
reference's classes compute (tests/golden/losses_fourier.npz), and the C entry points' declarations and argument checks (no launch happens for a
rejected call)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fourier_ref
from conftest import ROOT, load_golden

SHAPES = ("even_w", "odd_w", "background")
LOSSES = ("spectral", "hartley", "hartley_flat", "wavegan")


def test_factory_builds_the_three_fourier_losses():
    from synthanatomy_amd.losses.vqvae import VQVAE_LOSSES, HartleyLoss, SpectralLoss, WaveGANLoss, get_vqvae_loss
    for name, cls in (("spectral", SpectralLoss), ("hartley", HartleyLoss), ("wavegan", WaveGANLoss)):
        assert name in VQVAE_LOSSES
        fn = get_vqvae_loss({"loss": name})
        assert type(fn) is cls and fn.dimensions == 3 and fn.include_pixel_loss and fn.reduction == "mean"
        assert fn.fft_kwargs == {"s": None, "dim": (1, 2, 3, 4), "norm": "ortho"}
    assert get_vqvae_loss({"loss": "hartley"}).prioritise_high_frequency is True


def test_lpips_family_still_raises():
    from synthanatomy_amd.losses.vqvae import get_vqvae_loss
    for name in ("lpips", "perceptual", "jukebox_perceptual", "hartley_perceptual", "baseline"):
        with pytest.raises(ValueError, match="Loss function unknown"):
            get_vqvae_loss({"loss": name})


def test_factor_getters_and_setters():
    from synthanatomy_amd.losses.vqvae import HartleyLoss, SpectralLoss, WaveGANLoss
    for cls in (SpectralLoss, WaveGANLoss):
        fn = cls(dimensions=3)
        assert fn.get_fft_factor() == 1.0 == fn.fft_factor
        assert fn.set_fft_factor(0.25) == 0.25 == fn.get_fft_factor() == fn.fft_factor
    fn = HartleyLoss(dimensions=3, prioritise_high_frequency=False, include_pixel_loss=False)
    assert fn.get_fht_factor() == 1.0 == fn.fht_factor and not fn.prioritise_high_frequency and not fn.include_pixel_loss
    assert fn.set_fht_factor(3.5) == 3.5 == fn.get_fht_factor()


def test_unsupported_arguments_raise_not_implemented():
    from synthanatomy_amd.losses.vqvae import HartleyLoss, SpectralLoss, WaveGANLoss
    for cls in (SpectralLoss, HartleyLoss, WaveGANLoss):
        with pytest.raises(NotImplementedError, match="dimensions"):
            cls(dimensions=2)
        with pytest.raises(NotImplementedError, match="fft_kwargs"):
            cls(dimensions=3, fft_kwargs={"s": None, "dim": (2, 3, 4), "norm": "ortho"})
        with pytest.raises(NotImplementedError, match="fft_kwargs"):
            cls(dimensions=3, fft_kwargs={"s": None, "dim": (1, 2, 3, 4), "norm": "backward"})
        with pytest.raises(NotImplementedError, match="reduction"):
            cls(dimensions=3, reduction="none")
        assert cls(dimensions=3, fft_kwargs={"s": None, "dim": (1, 2, 3, 4), "norm": "ortho"}).dimensions == 3     # the default, spelled out


def test_bad_volume_is_a_value_error_before_any_launch():
    from synthanatomy_amd.losses.vqvae import SpectralLoss
    fn = SpectralLoss(dimensions=3)
    for shape in ((1, 1, 1, 8, 8), (8, 8, 8)):
        with pytest.raises(ValueError, match=r"\(" + ", ".join(str(s) for s in shape)):
            fn({"reconstruction": [torch.zeros(shape)], "quantization_losses": []}, torch.zeros(shape))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", LOSSES)
def test_restatement_matches_the_reference_golden(name, shape):
    g = load_golden("losses_fourier")
    c = f"case/{name}/{shape}/"
    y, pred, q = (torch.from_numpy(g[f"input/{shape}/{k}"]).double() for k in ("y", "pred", "qloss"))
    loss, summ, grad = fourier_ref.by_name(name, pred, y, q)
    np.testing.assert_allclose(float(loss), g[c + "loss"], rtol=1e-10)
    keys = sorted(k[len(c):] for k in g.files if k.startswith(c) and k[len(c):] not in ("loss", "dpred"))
    assert keys == sorted(summ)
    for k in keys:
        np.testing.assert_allclose(float(summ[k]), g[c + k], rtol=1e-10, err_msg=k)
    ref = torch.from_numpy(g[c + "dpred"])
    assert float((grad - ref).norm() / ref.norm()) < 1e-10


def test_self_conjugate_bins_decide_the_phase():
    """Im = -0 instead of +0 on one self-conjugate bin with a negative real part moves dphi there by 2 pi: the phase term changes by a large fraction,
    which is why the kernel forces +0 (the sign the reference's CPU fftn produces)."""
    g = load_golden("losses_fourier")
    y, pred = (torch.from_numpy(g[f"input/even_w/{k}"]).double() for k in ("y", "pred"))
    Yp, Yy, m, sc = fourier_ref._spectra(pred, y)
    assert int(sc.sum()) == 4      # the [C, D, H, W/2 + 1] mask: 1 (C = 1) x 1 (D = 5 is odd) x 2 (H) x 2 (k_W = 0, W/2)
    neg = sc & (Yp.real < 0)
    assert bool(neg.any())
    phi = torch.angle(Yp)
    flipped = torch.where(neg, -phi, phi)
    e0, e1 = torch.exp((phi - torch.angle(Yy)).abs()), torch.exp((flipped - torch.angle(Yy)).abs())
    n = pred.numel()
    p0, p1 = 0.5 / n * (m * (1 - e0) ** 2).sum(), 0.5 / n * (m * (1 - e1) ** 2).sum()
    assert abs(float(p1 - p0)) / float(p0) > 1e-3


def test_header_declares_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "synthanatomy_hip.h")).read()
    assert re.search(r"int sa_fourier_loss\(int kind, const float \*xp, const float \*xy, int64_t B, int C, int D, int H, int W, int prioritise_hf, "
                     r"float factor, double \*sums,\s+float \*grad, void \*ws, void \*stream\);", txt)
    assert "int64_t sa_fourier_loss_workspace_bytes(int64_t B, int C, int D, int H, int W);" in txt
    assert re.search(r"SA_FOURIER_SPECTRAL = 0, SA_FOURIER_HARTLEY = 1, SA_FOURIER_WAVEGAN = 2", txt)
    assert "vqvae.py:188-323" in txt and ":326-519" in txt and ":641-771" in txt


def test_entry_points_reject_bad_arguments():
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    for name, (res, args) in _ffi._SIGS.items():
        if name.startswith("sa_fourier_loss"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    ws = lib.sa_fourier_loss_workspace_bytes(8, 1, 160, 224, 160)
    assert ws > 0 and ws % 24 == 0
    for shape in ((0, 1, 4, 4, 4), (1, 0, 4, 4, 4), (1, 1, 1, 4, 4), (1, 1, 4, 1, 4), (1, 1, 4, 4, 1)):
        assert lib.sa_fourier_loss_workspace_bytes(*shape) == _ffi.SA_EINVAL
    assert lib.sa_fourier_loss_workspace_bytes(1 << 20, 1, 64, 64, 64) == _ffi.SA_EUNSUPPORTED
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for xp, xy, sums, w in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.sa_fourier_loss(0, xp, xy, 1, 1, 4, 4, 4, 1, 1.0, sums, None, w, None) == _ffi.SA_EINVAL
    for kind in (-1, 3):
        assert lib.sa_fourier_loss(kind, p, p, 1, 1, 4, 4, 4, 1, 1.0, p, p, p, None) == _ffi.SA_EINVAL
    assert lib.sa_fourier_loss(1, p, p, 1, 1, 4, 1, 4, 1, 1.0, p, p, p, None) == _ffi.SA_EINVAL
    assert lib.sa_fourier_loss(2, p, p, 1, 0, 4, 4, 4, 1, 1.0, p, p, p, None) == _ffi.SA_EINVAL
    assert np.all(np.frombuffer(buf, dtype=np.float32) == 0)      # nothing was written
