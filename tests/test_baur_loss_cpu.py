"""CPU: the host side of ``--loss=baur`` -- the gdl_factor schedule against the reference's ``ParamSchedulerHandler._linear`` values, the factory,
the constructor's reduction check, and the C entry points' argument checks (no launch happens for a rejected call)."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden


def _cfg(init, const, steps, top):
    return {"initial_factor_value": init, "initial_factor_steps": const, "max_factor_steps": steps, "max_factor_value": top}


def test_schedule_matches_the_reference_table():
    from synthanatomy_amd.losses.vqvae import gdl_factor_schedule
    g = load_golden("losses_baur")
    for (init, const, steps, top, s), want in zip(g["schedule/args"].tolist(), g["schedule/values"].tolist()):
        assert gdl_factor_schedule(_cfg(init, const, steps, top), int(s)) == pytest.approx(want, abs=1e-12), (init, const, steps, top, s)


def test_schedule_at_the_cli_defaults():
    """run_vqvae.py defaults (0, 25, 50, 5): 0 through 25 finished epochs, then (s - 25) / 50 * 5 -- 2.5 at 50 -- and 5.0 from 51 on (the ramp divides by
    max_factor_steps, reference src/handlers/general.py:113-116)."""
    import run_vqvae
    from synthanatomy_amd.losses.vqvae import gdl_factor_schedule
    cfg = dict(run_vqvae.DEFAULTS)
    assert [gdl_factor_schedule(cfg, s) for s in (0, 1, 25)] == [0, 0, 0]
    assert gdl_factor_schedule(cfg, 26) == pytest.approx(0.1)
    assert gdl_factor_schedule(cfg, 50) == pytest.approx(2.5)
    assert gdl_factor_schedule(cfg, 51) == 5.0 == gdl_factor_schedule(cfg, 100)
    # before step_constant upstream adds initial_value twice (general.py:110-111): kept as upstream computes it
    assert gdl_factor_schedule(_cfg(0.5, 1, 2, 3), 0) == pytest.approx(1.0)
    assert [gdl_factor_schedule(_cfg(0.5, 1, 2, 3), s) for s in (1, 2, 3)] == pytest.approx([0.5, 1.75, 3.0])


def test_factory_and_constructor():
    from synthanatomy_amd.losses.vqvae import VQVAE_LOSSES, BaurLoss, get_vqvae_loss
    fn = get_vqvae_loss({"loss": "baur"})
    assert isinstance(fn, BaurLoss) and fn.get_gdl_factor() == 0.0 and fn.reduction == "mean"
    assert "baur" in VQVAE_LOSSES
    assert fn.set_gdl_factor(1.25) == 1.25 == fn.get_gdl_factor()
    assert BaurLoss(reduction="sum").reduction == "sum"
    for bad in ("none", "avg", None):
        with pytest.raises(ValueError):
            BaurLoss(reduction=bad)


def test_extent_below_three_is_a_value_error_before_any_launch():
    import torch
    from synthanatomy_amd.losses.vqvae import BaurLoss
    fn = BaurLoss()
    for shape in ((1, 1, 2, 8, 8), (1, 1, 8, 2, 8), (1, 1, 8, 8, 2), (8, 8, 8)):
        with pytest.raises(ValueError, match=r"\(" + ", ".join(str(s) for s in shape)):
            fn({"reconstruction": [torch.zeros(shape)], "quantization_losses": []}, torch.zeros(shape))


def test_entry_points_reject_bad_arguments():
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    for name, (res, args) in _ffi._SIGS.items():
        if name.startswith("sa_baur_loss"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    assert lib.sa_baur_loss_workspace_bytes(8, 160, 224, 160) > 0
    assert lib.sa_baur_loss_workspace_bytes(8, 160, 224, 160) % 12 == 0
    for shape in ((1, 2, 5, 5), (1, 5, 2, 5), (1, 5, 5, 2), (0, 5, 5, 5)):
        assert lib.sa_baur_loss_workspace_bytes(*shape) == _ffi.SA_EINVAL
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        pred, target, sums, ws = args
        assert lib.sa_baur_loss(pred, target, 1, 3, 3, 3, 1.0, 0, 1.0, sums, None, ws, None) == _ffi.SA_EINVAL
    assert lib.sa_baur_loss(p, p, 1, 2, 3, 3, 1.0, 0, 1.0, p, None, p, None) == _ffi.SA_EINVAL
    assert lib.sa_baur_loss(p, p, 1, 3, 3, 2, 1.0, 0, 1.0, p, None, p, None) == _ffi.SA_EINVAL
    assert np.all(np.frombuffer(buf, dtype=np.float32) == 0)      # nothing was written
