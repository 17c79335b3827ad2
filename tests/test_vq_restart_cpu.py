"""CPU: the host side of dead-code restarts and of the EMA decay warm-up -- the donor index rule, ``decay_schedule`` against the reference's
rule written out, the flags' refusals, and that nothing changes while the feature is off."""
import math
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vq_restart_ref as ref  # noqa: E402


@pytest.mark.parametrize("Mtot,R", [(37, 4), (74, 4), (3, 8), (89600, 32)])
def test_donor_rows_are_distinct_in_range_and_one_per_stratum(Mtot, R):
    r_eff = min(R, Mtot)
    stride = Mtot // r_eff
    for seed, step in ((4, 0), (4, 1), (5, 0), (2 ** 40 + 3, 2 ** 33 + 9)):
        g = ref.donor_indices(Mtot, R, seed, step)
        assert len(g) == r_eff == len(set(g))
        assert all(0 <= v < Mtot for v in g)
        assert [v // stride for v in g] == list(range(r_eff))      # stratum j = [j stride, (j + 1) stride)


def test_draws_depend_on_step_and_seed():
    draws = {(seed, step): tuple(ref.donor_indices(89600, 32, seed, step)) for seed in (4, 5, 4 + (1 << 32)) for step in (0, 1, 2, 1 << 32)}
    assert len(set(draws.values())) == len(draws)
    assert draws[(4, 1)] == tuple(ref.donor_indices(89600, 32, 4, 1))      # and on nothing else


def test_idle_rule_and_substitution():
    idle = np.array([0, 1, 2, 5, ref.INT32_MAX, 1, 2], dtype=np.int32)
    counts = np.array([0, 0, 0, 3, 0, 2, 0], dtype=np.float32)
    new, info = ref.idle_rule(idle, counts, 3, 2)
    assert list(info) == [3, 2, 2, 4]                  # codes 2, 4 and 6 are dead; the cap takes the first two
    assert list(new) == [1, 2, 0, 0, 0, 0, 3]          # code 6 keeps counting
    new, info = ref.idle_rule(np.array([ref.INT32_MAX], dtype=np.int32), np.zeros(1), 1, 1)
    assert list(info) == [1, 1, 0]
    new, _ = ref.idle_rule(np.array([ref.INT32_MAX, ref.INT32_MAX], dtype=np.int32), np.zeros(2), 1, 1)
    assert list(new) == [0, ref.INT32_MAX]             # saturates instead of wrapping
    N, avg, c, dw = ref.substitute(np.ones(3), np.ones((3, 2)), np.full(3, 5.0), np.ones((3, 2)), [1], np.array([[7.0, 8.0]]))
    assert list(N) == [1, 0, 1] and list(c) == [5, 1, 5] and avg[1].tolist() == [0, 0] and dw[1].tolist() == [7, 8] and dw[0].tolist() == [1, 1]


# ------------------------------------------------------------------------------------------------ decay warm-up
def _written_out(kind, decay, top, s):
    """reference src/networks/vqvae/configure.py:46-59 and src/handlers/general.py:111-120 (step_constant = 0, max_value = 0.99), read on decay[0]"""
    if kind == "step":
        delta_step = (0.99 - decay) / 4
        stair_steps = np.linspace(0, top, 5)[1:]
        for n in (3, 2, 1, 0):
            if (s + 1) >= stair_steps[n]:
                return decay + (n + 1) * delta_step
        return decay
    if s < 0:
        delta = decay
    elif s > top:
        delta = 0.99 - decay
    else:
        delta = (0.99 - decay) * ((s - 0) / top)
    return decay + delta


@pytest.mark.parametrize("kind", ["step", "linear"])
def test_decay_schedule_is_the_reference_rule(kind):
    from synthanatomy_amd.networks.vqvae.configure import decay_schedule
    cfg = dict(decay=(0.5,), decay_warmup=kind, max_decay_epochs=50)
    epochs = (0, 11, 12, 24, 37, 49, 50, 51)
    got = [decay_schedule(cfg, s) for s in epochs]
    assert got == pytest.approx([_written_out(kind, 0.5, 50, s) for s in epochs], abs=1e-15)
    if kind == "step":
        assert got == pytest.approx([0.5, 0.5, 0.6225, 0.745, 0.8675, 0.99, 0.99, 0.99], abs=1e-12)
    else:
        assert got == pytest.approx([0.5, 0.5 + 0.49 * 11 / 50, 0.5 + 0.49 * 12 / 50, 0.5 + 0.49 * 24 / 50, 0.5 + 0.49 * 37 / 50, 0.5 + 0.49 * 49 / 50, 0.99, 0.99],
                                    abs=1e-12)
    # "auto": ceil(200 * 437 * 32 / (epoch_length * batch_size)) epochs (reference src/utils/general.py:51-72)
    auto = dict(cfg, max_decay_epochs="auto", epoch_length=437, batch_size=256)
    top = math.ceil(200 * 437 * 32 / (437 * 256))
    assert top == 25
    for s in epochs:
        assert decay_schedule(auto, s) == pytest.approx(_written_out(kind, 0.5, top, s), abs=1e-15)
    assert decay_schedule(dict(cfg, decay_warmup=None), 30) == 0.5


# ------------------------------------------------------------------------------------------------ flags
BASE = ["--training_subjects=synthetic:2", "--validation_subjects=synthetic:1", "--experiment_name=e"]


def test_every_refusal_names_its_flag_before_any_device_call(tmp_path, monkeypatch):
    import torch

    import run_vqvae
    import synthanatomy_amd.networks.vqvae.configure  # noqa: F401  (imported before the device calls are booby-trapped)
    from synthanatomy_amd.runtime import ddp

    def no_device(*a, **k):
        raise AssertionError("a device call was made before the refusal")

    monkeypatch.setattr(ddp, "init_distributed", no_device)
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "current_stream", no_device)
    base = BASE + ["--project_directory=" + str(tmp_path) + "/"]

    def refuse(flag, *more, mode="training"):
        with pytest.raises(ValueError) as e:
            run_vqvae.run(base + [f"--mode={mode}", flag, *more])
        assert str(e.value).startswith(flag.split("=")[0] + "="), str(e.value)

    for v in ("0", "-3", "2.5", "True", "soon"):
        refuse(f"--codebook_restart_patience={v}")
    for v in ("0", "65", "1.5", "False", "many"):
        refuse(f"--codebook_restart_max={v}", "--codebook_restart_patience=2")
    refuse("--codebook_restart_max=16")                                         # without a patience it would never act
    for mode in ("extracting", "decoding", "anomaly"):
        refuse("--codebook_restart_patience=2", mode=mode)
        refuse("--codebook_restart_max=16", mode=mode)
    for v in ("cosine", "True", "3"):
        refuse(f"--decay_warmup={v}")
    for v in ("0", "-1", "2.5", "never", "None"):
        refuse(f"--max_decay_epochs={v}", "--decay_warmup=linear")
    assert not os.listdir(tmp_path)      # nothing was created either


def test_header_declares_the_two_entry_points():
    from synthanatomy_amd import _ffi
    txt = open(os.path.join(ROOT, "include", "synthanatomy_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+sa_vq_restart_donors\s*\(const float \*rows, int64_t M, int D, int64_t row_base, int64_t Mtot, int R, uint64_t seed, uint64_t step", code)
    assert re.search(r"\bint\s+sa_vq_ema_update_restart\s*\(float \*N, float \*embed_avg, float \*codebook, const float \*counts, const float \*dw, int K, int D", code)
    assert "baseline.py:66-80" in txt[txt.index("Dead-code restarts"):txt.index("sa_vq_restart_donors(")]
    assert re.search(r"#define\s+SA_ABI_VERSION\s+5\b", txt) and _ffi.ABI_VERSION == 5
    for name, nargs in (("sa_vq_restart_donors", 10), ("sa_vq_ema_update_restart", 15)):
        assert name in _ffi.declared_symbols() and len(_ffi._SIGS[name][1]) == nargs
    assert len(_ffi._SIGS["sa_vq_ema_update"][1]) == 10      # the plain update keeps its signature


def test_nothing_changes_while_the_feature_is_off():
    import torch
    from synthanatomy_amd.networks.vqvae.baseline import BaselineVQVAE, CodebookRestartState
    torch.manual_seed(0)
    net = BaselineVQVAE(n_levels=2, downsample_parameters=((4, 2, 1, 1),) * 2, upsample_parameters=((4, 2, 1, 0, 1),) * 2, n_embed=16, embed_dim=8,
                        n_channels=16, n_res_channels=16, n_res_layers=1)
    impl = net.quantizer[0].impl
    keys = list(net.state_dict())
    stats, _ = impl._work_buffers(torch.device("cpu"))
    assert stats.numel() == 16 + 16 * 8 and impl._restart is None and not hasattr(impl, "idle")
    with pytest.raises(RuntimeError, match="off"):
        net.get_codebook_restart_info()
    # on: two buffers that stay off the state_dict, a longer packed buffer [counts | dw | donors]
    net.set_codebook_restart(3, 4, seed=7)
    assert list(net.state_dict()) == keys and [k for k, _ in impl.named_buffers()] == ["N", "embed_avg", "idle", "restart_total"]
    assert impl.idle.dtype == torch.int32 and impl.idle.shape == (16,)
    assert impl._work_buffers(torch.device("cpu"))[0].numel() == 16 + 16 * 8 + 4 * 8
    assert net.get_codebook_restart_info() == {"dead": 0, "restarted": 0, "ids": [], "total": 0}
    net.set_codebook_restart_step(41)
    assert impl._restart_step == 41
    impl.idle[3] = 5
    sd = net.codebook_restart_state().state_dict()
    assert sd["idle"][3] == 5 and sd["total"] == 0 and (sd["patience"], sd["max_per_step"]) == (3, 4)
    impl.idle.zero_()
    CodebookRestartState(impl).load_state_dict(dict(sd, total=9))
    assert impl.idle[3] == 5 and net.get_codebook_restart_info()["total"] == 9
    with pytest.raises(ValueError, match="idle counters"):
        CodebookRestartState(impl).load_state_dict(dict(sd, idle=torch.zeros(5, dtype=torch.int32)))
    for bad in ((0, 4), (2, 0), (2, 65), (True, 4), (2.0, 4)):
        with pytest.raises(ValueError, match="codebook_restart_"):
            net.set_codebook_restart(*bad)
    # and off again
    net.set_codebook_restart(None)
    assert list(net.state_dict()) == keys and not hasattr(impl, "idle") and impl._work_buffers(torch.device("cpu"))[0].numel() == 16 + 16 * 8


def test_default_flags_leave_the_feature_off():
    import run_vqvae
    assert run_vqvae.DEFAULTS["codebook_restart_patience"] is None and run_vqvae.DEFAULTS["codebook_restart_max"] == 32
    assert run_vqvae.DEFAULTS["decay_warmup"] is None and run_vqvae.DEFAULTS["max_decay_epochs"] == 50
