"""CPU: run_transformer.py --mode=healing up to the point where a device is needed -- the flag's refusals (before anything touches the device), the
refusal of a code file the vocabulary does not cover, the three output files and what the decoding stage picks up of them."""
import os

import numpy as np
import pytest
import torch

import run_transformer as RT
from synthanatomy_amd.utils.general import list_inputs


class _DeviceTouched(Exception):
    pass


def _argv(tmp_path, *extra):
    return ["run", "--training_subjects=synthetic:2", "--validation_subjects=synthetic:2", f"--project_directory={tmp_path}/", "--experiment_name=e",
            *extra]


@pytest.fixture
def no_device(monkeypatch):
    """run() reaches the device through init_distributed first: any path that gets there raises _DeviceTouched"""
    from synthanatomy_amd.runtime import ddp

    def touched():
        raise _DeviceTouched()
    monkeypatch.setattr(ddp, "init_distributed", touched)
    monkeypatch.setattr(torch.cuda, "is_available", touched)


@pytest.mark.parametrize("value", ["0", "0.0", "-0.25", "1.5", "2", "abc", "True", "(0.5,)"])
def test_a_threshold_outside_the_unit_interval_is_refused_before_the_device(tmp_path, no_device, value):
    with pytest.raises(ValueError, match="--resample_threshold"):
        RT.run(_argv(tmp_path, "--mode=healing", f"--resample_threshold={value}"))
    assert not os.path.exists(tmp_path / "e")          # not even the folder structure


@pytest.mark.parametrize("extra", [(), ("--resample_threshold=None",), ("--resample_threshold=0.05",), ("--resample_threshold=1",), ("--resample_threshold=1e-9",)])
def test_a_valid_threshold_goes_on_to_the_device(tmp_path, no_device, extra):
    with pytest.raises(_DeviceTouched):
        RT.run(_argv(tmp_path, "--mode=healing", *extra))
    assert RT.DEFAULTS["resample_threshold"] is None
    assert RT.resample_threshold(None) is None and RT.resample_threshold(1) == 1.0 and RT.resample_threshold(0.05) == 0.05


def test_the_flag_is_not_checked_in_the_other_modes_and_an_unknown_mode_names_all_three(tmp_path, no_device):
    with pytest.raises(_DeviceTouched):
        RT.run(_argv(tmp_path, "--mode=inference", "--resample_threshold=7"))
    with pytest.raises(ValueError, match=r"bogus.*\['training', 'inference', 'healing'\]"):
        RT.run(_argv(tmp_path, "--mode=bogus"))


def test_a_code_outside_the_vocabulary_is_refused_by_file_name(tmp_path):
    cfg = dict(vocab_size=16, seed=0, spatial_shape=(2, 2, 2))
    good, high, low = (str(tmp_path / f"{n}_quantization_0.npy") for n in ("good", "high", "low"))
    np.save(good, np.arange(8, dtype=np.uint16).reshape(2, 2, 2) + 8)
    np.save(high, np.full((2, 2, 2), 16, dtype=np.uint16))
    np.save(low, np.array([0, 1, -1, 3, 4, 5, 6, 7], dtype=np.int32).reshape(2, 2, 2))
    assert torch.equal(RT.checked_codes(good, cfg, None), torch.arange(8, 16).reshape(2, 2, 2))
    for bad in (high, low):
        with pytest.raises(ValueError, match=os.path.basename(bad)):
            RT.checked_codes(bad, cfg, None)
    assert RT.checked_codes("synthetic_0001", cfg, None).shape == (2, 2, 2)


def test_the_three_outputs_and_what_decoding_lists(tmp_path):
    out = str(tmp_path / "outputs") + "/"
    healed = np.arange(24).reshape(2, 3, 4) * 100
    nll = np.linspace(0.0, 9.0, 24).reshape(2, 3, 4)
    rep = (np.arange(24).reshape(2, 3, 4) % 5 == 0)
    for name in ("a_quantization_0.npy", "b_quantization_0.npy"):
        paths = RT.save_healing(healed, nll, rep, out, "/somewhere/" + name)
        stem = name[:-4]
        assert [os.path.relpath(p, out) for p in paths] == [f"{stem}/{stem}_{post}.npy" for post in ("healed_sample", "nll", "resampled")]
        h, n, r = (np.load(p) for p in paths)
        assert (h.dtype, n.dtype, r.dtype) == (np.uint16, np.float32, np.uint8)
        assert np.array_equal(h, healed) and np.array_equal(n, nll.astype(np.float32)) and np.array_equal(r, rep.astype(np.uint8))
    listed = list_inputs(out, postfix="sample")
    assert [os.path.basename(p) for p in listed] == ["a_quantization_0_healed_sample.npy", "b_quantization_0_healed_sample.npy"]
