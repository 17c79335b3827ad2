"""GPU: ``run_vqvae.py --augmentation`` / ``--patch_size`` / ``--no_augmented_extractions``.  The switch at probability 0 changes nothing;
at probability 1 the run is reproducible, differs from the plain one and resumes onto the same draws; ``--patch_size`` feeds 16^3 patches and the
augmented extraction writes ``<name>_<i>`` files."""
import glob
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AUG = ["--augmentation=True", "--augmentation_probability=1", "--augmentation_strength=1"]


def _flags(proj, exp, extra=()):
    from test_baur_cli_gpu import _flags as baur_flags
    return baur_flags(proj, exp, ["--deterministic", *extra])


@pytest.fixture(autouse=True)
def _leave_deterministic_mode():
    yield
    from synthanatomy_amd import debug
    debug.set_deterministic(False)                # the CLI switched the process-wide library flag on


def _train(capsys, proj, exp, extra, epochs):
    import run_vqvae
    run_vqvae.run(_flags(proj, exp, extra) + [f"--epochs={epochs}"])
    out = capsys.readouterr().out
    return [l for l in out.splitlines() if re.match(r"epoch \d+ (it|validation)", l)]


def _losses(lines):
    got = [m.group(1) for l in lines for m in [re.match(r"epoch \d+ it \d+ loss (\S+)", l)] if m]
    assert got and all(np.isfinite(float(v)) for v in got)
    return got


def test_probability_zero_changes_no_logged_digit(tmp_path, capsys):
    proj = str(tmp_path) + "/"
    plain = _train(capsys, proj, "plain", [], 2)
    ident = _train(capsys, proj, "ident", ["--augmentation=True", "--augmentation_probability=0"], 2)
    assert len(_losses(plain)) == 4 and _losses(plain) == _losses(ident)
    assert [l for l in plain if "validation" in l] == [l for l in ident if "validation" in l]
    assert not any("noise_seed" in l for l in plain) and all("input 32x32x32 noise_seed 0x" in l for l in ident if " it " in l)


def test_augmented_run_is_reproducible_differs_and_resumes(tmp_path, capsys):
    proj = str(tmp_path) + "/"
    plain = _train(capsys, proj, "plain", [], 2)
    a = _train(capsys, proj, "a", AUG, 2)
    b = _train(capsys, proj, "b", AUG, 2)
    assert a == b and len(_losses(a)) == 4
    assert all(x != y for x, y in zip(_losses(a), _losses(plain)))
    seeds = [re.search(r"noise_seed (0x[0-9a-f]{16})", l).group(1) for l in a if " it " in l]
    assert len(set(seeds)) == 4                                      # one noise seed per iteration
    # one epoch, then a resumed run for the second: the draws are keyed on (epoch, subject) and the noise on the iteration, not on call counts
    first = _train(capsys, proj, "split", AUG, 1)
    second = _train(capsys, proj, "split", AUG, 2)
    assert first + second == a


def test_patch_size_feeds_patches_and_extraction_writes_augmented_files(tmp_path, capsys):
    import run_vqvae
    proj = str(tmp_path) + "/"
    patch = ["--patch_size=(16,16,16)"]
    lines = _train(capsys, proj, "patch", AUG + patch, 1)
    assert len(_losses(lines)) == 2 and all("input 16x16x16 " in l for l in lines if " it " in l)
    crop_only = _train(capsys, proj, "crop", patch, 1)               # without the switch: the random crop alone
    assert all("input 16x16x16 " in l for l in crop_only if " it " in l) and _losses(crop_only) != _losses(lines)
    run_vqvae.run(_flags(proj, "patch", patch) + ["--mode=extracting", "--no_augmented_extractions=2"])      # no --augmentation needed, as upstream
    capsys.readouterr()
    out = proj + "patch/baseline_vqvae/outputs/"
    assert sorted(os.listdir(out)) == [f"synthetic_{s:04d}_{i}" for s in range(2) for i in range(2)]
    assert len(glob.glob(out + "*/*_quantization_0.npy")) == 4
    # the files hold the checkpoint's codes of subject s augmented with the draws of (augmentation id i, subject s): two different inputs per subject
    # (a network two iterations old may still map them to the same codes, so the inputs are compared, and the files with their recomputation)
    import torch
    from synthanatomy_amd.utils.general import load_network_state, parse_flags
    from synthanatomy_amd.utils.vqvae import draw_augmentation, hip_augment
    cfg = parse_flags(_flags(proj, "patch", patch) + ["--mode=extracting", "--no_augmented_extractions=2"], run_vqvae.DEFAULTS)
    dev = torch.device("cuda", 0)
    net = run_vqvae.build_network(cfg, dev).eval()
    load_network_state(net, glob.glob(proj + "patch/baseline_vqvae/checkpoints/checkpoint_epoch=1.pt")[0])
    for s in range(2):
        codes = [np.load(f"{out}synthetic_{s:04d}_{i}/synthetic_{s:04d}_{i}_quantization_0.npy") for i in range(2)]
        recs = [np.load(f"{out}synthetic_{s:04d}_{i}/synthetic_{s:04d}_{i}_reconstruction.npy") for i in range(2)]
        assert all(c.dtype == np.uint16 and c.shape == (4, 4, 4) for c in codes) and all(r.shape == (16, 16, 16) for r in recs)
        x = run_vqvae._load_volume(f"synthetic_{s:04d}", cfg, None, dev)
        draws = [draw_augmentation(cfg, "extracting", cfg["seed"], i, s, (32, 32, 32)) for i in range(2)]
        assert draws[0].tobytes() != draws[1].tobytes()
        xa = hip_augment(torch.stack([x, x]), np.stack(draws), (16, 16, 16), run_vqvae._noise_seed(cfg["seed"], s, 2))      # batch s = subject s, ids 0 and 1
        assert xa.shape == (2, 1, 16, 16, 16) and not torch.equal(xa[0], xa[1])
        with torch.no_grad():
            idx = net.index_quantize(xa)[0]
            rec = net.decode_samples([idx]).float().cpu().numpy()
        for i in range(2):
            assert np.array_equal(codes[i], idx[i].cpu().numpy().astype(np.uint16)) and np.array_equal(recs[i], rec[i, 0])
