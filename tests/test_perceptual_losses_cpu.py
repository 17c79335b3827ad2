"""CPU: the host side of the LPIPS family (``--loss=perceptual | jukebox_perceptual | hartley_perceptual``): the fp64 restatement of tests/lpips_ref.py
against the fixture made from the reference's own classes, the factory, every refusal, the weight loader and merging tool, the slice draw, and the
witnesses -- each planted defect of lpips_ref must move the golden case by more than the tolerance the GPU tests grant."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lpips_ref
from conftest import ROOT

torch.set_num_threads(min(16, torch.get_num_threads()))
GPU_TOL = 1e-3      # tests/test_perceptual_losses_gpu.py, fp32 mode
NAMES = ("perceptual", "jukebox_perceptual", "hartley_perceptual")


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "losses_perceptual.npz"))


def _inputs(sname):
    gold = _golden()
    return (torch.from_numpy(gold[f"input/{sname}/y_u8"]).float() / 255, torch.from_numpy(gold[f"input/{sname}/pred_u8"]).float() / 255,
            torch.from_numpy(gold[f"input/{sname}/qloss"]))


@pytest.mark.parametrize("sname", ["small", "background"])
@pytest.mark.parametrize("lname", NAMES)
def test_restatement_matches_the_reference_fixture(lname, sname):
    gold = _golden()
    y, pred, q = _inputs(sname)
    sd = lpips_ref.draw_weights(int(gold["seed"]))
    p = pred.double().requires_grad_(True)
    loss, summ = lpips_ref.loss(lname, p, y, q, sd)
    loss.backward()
    c = f"case/{lname}/{sname}/"
    assert abs(float(loss.detach()) - float(gold[c + "loss"])) <= 1e-10
    keys = [k[len(c):] for k in gold.files if k.startswith(c) and k[len(c):] not in ("loss", "dpred_strided")]
    assert sorted(keys) == sorted(summ), (keys, sorted(summ))
    for k in keys:
        assert abs(float(summ[k]) - float(gold[c + k])) <= 1e-10, k
    assert float((p.grad.reshape(-1)[::8] - torch.from_numpy(gold[c + "dpred_strided"])).abs().max()) <= 1e-10


def test_factory_builds_the_family_with_upstream_defaults():
    from synthanatomy_amd.losses import vqvae
    classes = {"perceptual": vqvae.PerceptualLoss, "jukebox_perceptual": vqvae.JukeboxPerceptualLoss, "hartley_perceptual": vqvae.HartleyPerceptualLoss}
    for name in NAMES:
        assert name in vqvae.VQVAE_LOSSES
        fn = vqvae.get_vqvae_loss({"loss": name, "perceptual_weights": "random:0"})
        assert type(fn) is classes[name]
        assert fn.keep_ratio == 0.5 and fn.perceptual_factor == 0.001 and fn.lpips_normalize is True and fn.fake_3D_views == [0, 1, 2]
        assert fn.get_perceptual_factor() == 0.001 and fn.set_perceptual_factor(0.5) == 0.5 == fn.get_perceptual_factor()
        assert not list(fn.parameters()) and not fn.state_dict(), "the frozen weights must be non-persistent buffers"
        assert len(list(fn.buffers())) >= 15
        assert fn.set_step(7) == 7
    jp = vqvae.get_vqvae_loss({"loss": "jukebox_perceptual", "perceptual_weights": "random:0"})
    assert jp.get_fft_factor() == 1.0 == jp.fft_factor and jp.set_fft_factor(0.25) == 0.25 == jp.get_fft_factor() == jp.fft_factor
    hp = vqvae.get_vqvae_loss({"loss": "hartley_perceptual", "perceptual_weights": "random:0"})
    assert hp.get_fht_factor() == 1.0 == hp.fht_factor and hp.set_fht_factor(0.5) == 0.5 == hp.get_fht_factor() == hp.fht_factor
    assert vqvae.get_vqvae_loss({"loss": "perceptual", "perceptual_weights": "random:0", "amp": True}).perceptual_function.compute_dtype == torch.bfloat16
    with pytest.raises(ValueError, match="Loss function unknown.*--perceptual_weights"):
        vqvae.get_vqvae_loss({"loss": "perceptual"})


def test_package_draws_equal_the_restated_ones():
    from synthanatomy_amd.losses import lpips
    a, b = lpips.random_state_dict(3), lpips_ref.draw_weights(3)
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert all(float(a[k].min()) >= 0 for k in lpips.LIN_KEYS)
    for args in ((0, 0, 0, 62, 31), (4, 9, 2, 77, 19), (4, 9, 1, 8, 8)):
        assert np.array_equal(lpips.draw_slices(*args), lpips_ref.draw_slices(*args))


def test_slice_draw():
    from synthanatomy_amd.losses.lpips import draw_slices
    for n, keep in ((62, 0.5), (99, 0.25), (7, 0.9)):
        ids = draw_slices(4, 10, 1, n, int(n * keep))
        assert ids.dtype == np.int32 and len(ids) == int(n * keep) == len(set(ids.tolist())) and ids.min() >= 0 and ids.max() < n
        assert np.array_equal(ids, draw_slices(4, 10, 1, n, int(n * keep)))
    base = draw_slices(4, 10, 1, 200, 100)
    assert not np.array_equal(base, draw_slices(4, 11, 1, 200, 100)), "steps must differ"
    assert not np.array_equal(base, draw_slices(4, 10, 2, 200, 100)), "views must differ"
    assert not np.array_equal(base, draw_slices(5, 10, 1, 200, 100)), "seeds must differ"
    assert np.array_equal(draw_slices(4, 10, 1, 9, 9), np.arange(9))


def test_constructor_refusals():
    from synthanatomy_amd.losses import lpips, vqvae
    w = lpips.load_weights("random:0")
    for cls in (vqvae.PerceptualLoss, vqvae.JukeboxPerceptualLoss, vqvae.HartleyPerceptualLoss):
        with pytest.raises(NotImplementedError, match="dimensions"):
            cls(dimensions=2, perceptual_weights=w)
        with pytest.raises(NotImplementedError, match="is_fake_3d"):
            cls(dimensions=3, is_fake_3d=False, perceptual_weights=w)
        for kw in ({"net": "vgg"}, {"spatial": True}, {"version": "0.0"}, {"pnet_tune": True}, {"lpips": False}):
            with pytest.raises(NotImplementedError, match="lpips_kwargs"):
                cls(dimensions=3, lpips_kwargs=kw, perceptual_weights=w)
        cls(dimensions=3, lpips_kwargs={"net": "alex", "verbose": True}, perceptual_weights=w)
        for bad in (-0.1, 1.0, 1.5):
            with pytest.raises(ValueError, match="drop_ratio"):
                cls(dimensions=3, drop_ratio=bad, perceptual_weights=w)
        with pytest.raises(ValueError, match="perceptual_weights"):
            cls(dimensions=3)


def test_forward_refusals_come_before_any_launch():
    """every one is raised on the host: this machine has no GPU, so reaching a launch would raise HipLibraryError instead"""
    from synthanatomy_amd.losses import lpips, vqvae
    w = lpips.load_weights("random:0")

    def call(fn, shape):
        x = torch.rand(shape)
        return fn({"reconstruction": [x], "quantization_losses": []}, x)

    fn = vqvae.PerceptualLoss(dimensions=3, perceptual_weights=w)
    with pytest.raises(NotImplementedError, match="C = 1"):
        call(fn, (1, 2, 31, 31, 31))
    with pytest.raises(ValueError, match="side"):
        call(fn, (1, 1, 30, 40, 40))
    with pytest.raises(ValueError, match="side"):
        call(fn, (1, 1, 40, 40, 30))
    call_ok = vqvae.PerceptualLoss(dimensions=3, perceptual_weights=w, fake_3d_axis=(2,))
    with pytest.raises(ValueError, match="side"):
        call(call_ok, (1, 1, 40, 30, 40))
    with pytest.raises(ValueError, match="drop_ratio.*keeps 0"):
        call(vqvae.JukeboxPerceptualLoss(dimensions=3, drop_ratio=0.99, perceptual_weights=w), (1, 1, 31, 31, 31))


def test_weight_files_round_trip_and_are_refused_by_name(tmp_path):
    from synthanatomy_amd.losses import lpips
    sd = lpips.random_state_dict(2)
    path = str(tmp_path / "alex.pth")
    torch.save(dict(sd, **{"scaling_layer.shift": torch.tensor(lpips.SHIFT).view(1, 3, 1, 1), "scaling_layer.scale": torch.tensor(lpips.SCALE).view(1, 3, 1, 1)}), path)
    got = lpips.load_weights(path)
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    assert torch.allclose(got["scaling_layer.shift"], torch.tensor(lpips.SHIFT, dtype=torch.float64))
    missing = {k: v for k, v in sd.items() if k != "lin3.model.1.weight"}
    torch.save(missing, path)
    with pytest.raises(ValueError, match=r"perceptual_weights.*'lin3\.model\.1\.weight' is missing"):
        lpips.load_weights(path)
    torch.save(dict(sd, **{"net.slice2.3.weight": torch.zeros(192, 64, 3, 3)}), path)
    with pytest.raises(ValueError, match=r"perceptual_weights.*'net\.slice2\.3\.weight' has shape \(192, 64, 3, 3\)"):
        lpips.load_weights(path)
    with pytest.raises(ValueError, match="perceptual_weights.*no such file"):
        lpips.load_weights(str(tmp_path / "absent.pth"))
    with open(path, "wb") as f:
        f.write(b"not a checkpoint")
    with pytest.raises(ValueError, match="perceptual_weights.*cannot be read"):
        lpips.load_weights(path)
    with pytest.raises(ValueError, match="perceptual_weights.*seed"):
        lpips.load_weights("random:abc")


def test_cli_checks_the_flag_before_the_device(tmp_path):
    """run_vqvae.run refuses before init_distributed / any device use (there is no GPU here: getting further would fail differently)"""
    import run_vqvae
    base = ["--project_directory=" + str(tmp_path) + "/", "--experiment_name=e", "--training_subjects=synthetic:2", "--validation_subjects=synthetic:1",
            "--mode=training", "--loss=jukebox_perceptual"]
    with pytest.raises(ValueError, match="--loss=jukebox_perceptual needs --perceptual_weights"):
        run_vqvae.run(base)
    with pytest.raises(ValueError, match="--perceptual_weights.*no such file"):
        run_vqvae.run(base + ["--perceptual_weights=" + str(tmp_path / "none.pth")])
    bad = str(tmp_path / "bad.pth")
    from synthanatomy_amd.losses import lpips
    sd = lpips.random_state_dict(0)
    del sd["net.slice5.10.bias"]
    torch.save(sd, bad)
    with pytest.raises(ValueError, match=r"'net\.slice5\.10\.bias' is missing"):
        run_vqvae.run(base + ["--perceptual_weights=" + bad])


def test_merging_tool_on_synthetic_files(tmp_path):
    from synthanatomy_amd.losses import lpips
    sd = lpips.random_state_dict(6)
    feat_idx = (0, 3, 6, 8, 10)
    alexnet = {f"features.{i}.{p}": sd[f"{key}.{p}"] for i, key in zip(feat_idx, lpips.CONV_KEYS) for p in ("weight", "bias")}
    alexnet.update({"classifier.1.weight": torch.zeros(4, 4), "classifier.1.bias": torch.zeros(4)})
    lins = {k: sd[k] for k in lpips.LIN_KEYS}
    a, b, out = (str(tmp_path / n) for n in ("alexnet-owt-test.pth", "alex.pth", "merged.pth"))
    torch.save(alexnet, a)
    torch.save(lins, b)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_lpips_weights.py"), "--alexnet", a, "--lpips", b, "--out", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = lpips.load_weights(out)
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    del alexnet["features.8.bias"]
    torch.save(alexnet, a)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_lpips_weights.py"), "--alexnet", a, "--lpips", b, "--out", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "features.8.bias" in r.stderr


@functools.lru_cache(maxsize=None)
def _witness_base():
    gold = _golden()
    y, pred, _ = _inputs("small")
    sd = lpips_ref.draw_weights(int(gold["seed"]))
    return y, pred, sd, _term(y, pred, sd, None)


def _term(y, pred, sd, defect):
    p = pred.double().requires_grad_(True)
    total = sum(lpips_ref.perceptual_terms(p, y, sd, defect=defect))
    total.backward()
    return float(total), p.grad.clone()


@pytest.mark.parametrize("defect", lpips_ref.DEFECTS)
def test_planted_defect_moves_the_golden_case_beyond_the_gpu_tolerance(defect):
    """if a defect stays inside the tolerance, the GPU tolerance cannot see it: the test fails"""
    y, pred, sd, (loss, grad) = _witness_base()
    wl, wg = _term(y, pred, sd, defect)
    dl, dg = abs(wl - loss) / abs(loss), float((wg - grad).abs().max() / grad.abs().max())
    print(f"[{defect}] loss moves by {dl:.2e} of |ref|, gradient by {dg:.2e} of max|ref| (GPU tolerance {GPU_TOL:g})")
    assert dl > GPU_TOL or dg > GPU_TOL
