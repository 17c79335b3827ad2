"""CPU: the host side of ``--loss=baseline`` (BaselineLoss: L1 + five-axis FFT amplitude + three-plane LPIPS-squeeze): the fp64
restatement of tests/squeeze_ref.py against the fixture made from the reference's own class, the factory, the weight checks and the merging tool, the
first-layer fold, the merged expand, the ceil-mode extents, ``lpips_kwargs net='squeeze'``, and the witnesses -- each planted defect of squeeze_ref must move
the golden case far outside the tolerance the GPU tests grant."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref
import squeeze_ref
from conftest import ROOT

torch.set_num_threads(min(16, torch.get_num_threads()))
GPU_TOL = 1e-3      # tests/test_baseline_loss_gpu.py, fp32 mode
SUMMARY_KEYS = ("Loss-MAE-Reconstruction", "Loss-Jukebox-Reconstruction", "Loss-Perceptual_Sagittal-Reconstruction", "Loss-Perceptual_Axial-Reconstruction",
                "Loss-Perceptual_Coronal-Reconstruction", "Loss-Perceptual-Reconstruction")


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "losses_baseline.npz"))


def _inputs(sname):
    gold = _golden()
    return (torch.from_numpy(gold[f"input/{sname}/y_u8"]).float() / 255, torch.from_numpy(gold[f"input/{sname}/pred_u8"]).float() / 255,
            torch.from_numpy(gold[f"input/{sname}/qloss"]))


@pytest.mark.parametrize("sname", ["small", "background"])
def test_restatement_matches_the_reference_fixture(sname):
    gold = _golden()
    y, pred, q = _inputs(sname)
    assert y.shape[0] == 2, "B = 2: the frequency term's batch-axis transform must be exercised"
    sd = squeeze_ref.draw_weights(int(gold["seed"]))
    p = pred.double().requires_grad_(True)
    loss, summ = squeeze_ref.baseline_loss(p, y, q, sd)
    loss.backward()
    c = f"case/{sname}/"
    assert abs(float(loss.detach()) - float(gold[c + "loss"])) <= 1e-10
    keys = [k[len(c):] for k in gold.files if k.startswith(c) and k[len(c):] not in ("loss", "dpred_strided")]
    assert sorted(keys) == sorted(summ) == sorted(SUMMARY_KEYS), (keys, sorted(summ))
    for k in keys:
        assert abs(float(summ[k].detach()) - float(gold[c + k])) <= 1e-10, k
    assert float((p.grad.reshape(-1)[::8] - torch.from_numpy(gold[c + "dpred_strided"])).abs().max()) <= 1e-10


def test_factory_builds_baseline_with_upstream_attributes():
    from synthanatomy_amd.losses import vqvae
    assert "baseline" in vqvae.VQVAE_LOSSES and len(vqvae.VQVAE_LOSSES) == 10
    fn = vqvae.get_vqvae_loss({"loss": "baseline", "perceptual_weights": "random:0"})
    assert type(fn) is vqvae.BaselineLoss
    assert fn.pixel_factor == 1.0 and fn.perceptual_factor == 0.002 and fn.n_slices == 512 and fn.fft_factor == 1.0
    fn.pixel_factor, fn.perceptual_factor, fn.n_slices, fn.fft_factor = 0.5, 0.01, 7, 2.0       # plain settable attributes, as upstream
    assert (fn.pixel_factor, fn.perceptual_factor, fn.n_slices, fn.fft_factor) == (0.5, 0.01, 7, 2.0)
    assert not list(fn.parameters()) and not fn.state_dict(), "the frozen weights must be non-persistent buffers"
    assert len(list(fn.buffers())) >= 2 + 4 * 8 + 7
    assert fn.set_step(7) == 7 and fn.get_summaries() == {"scalar": {}}
    assert fn.perceptual_function.compute_dtype == torch.float32
    assert vqvae.get_vqvae_loss({"loss": "baseline", "perceptual_weights": "random:0", "amp": True}).perceptual_function.compute_dtype == torch.bfloat16


def test_factory_without_weights_still_raises():
    from synthanatomy_amd.losses import vqvae
    with pytest.raises(ValueError, match="Loss function unknown.*--perceptual_weights"):
        vqvae.get_vqvae_loss({"loss": "baseline"})
    with pytest.raises(ValueError, match="perceptual_weights is required"):
        vqvae.BaselineLoss()


def test_package_squeeze_draws_equal_the_restated_ones():
    from synthanatomy_amd.losses import lpips, lpips_squeeze
    a, b = lpips_squeeze.random_state_dict(3), squeeze_ref.draw_weights(3)
    assert sorted(a) == sorted(b) and len(a) == 2 + 6 * 8 + 7 and all(torch.equal(a[k], b[k]) for k in a)
    assert all(float(a[k].min()) >= 0 for k in lpips_squeeze.LIN_KEYS)
    assert lpips_squeeze.expected_shapes() == squeeze_ref.shapes()
    got = lpips.load_weights("random:3", net="squeeze")
    assert all(torch.equal(got[k], b[k]) for k in b)
    # the alex draws keep their results (pinned by test_perceptual_losses_cpu.py too)
    c, d = lpips.random_state_dict(3), lpips_ref.draw_weights(3)
    assert all(torch.equal(c[k], d[k]) for k in d)


def test_weight_files_are_checked_by_key_shape_and_network(tmp_path):
    from synthanatomy_amd.losses import lpips, lpips_squeeze, vqvae
    sd = lpips_squeeze.random_state_dict(2)
    path = str(tmp_path / "squeeze.pth")
    torch.save(sd, path)
    got = lpips.load_weights(path, net="squeeze")
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    assert torch.allclose(got["scaling_layer.shift"], torch.tensor(lpips.SHIFT, dtype=torch.float64))
    torch.save({k: v for k, v in sd.items() if k != "net.slice5.10.expand3x3.bias"}, path)
    with pytest.raises(ValueError, match=r"perceptual_weights.*'net\.slice5\.10\.expand3x3\.bias' is missing"):
        lpips.load_weights(path, net="squeeze")
    torch.save(dict(sd, **{"net.slice4.9.squeeze.weight": torch.zeros(48, 256, 3, 3)}), path)
    with pytest.raises(ValueError, match=r"perceptual_weights.*'net\.slice4\.9\.squeeze\.weight' has shape \(48, 256, 3, 3\)"):
        lpips.load_weights(path, net="squeeze")
    alex = str(tmp_path / "alex.pth")
    torch.save(lpips.random_state_dict(0), alex)
    with pytest.raises(ValueError, match="perceptual_weights.*LPIPS-alex file"):
        lpips.load_weights(alex, net="squeeze")
    with pytest.raises(ValueError, match="LPIPS-alex file"):
        vqvae.get_vqvae_loss({"loss": "baseline", "perceptual_weights": alex})
    torch.save(sd, path)
    with pytest.raises(ValueError, match="perceptual_weights.*LPIPS-squeeze file"):
        lpips.load_weights(path)
    with pytest.raises(ValueError, match="LPIPS-squeeze file"):
        vqvae.get_vqvae_loss({"loss": "perceptual", "perceptual_weights": path})
    with pytest.raises(ValueError, match="LPIPS-squeeze layout"):
        vqvae.PerceptualLoss(dimensions=3, perceptual_weights=lpips.load_weights(path, net="squeeze"))


def test_cli_checks_the_flag_before_the_device(tmp_path):
    """run_vqvae.run refuses before init_distributed / any device use (there is no GPU here: getting further would fail differently)"""
    import run_vqvae
    from synthanatomy_amd.losses import lpips
    base = ["--project_directory=" + str(tmp_path) + "/", "--experiment_name=e", "--training_subjects=synthetic:2", "--validation_subjects=synthetic:1",
            "--mode=training", "--loss=baseline"]
    with pytest.raises(ValueError, match="--loss=baseline needs --perceptual_weights.*squeeze"):
        run_vqvae.run(base)
    with pytest.raises(ValueError, match="--perceptual_weights.*no such file"):
        run_vqvae.run(base + ["--perceptual_weights=" + str(tmp_path / "none.pth")])
    alex = str(tmp_path / "alex.pth")
    torch.save(lpips.random_state_dict(0), alex)
    with pytest.raises(ValueError, match="LPIPS-alex file"):
        run_vqvae.run(base + ["--perceptual_weights=" + alex])


def test_first_layer_fold_reproduces_the_scaled_three_channel_convolution():
    from synthanatomy_amd.losses import lpips_squeeze
    sd = squeeze_ref.draw_weights(4)
    w, b = sd["net.slice1.0.weight"].double(), sd["net.slice1.0.bias"].double()
    shift, scale = torch.tensor(lpips_ref.SHIFT, dtype=torch.float64), torch.tensor(lpips_ref.SCALE, dtype=torch.float64)
    wf, bf = lpips_squeeze.folded_conv1(w, b, shift, scale)
    assert wf.shape == (64, 9) and bf.shape == (64,) and wf.dtype == torch.float64
    u = torch.rand(3, 1, 18, 23, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 2 - 1
    want = F.conv2d((u - shift.view(1, 3, 1, 1)) / scale.view(1, 3, 1, 1), w, b, stride=2)
    got = F.conv2d(u, wf.view(64, 1, 3, 3), bf, stride=2)
    assert want.shape[2:] == (lpips_squeeze.conv1_extent(18), lpips_squeeze.conv1_extent(23))
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_merged_expand_equals_the_concatenation():
    from synthanatomy_amd.losses import lpips_squeeze
    g = torch.Generator().manual_seed(2)
    w1, b1 = torch.randn(5, 4, 1, 1, generator=g, dtype=torch.float64), torch.randn(5, generator=g, dtype=torch.float64)
    w3, b3 = torch.randn(6, 4, 3, 3, generator=g, dtype=torch.float64), torch.randn(6, generator=g, dtype=torch.float64)
    z = torch.randn(2, 4, 7, 6, generator=g, dtype=torch.float64)
    wm, bm = lpips_squeeze.merged_expand(w1, b1, w3, b3)
    want = torch.cat([F.conv2d(z, w1, b1), F.conv2d(z, w3, b3, padding=1)], 1)
    assert float((F.conv2d(z, wm, bm, padding=1) - want).abs().max()) <= 1e-14


def test_extents_agree_with_torch_and_side_16_is_refused():
    from synthanatomy_amd.losses import lpips_squeeze
    for e in range(17, 49):
        x = torch.zeros(1, 1, e, e)
        want = []
        x = F.conv2d(x, torch.zeros(1, 1, 3, 3), stride=2)
        want.append(x.shape[-1])
        for _ in range(3):
            x = F.max_pool2d(x, 3, 2, ceil_mode=True)
            want.append(x.shape[-1])
        assert lpips_squeeze.extents(e) == tuple(want), e
    assert lpips_squeeze.extents(17) == (8, 4, 2, 1) and lpips_squeeze.MIN_SIDE == 17
    with pytest.raises(ValueError, match="side 16.*>= 17"):
        lpips_squeeze.extents(16)
    with pytest.raises(RuntimeError):       # torch itself: the third pool of a 16-pixel side has no output
        x = F.conv2d(torch.zeros(1, 1, 16, 16), torch.zeros(1, 1, 3, 3), stride=2)
        for _ in range(3):
            x = F.max_pool2d(x, 3, 2, ceil_mode=True)
    fn = _baseline()
    x = torch.rand(1, 1, 16, 20, 20)
    with pytest.raises(ValueError, match="side.*>= 17"):       # on the host: reaching a launch without a GPU would raise HipLibraryError instead
        fn({"reconstruction": [x], "quantization_losses": []}, x)
    with pytest.raises(NotImplementedError, match="C = 1"):
        fn({"reconstruction": [torch.rand(1, 2, 20, 20, 20)], "quantization_losses": []}, torch.rand(1, 2, 20, 20, 20))


def _baseline():
    from synthanatomy_amd.losses import vqvae
    return vqvae.get_vqvae_loss({"loss": "baseline", "perceptual_weights": "random:0"})


def test_perceptual_classes_accept_net_squeeze():
    from synthanatomy_amd.losses import lpips, lpips_squeeze, vqvae
    w = lpips.load_weights("random:0", net="squeeze")
    for cls in (vqvae.PerceptualLoss, vqvae.JukeboxPerceptualLoss, vqvae.HartleyPerceptualLoss):
        fn = cls(dimensions=3, lpips_kwargs={"net": "squeeze", "verbose": False}, perceptual_weights=w)
        assert isinstance(fn.perceptual_function, lpips_squeeze.LpipsSqueeze) and fn.lpips_kwargs["net"] == "squeeze"
        assert not list(fn.parameters()) and not fn.state_dict()
        with pytest.raises(NotImplementedError, match="lpips_kwargs"):
            cls(dimensions=3, lpips_kwargs={"net": "vgg"}, perceptual_weights=w)
        with pytest.raises(NotImplementedError, match="lpips_kwargs"):
            cls(dimensions=3, lpips_kwargs={"net": "squeeze", "spatial": True}, perceptual_weights=w)
        with pytest.raises(ValueError, match="net='squeeze' needs perceptual_weights"):
            cls(dimensions=3, lpips_kwargs={"net": "squeeze"}, perceptual_weights=lpips.load_weights("random:0"))
        x = torch.rand(1, 1, 16, 20, 20)
        with pytest.raises(ValueError, match="side"):
            fn({"reconstruction": [x], "quantization_losses": []}, x)
    assert isinstance(vqvae.PerceptualLoss(dimensions=3, perceptual_weights=lpips.load_weights("random:0")).perceptual_function, lpips.LpipsAlex)


def test_merging_tool_on_synthetic_squeeze_files(tmp_path):
    from synthanatomy_amd.losses import lpips, lpips_squeeze
    sd = lpips_squeeze.random_state_dict(6)
    backbone = {"features.0.weight": sd["net.slice1.0.weight"], "features.0.bias": sd["net.slice1.0.bias"],
                "classifier.1.weight": torch.zeros(4, 4, 1, 1), "classifier.1.bias": torch.zeros(4)}
    for feat, key, *_ in lpips_squeeze.FIRES:
        for part in ("squeeze", "expand1x1", "expand3x3"):
            for p in ("weight", "bias"):
                backbone[f"features.{feat}.{part}.{p}"] = sd[f"{key}.{part}.{p}"]
    lins = {k: sd[k] for k in lpips_squeeze.LIN_KEYS}
    a, b, out = (str(tmp_path / n) for n in ("squeezenet1_1-test.pth", "squeeze.pth", "merged.pth"))
    torch.save(backbone, a)
    torch.save(lins, b)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "make_lpips_weights.py"), "--net=squeeze", "--backbone", a, "--lpips", b, "--out", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = lpips.load_weights(out, net="squeeze")
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    del backbone["features.9.expand1x1.bias"]
    torch.save(backbone, a)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "features.9.expand1x1.bias" in r.stderr


@functools.lru_cache(maxsize=None)
def _witness_base():
    gold = _golden()
    y, pred, _ = _inputs("small")
    sd = squeeze_ref.draw_weights(int(gold["seed"]))
    return y, pred, sd, _term(y, pred, sd, None)


def _term(y, pred, sd, defect):
    p = pred.double().requires_grad_(True)
    total = sum(squeeze_ref.perceptual_means(p, y, sd, defect=defect))
    total.backward()
    return float(total), p.grad.clone()


@pytest.mark.parametrize("defect", squeeze_ref.DEFECTS)
def test_planted_defect_moves_the_golden_case_far_beyond_the_gpu_tolerance(defect):
    """if a defect stays near the tolerance, the GPU tolerance cannot see it: the test fails.  (Exchanging axial and coronal leaves the SUM of the three
    means unchanged -- it is a defect of the summaries -- so that witness compares the per-view means under their keys.)"""
    y, pred, sd, (loss, grad) = _witness_base()
    if defect == "swap_axial_coronal":
        good = squeeze_ref.perceptual_means(pred.double(), y, sd)
        bad = squeeze_ref.perceptual_means(pred.double(), y, sd, defect=defect)
        d = max(abs(float(a) - float(b)) / abs(float(a)) for a, b in zip(good[1:], bad[1:]))
        print(f"[{defect}] the axial / coronal means move by {d:.2e} of |ref| (GPU tolerance {GPU_TOL:g})")
        assert float(good[0]) == float(bad[0]) and d > 10 * GPU_TOL
        return
    if defect == "floor_pool":
        # (the golden case's 17-pixel sides leave floor-mode pools without an output -- there the defect is a crash; the witness for the arithmetic takes
        # the smallest sides at which three floor-mode pools still have one: 33 -> 16 -> 7, 3, 1 against ceil's 8, 4, 2)
        g = torch.Generator().manual_seed(12)
        y = torch.rand((1, 1, 33, 34, 35), generator=g)
        pred = (y + 0.1 * torch.randn(y.shape, generator=g)).clamp(0, 1)
        loss, grad = _term(y, pred, sd, None)
    wl, wg = _term(y, pred, sd, defect)
    dl, dg = abs(wl - loss) / abs(loss), float((wg - grad).abs().max() / grad.abs().max())
    print(f"[{defect}] loss moves by {dl:.2e} of |ref|, gradient by {dg:.2e} of max|ref| (GPU tolerance {GPU_TOL:g})")
    assert dl > 10 * GPU_TOL or dg > 10 * GPU_TOL
