"""GPU: ``run_vqvae.py`` at a 48^3 roi keeps its best checkpoint by the reference's key metric, Metric-MS-SSIM_3-Reconstruction (higher is better,
``checkpoint_key_metric=<v>.pt`` with 0 <= v <= 1), logs it with MAE and MSE, and ``--evaluation_checkpoint=best`` loads that checkpoint."""
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

import ms_ssim_ref as R

pytestmark = pytest.mark.gpu


def _flags(proj, exp, extra=()):
    return ["--project_directory=" + proj, "--experiment_name=" + exp, "--no_levels=2", "--downsample_parameters=((4,2,1,1),(4,2,1,1))",
            "--upsample_parameters=((4,2,1,0,1),(4,2,1,0,1))", "--no_channels=32", "--num_embeddings=(64,)", "--embedding_dim=(16,)", "--decay=(0.5,)",
            "--roi=((0,48),(0,48),(0,48))", "--batch_size=2", "--eval_batch_size=2", "--learning_rate=1e-3", "--gamma=0.9", "--amp=False",
            "--training_subjects=synthetic:4", "--validation_subjects=synthetic:3", *extra]


def test_key_metric_is_ms_ssim_and_best_loads_it(tmp_path, capsys):
    import run_vqvae
    from synthanatomy_amd.utils.general import load_network_state, parse_flags
    proj = str(tmp_path) + "/"
    run_vqvae.run(_flags(proj, "ms", ["--mode=training", "--epochs=2", "--eval_every=1"]))
    out = capsys.readouterr().out
    lines = re.findall(r"^epoch (\d+) validation Metric-MS-SSIM_3-Reconstruction (\S+) Metric-MAE-Reconstruction (\S+) "
                       r"Metric-MSE-Reconstruction (\S+)$", out, flags=re.M)
    assert [int(e) for e, *_ in lines] == [0, 1], out
    mses = [float(m) for m in re.findall(r"^epoch \d+ validation mse (\S+)$", out, flags=re.M)]
    assert len(mses) == 2
    for (_, ms, mae, mse), m in zip(lines, mses):
        assert 0.0 <= float(ms) <= 1.0 and float(mae) > 0 and float(mse) == pytest.approx(m, abs=2e-6)
    ck = proj + "ms/baseline_vqvae/checkpoints/"
    best = glob.glob(ck + "checkpoint_key_metric=*.pt")
    assert len(best) == 1
    v = float(re.search(r"key_metric=([0-9.]+)\.pt$", best[0]).group(1))
    assert 0.0 <= v <= 1.0
    side = json.load(open(ck + "checkpoint_key_metric.json"))
    assert side["file"] == os.path.basename(best[0]) and side["name"] == "Metric-MS-SSIM_3-Reconstruction"
    logged = [float(ms) for _, ms, _, _ in lines]
    assert f"{side['score']:.6f}" == f"{max(logged):.6f}" and f"{side['score']:.4f}" == f"{v:.4f}"

    # the checkpoint's network on the validation volumes, MS-SSIM by the fp64 restatement
    cfg = parse_flags(_flags(proj, "ms", ["--mode=training"]), run_vqvae.DEFAULTS)
    dev = torch.device("cuda", 0)
    net = run_vqvae.build_network(cfg, dev).eval()
    load_network_state(net, best[0])
    ref, tv = [], []
    with torch.no_grad():
        for name in ("synthetic_0000", "synthetic_0001", "synthetic_0002"):
            x = run_vqvae._load_volume(name, cfg, None, dev)[None]
            rec = net(x)["reconstruction"][0].float()
            ref.append(R.ms_ssim(x.double().cpu().numpy(), rec.double().cpu().numpy(), win_size=3)[0])
            tv.append(R.torch_ms_ssim(x, rec, win_size=3)[0].item())
    ref, tv = float(np.mean(ref)), float(np.mean(tv))
    assert abs(side["score"] - ref) <= max(2 * abs(tv - ref), 1e-5), (side["score"], ref, tv)

    run_vqvae.run(_flags(proj, "ms", ["--mode=extracting", "--evaluation_checkpoint=best"]))
    out = capsys.readouterr().out
    assert f"loaded {best[0]}" in out
