"""GPU: ``run_vqvae.py --loss=baur`` -- the gdl_factor follows the reference's epoch-level schedule (0.0 during the first epoch, then
``ParamSchedulerHandler._linear`` of the finished epochs), a resumed run equals an uninterrupted one, and the adversarial path trains with it."""
import glob
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

FACTOR_FLAGS = ["--initial_factor_value=0.5", "--initial_factor_steps=1", "--max_factor_steps=2", "--max_factor_value=3"]


def _flags(proj, exp, extra=()):
    return ["--project_directory=" + proj, "--experiment_name=" + exp, "--no_levels=2", "--downsample_parameters=((4,2,1,1),(4,2,1,1))",
            "--upsample_parameters=((4,2,1,0,1),(4,2,1,0,1))", "--no_channels=32", "--num_embeddings=(64,)", "--embedding_dim=(16,)", "--decay=(0.5,)",
            "--roi=((0,32),(0,32),(0,32))", "--batch_size=2", "--eval_batch_size=2", "--learning_rate=1e-3", "--gamma=0.9", "--amp=False",
            "--training_subjects=synthetic:4", "--validation_subjects=synthetic:2", "--mode=training", "--eval_every=1", "--loss=baur",
            *FACTOR_FLAGS, *extra]


def _factors(out):
    """{epoch: [gdl_factor of each logged iteration]}"""
    got = {}
    for m in re.finditer(r"^epoch (\d+) it \d+ loss (\S+) .*gdl_factor (\S+)", out, flags=re.M):
        assert torch.isfinite(torch.tensor(float(m.group(2))))
        got.setdefault(int(m.group(1)), []).append(float(m.group(3)))
    return got


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def test_logged_factor_follows_the_schedule(tmp_path, capsys):
    import run_vqvae
    from synthanatomy_amd.losses.vqvae import gdl_factor_schedule
    run_vqvae.run(_flags(str(tmp_path) + "/", "sched") + ["--epochs=3"])
    got = _factors(capsys.readouterr().out)
    cfg = {"initial_factor_value": 0.5, "initial_factor_steps": 1, "max_factor_steps": 2, "max_factor_value": 3}
    want = {0: 0.0, 1: gdl_factor_schedule(cfg, 1), 2: gdl_factor_schedule(cfg, 2)}
    assert want == {0: 0.0, 1: 0.5, 2: 1.75}
    assert sorted(got) == [0, 1, 2]
    for e, vals in got.items():
        assert len(vals) == 2 and all(v == pytest.approx(want[e]) for v in vals), (e, vals)


def test_resume_equals_uninterrupted(tmp_path, capsys):
    import run_vqvae
    proj = str(tmp_path) + "/"
    run_vqvae.run(_flags(proj, "full") + ["--epochs=2"])
    full_log = _factors(capsys.readouterr().out)
    run_vqvae.run(_flags(proj, "split") + ["--epochs=1"])
    run_vqvae.run(_flags(proj, "split") + ["--epochs=2"])      # finds checkpoint_epoch=1 and resumes at epoch 1
    split_log = _factors(capsys.readouterr().out)
    assert full_log == split_log == {0: [0.0, 0.0], 1: [0.5, 0.5]}
    a = torch.load(glob.glob(proj + "full/baseline_vqvae/checkpoints/checkpoint_epoch=2.pt")[0], map_location="cpu", weights_only=False)
    b = torch.load(glob.glob(proj + "split/baseline_vqvae/checkpoints/checkpoint_epoch=2.pt")[0], map_location="cpu", weights_only=False)
    assert a["trainer"] == b["trainer"] and a["lr_scheduler"] == b["lr_scheduler"]
    for k in a["network"]:      # (the same gates as tests/test_training_gpu.py's plain resume case: fp32 atomics' summation order only)
        if a["network"][k].is_floating_point():
            assert _rel(a["network"][k], b["network"][k]) < 1e-4, k
        else:
            assert torch.equal(a["network"][k], b["network"][k]), k
    assert a["optimizer"]["param_groups"] == b["optimizer"]["param_groups"]
    for i, ent in a["optimizer"]["state"].items():
        assert float(ent["step"]) == 4.0 == float(b["optimizer"]["state"][i]["step"])
        assert _rel(ent["exp_avg"], b["optimizer"]["state"][i]["exp_avg"]) < 1e-3 and _rel(ent["exp_avg_sq"], b["optimizer"]["state"][i]["exp_avg_sq"]) < 1e-3, i


def test_adversarial_component_trains_with_baur(tmp_path, capsys):
    import run_vqvae
    run_vqvae.run(_flags(str(tmp_path) + "/", "adv", ["--adversarial_component=True", "--use_adversarial_adaptive_weight=True"]) + ["--epochs=2"])
    out = capsys.readouterr().out
    got = _factors(out)
    assert got == {0: [0.0, 0.0], 1: [0.5, 0.5]}
    assert len(re.findall(r"g_loss \S+ d_loss \S+ adv_weight \S+ gdl_factor", out)) == 4
    assert glob.glob(str(tmp_path) + "/adv/baseline_vqvae/checkpoints/checkpoint_epoch=2.pt")
