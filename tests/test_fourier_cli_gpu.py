"""GPU: ``run_vqvae.py --loss=spectral | hartley | wavegan`` on the tiny configuration of test_baur_cli_gpu.py -- the loss is finite and a checkpoint
is written on the plain and on the adversarial path (adaptive weight on), and a resumed run equals an uninterrupted one."""
import glob
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

LOSSES = ("spectral", "hartley", "wavegan")


def _flags(proj, exp, loss, extra=()):
    return ["--project_directory=" + proj, "--experiment_name=" + exp, "--no_levels=2", "--downsample_parameters=((4,2,1,1),(4,2,1,1))",
            "--upsample_parameters=((4,2,1,0,1),(4,2,1,0,1))", "--no_channels=32", "--num_embeddings=(64,)", "--embedding_dim=(16,)", "--decay=(0.5,)",
            "--roi=((0,32),(0,32),(0,32))", "--batch_size=2", "--eval_batch_size=2", "--learning_rate=1e-3", "--gamma=0.9", "--amp=False",
            "--training_subjects=synthetic:4", "--validation_subjects=synthetic:2", "--mode=training", "--eval_every=1", "--loss=" + loss, *extra]


def _losses(out):
    """{epoch: [logged loss of each iteration]}"""
    got = {}
    for m in re.finditer(r"^epoch (\d+) it \d+ loss (\S+)", out, flags=re.M):
        got.setdefault(int(m.group(1)), []).append(float(m.group(2)))
    return got


def _ckpt(proj, exp, epoch):
    return glob.glob(f"{proj}{exp}/baseline_vqvae/checkpoints/checkpoint_epoch={epoch}.pt")


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("adversarial", [False, True])
def test_trains_and_checkpoints(tmp_path, capsys, loss, adversarial):
    import run_vqvae
    proj = str(tmp_path) + "/"
    extra = ["--adversarial_component=True", "--use_adversarial_adaptive_weight=True"] if adversarial else []
    run_vqvae.run(_flags(proj, "run", loss, extra) + ["--epochs=2"])
    out = capsys.readouterr().out
    got = _losses(out)
    assert sorted(got) == [0, 1] and all(len(v) == 2 for v in got.values())
    assert all(torch.isfinite(torch.tensor(v)).all() for v in got.values()), got
    if adversarial:
        assert len(re.findall(r"g_loss \S+ d_loss \S+ adv_weight \S+", out)) == 4
    assert _ckpt(proj, "run", 2)


@pytest.mark.parametrize("loss", LOSSES)
def test_resume_equals_uninterrupted(tmp_path, capsys, loss):
    """With --deterministic (fixed-order reductions): the spectral loss's phase term is discontinuous, so summation-order noise in the weights can
    flip spectrum bins across the negative real axis and move the loss by whole percent within an epoch."""
    import run_vqvae
    proj = str(tmp_path) + "/"
    det = ["--deterministic=True"]
    run_vqvae.run(_flags(proj, "full", loss, det) + ["--epochs=2"])
    full_log = _losses(capsys.readouterr().out)
    run_vqvae.run(_flags(proj, "split", loss, det) + ["--epochs=1"])
    run_vqvae.run(_flags(proj, "split", loss, det) + ["--epochs=2"])      # finds checkpoint_epoch=1 and resumes at epoch 1
    split_log = _losses(capsys.readouterr().out)
    assert sorted(full_log) == sorted(split_log) == [0, 1]
    for e in (0, 1):
        assert split_log[e] == pytest.approx(full_log[e], rel=1e-4), e
    a = torch.load(_ckpt(proj, "full", 2)[0], map_location="cpu", weights_only=False)
    b = torch.load(_ckpt(proj, "split", 2)[0], map_location="cpu", weights_only=False)
    assert a["trainer"] == b["trainer"] and a["lr_scheduler"] == b["lr_scheduler"]
    for k in a["network"]:      # (the same gates as test_baur_cli_gpu.py: fp32 atomics' summation order only)
        if a["network"][k].is_floating_point():
            assert _rel(a["network"][k], b["network"][k]) < 1e-4, k
        else:
            assert torch.equal(a["network"][k], b["network"][k]), k
