"""GPU: ``run_vqvae.py --mode=training --codebook_restart_patience --codebook_restart_max --decay_warmup=linear`` -- the log line carries the restarts and the
decay of every finished epoch, the checkpoint has the ``codebook_restart`` entry, and a resumed run continues with the restarts of an uninterrupted one
(``--deterministic=True``: the runs are then bit-reproducible, so "the same" is exact)."""
import glob
import re

import pytest
import torch

pytestmark = pytest.mark.gpu


def _flags(proj, exp, extra=()):
    return ["--project_directory=" + proj, "--experiment_name=" + exp, "--no_levels=2", "--downsample_parameters=((4,2,1,1),(4,2,1,1))",
            "--upsample_parameters=((4,2,1,0,1),(4,2,1,0,1))", "--no_channels=32", "--num_embeddings=(64,)", "--embedding_dim=(16,)", "--decay=(0.5,)",
            "--roi=((0,32),(0,32),(0,32))", "--batch_size=2", "--eval_batch_size=2", "--learning_rate=1e-3", "--gamma=0.9", "--amp=False",
            "--training_subjects=synthetic:4", "--validation_subjects=synthetic:2", "--mode=training", "--eval_every=100", "--deterministic=True",
            "--codebook_restart_patience=1", "--codebook_restart_max=4", "--decay_warmup=linear", "--max_decay_epochs=4", *extra]


def _restarts(out):
    """[(epoch, iteration, dead, restarted)] of every logged iteration"""
    return [tuple(int(v) for v in m.groups()) for m in re.finditer(r"^epoch (\d+) it (\d+) loss \S+ .*codebook_dead (\d+) restarted (\d+) perplexity", out, flags=re.M)]


def _decays(out):
    return {int(m.group(1)): float(m.group(2)) for m in re.finditer(r"^epoch (\d+) decay (\S+)$", out, flags=re.M)}


def _checkpoint(proj, exp, epoch):
    return torch.load(glob.glob(f"{proj}{exp}/baseline_vqvae/checkpoints/checkpoint_epoch={epoch}.pt")[0], map_location="cpu", weights_only=False)


def test_restarts_and_decay_are_logged_saved_and_resumed(tmp_path, capsys):
    import run_vqvae
    from synthanatomy_amd import debug
    from synthanatomy_amd.networks.vqvae.configure import decay_schedule
    proj = str(tmp_path) + "/"
    try:
        run_vqvae.run(_flags(proj, "full") + ["--epochs=3"])
        full_out = capsys.readouterr().out
        run_vqvae.run(_flags(proj, "split") + ["--epochs=1"])
        run_vqvae.run(_flags(proj, "split") + ["--epochs=3"])      # finds checkpoint_epoch=1 and resumes at epoch 1
        split_out = capsys.readouterr().out
    finally:
        debug.set_deterministic(False)
    full = _restarts(full_out)
    assert [(e, i) for e, i, _, _ in full] == [(0, 1), (0, 2), (1, 3), (1, 4), (2, 5), (2, 6)]
    assert all(0 < r == min(d, 4) for _, _, d, r in full)      # 64 codes, uniform-noise volumes: there are dead codes at every step, four restart
    cfg = dict(decay=(0.5,), decay_warmup="linear", max_decay_epochs=4)
    want = {e: decay_schedule(cfg, e + 1) for e in range(3)}
    assert want == pytest.approx({0: 0.6225, 1: 0.745, 2: 0.8675})
    assert _decays(full_out) == pytest.approx(want, abs=1e-6)
    # the resumed run: the same restarts at the same iterations, the decay of the finished epoch applied on resume
    assert _restarts(split_out) == full
    assert "resumed with --decay_warmup=linear: decay 0.6225" in split_out
    a, b = _checkpoint(proj, "full", 3), _checkpoint(proj, "split", 3)
    assert sorted(a) == ["codebook_restart", "lr_scheduler", "network", "optimizer", "trainer"]
    ra, rb = a["codebook_restart"], b["codebook_restart"]
    assert ra["idle"].dtype == torch.int32 and ra["idle"].shape == (64,) and ra["total"] == sum(r for *_, r in full) == rb["total"]
    assert torch.equal(ra["idle"], rb["idle"]) and (ra["patience"], ra["max_per_step"]) == (1, 4)
    assert not any(k.endswith("idle") or "restart" in k for k in a["network"])
    for k in ("quantizer.0.impl.weight", "quantizer.0.impl.N", "quantizer.0.impl.embed_avg"):
        assert torch.equal(a["network"][k], b["network"][k]), k


def test_an_older_checkpoint_starts_the_counters_at_zero(tmp_path, capsys):
    import run_vqvae
    proj = str(tmp_path) + "/"
    plain = [f for f in _flags(proj, "old") if not f.startswith(("--codebook_restart", "--decay_warmup", "--max_decay_epochs", "--deterministic"))]
    run_vqvae.run(plain + ["--epochs=1"])
    out = capsys.readouterr().out
    assert "codebook_dead" not in out and " decay " not in out      # the default log line
    assert sorted(_checkpoint(proj, "old", 1)) == ["lr_scheduler", "network", "optimizer", "trainer"]
    run_vqvae.run(plain + ["--epochs=2", "--codebook_restart_patience=1", "--codebook_restart_max=4"])
    out = capsys.readouterr().out
    assert out.count("has no codebook_restart entry") == 1 and "the idle counters start at zero" in out
    assert [(e, i) for e, i, _, _ in _restarts(out)] == [(1, 3), (1, 4)]
    assert "codebook_restart" in _checkpoint(proj, "old", 2)
