"""GPU: a plain `python bench.py` run -- the headline steps only, the result line's fields, and `--dump-outputs` writing what the last timed
step computed (float32 / float64 arrays, at most 64 MB in all): the same on every run of the same arguments, and taken after exactly
warmup + steps training steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1.65e-4     # bench.py's Adam learning rate: the first Adam step moves every parameter by about this much


def _bench(out, steps, warmup):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--batch", "1",
                        "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return lines[0], {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}


def _moved(a, b):
    """Fraction of the sampled parameters that differ by more than a rounding-level amount (an Adam step moves them by ~LR)."""
    return float((np.abs(a["parameters_sample"] - b["parameters_sample"]) > 1e-6).mean())


def _rel(x, y):
    return abs(float(x) - float(y)) / abs(float(y))


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    d, a = _bench(tmp_path / "a", steps=1, warmup=0)
    assert d["metric"] == "vqvae_train_volumes_per_sec" and d["unit"] == "volumes/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["ms_per_step"] > 0 and d["value"] > 0
    for extra in ("roofline", "roofline_hbm", "inference", "cpu_baseline", "fp32_mode", "latency_b1", "adversarial", "secondary", "end_to_end",
                  "regression_guard"):
        assert extra not in d, extra
    assert set(a) == {"loss", "quantization_loss", "reconstruction_sample", "parameters_sample", "codebook"}
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in a) <= 64 * 2 ** 20
    for k, v in a.items():
        assert v.dtype in (np.float32, np.float64) and np.isfinite(v).all(), k
    assert a["codebook"].shape == (2048, 32)
    assert a["reconstruction_sample"].size > 1 << 21 and a["parameters_sample"].size > 1 << 21

    # the same arguments again: seeded inputs and initial weights, so the first step computes the same outputs (up to the order of atomic sums)
    _, b = _bench(tmp_path / "b", steps=1, warmup=0)
    assert {k: v.shape for k, v in b.items()} == {k: v.shape for k, v in a.items()}
    assert _rel(b["loss"], a["loss"]) < 1e-4, (float(b["loss"]), float(a["loss"]))
    rec = np.abs(b["reconstruction_sample"] - a["reconstruction_sample"]).max() / np.abs(a["reconstruction_sample"]).max()
    assert rec < 2e-2, rec
    assert np.allclose(b["codebook"], a["codebook"], rtol=1e-3, atol=1e-6)
    assert _moved(a, b) < 0.01, _moved(a, b)

    # the dump is the LAST timed step, after exactly warmup + steps optimizer steps: two timed steps end where one warm-up + one timed step ends,
    # and one step further than a single step
    _, c = _bench(tmp_path / "c", steps=2, warmup=0)
    _, e = _bench(tmp_path / "e", steps=1, warmup=1)
    assert _rel(c["loss"], e["loss"]) < 1e-3, (float(c["loss"]), float(e["loss"]))
    assert _moved(c, e) < 0.01, _moved(c, e)
    assert _rel(c["loss"], a["loss"]) > 1e-3, (float(c["loss"]), float(a["loss"]))
    assert _moved(c, a) > 0.5, _moved(c, a)
    assert np.abs(c["parameters_sample"] - a["parameters_sample"]).max() < 3 * LR
