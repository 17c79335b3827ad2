"""CPU: the bounds of tests/norm_bounds.py separate a correct fp32 BatchNorm from the planted defects.  An fp32 model of csrc/norm.hip's arithmetic
(one-pass E[x^2] - mu^2, the column sums in the kernel's order) must pass every bound at every case of the GPU test, and every witness (a lost
row block, the biased running variance, momentum on the wrong side, the other mode's dx, a truncating store, a neighbour's statistics) must
fail it -- the analogue of test_bound_separates_fp32_accumulation_from_a_dropped_channel.  Run with -s to read every ratio."""
import pytest
import torch

import norm_bounds as nb

torch.set_num_threads(min(16, torch.get_num_threads()))

PARAMS = [(M, C, off, dt, det) for (M, C, off, modes) in nb.CASES for dt in ("f32", "bf16") for det in modes]
IDS = [f"{M}x{C}-{dt}-{'det' if det else 'atomic'}" for (M, C, off, dt, det) in PARAMS]
RATIOS = {}          # operand type -> output -> worst max |err| / bound so far (printed, never asserted)


def test_launch_rule_restates_the_cases():
    assert nb.launch_rule(4100, False) == (64, 65, 8 + 8 + 65) and nb.last_block_rows(4100, False) == 4
    assert nb.launch_rule(4100, True) == (65, 64, 9 + 8 + 64) and nb.last_block_rows(4100, True) == 5
    assert nb.launch_rule(65, False)[:2] == (64, 2) and nb.last_block_rows(65, True) == 1
    assert nb.launch_rule(70001, False) == (69, 1015, 9 + 8 + 1015)
    for M, _, _, modes in nb.CASES:      # deterministic mode keeps at most 64 partial slots per statistic (sa_bn_sums_ws_floats)
        assert True not in modes or nb.launch_rule(M, True)[1] <= 64


@pytest.mark.parametrize("M,C,off,dt,det", PARAMS, ids=IDS)
def test_fp32_model_passes_and_every_witness_fails(M, C, off, dt, det):
    ops = nb.draw(M, C, off, dt)
    tag = f"[{M}x{C} {dt} {'det' if det else 'atomic'}]"
    for mode in ("train", "train_norun", "eval"):
        run = mode == "train"
        got = nb.model_forward(ops["x"], ops["w"], ops["b"], ops["rm0"] if mode != "train_norun" else None, ops["rv0"] if mode != "train_norun" else None,
                               mode != "eval", det, dt)
        if not run:
            got = got[:3] + (None, None)
        nb.verify_forward(f"{tag} fwd {mode}", ops, dt, det, mode, got, RATIOS.setdefault(dt, {}))
    for training in (True, False):
        mean32, rstd32 = nb.backward_stats(ops, training)
        got = nb.model_backward(ops["x"], ops["g"], ops["w"], mean32, rstd32, ops["dw0"], ops["db0"], training, det, dt)
        nb.verify_backward(f"{tag} bwd {'train' if training else 'eval'}", ops, dt, det, training, mean32, rstd32, got, RATIOS.setdefault(dt, {}))
    print("worst max |err| / bound so far:", {d: {k: float(f"{v:.3g}") for k, v in r.items()} for d, r in RATIOS.items()})


def test_bounds_reject_a_two_ulp_mean_and_a_shifted_variance():
    """the bound itself is tight: a mean two bounds away, and a variance computed about the wrong centre, fail"""
    ops = nb.draw(1000, 33, 30.0, "f32")
    x = ops["x"].double()
    S = nb.train_stats(x, nb.gamma(1000, False))
    assert nb.check((S.mu + 0.5 * S.dmu).float(), S.mu, S.dmu)[0]
    assert not nb.check((S.mu + 2.0 * S.dmu).float(), S.mu, S.dmu)[0]
    off_centre = ((x - S.mu * (1 + 1e-2)) ** 2).mean(0)          # var + (0.01 mu)^2 = 1.09 var at 30 sigma
    assert not nb.check((off_centre + nb.EPS32).rsqrt().float(), S.rstd, S.drstd)[0]
