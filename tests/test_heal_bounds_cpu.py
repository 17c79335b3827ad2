"""CPU: the fp32 model of heal_step_kernel's score (tests/heal_bounds.py: model_nll) holds the bound the kernel is held to in
tests/test_heal_step_gpu.py, on the same cases, and each planted defect is caught in at least one of them."""
import pytest
import torch

import heal_bounds as hlb


@pytest.mark.parametrize("temperature,k", hlb.DRAWS)
@pytest.mark.parametrize("B,V", hlb.SHAPES)
def test_model_scores_within_the_bound(B, V, temperature, k):
    c = hlb.case(B, V, temperature, hlb.top_k_of(V, k))
    asserted = set()
    for s, l in enumerate(c["logits"]):
        x = c["seq0"][:, s + 1].clone()
        if s == 3:
            x[0], x[1] = V, -1
        hlb.verify_nll(f"model {B}x{V} step {s}", l, x, temperature, hlb.model_nll(l, x, temperature), asserted=asserted)
    assert "no last pass" in asserted
    assert temperature == 1.0 or "scaled logits scored" in asserted


def test_chain_rule_and_threshold_choice():
    assert [hlb.heal_chain(V) for V in (19, 1000, 2049, 16384)] == [22, 22, 24, 37]
    assert int(hlb.last_pass(2049).sum()) == 683 and int(hlb.last_pass(19).sum()) == 19 and int(hlb.last_pass(1000).sum()) == 40
    for (B, V) in hlb.SHAPES:            # a seed exists for every case of the in-between test, decided here without a device
        for (t, k) in hlb.DRAWS:
            for P_ in (1, 2):
                c, cut = hlb.middle_threshold(B, V, t, hlb.top_k_of(V, k), P_)
                assert cut < 0 and torch.isfinite(c["nll"]).all()
