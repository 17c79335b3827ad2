"""CPU: the bounds of tests/head_bounds.py separate a correct fp32 LayerNorm / cross-entropy from the planted defects.  An fp32 model of the kernels'
arithmetic (the stride-64 lane sums and the butterfly in order, the block partials in one fixed order, torch's exp / log / rsqrt for the device
functions) must pass every bound at every case of the GPU test, every witness must fail it or be reported as below what the bound resolves at
that shape, and every witness must be asserted in at least one case.  Run with -s to read every ratio."""
import pytest
import torch

import head_bounds as hb

torch.set_num_threads(min(16, torch.get_num_threads()))

RATIOS = {"ln": {}, "ce": {}}        # output -> worst max |err| / bound so far (asserted <= 1 element-wise by the checks themselves)
ASSERTED = {"ln": set(), "ce": set()}


def test_launch_rules_restate_the_cases():
    assert hb.wave_chain(32) == 7 and hb.wave_chain(64) == 7 and hb.wave_chain(65) == 8 and hb.wave_chain(2049) == 33 + 6
    assert hb.last_stride(32) == 0 and hb.last_stride(64) == 0 and hb.last_stride(65) == 64 and hb.last_stride(200) == 192 and hb.last_stride(513) == 512
    assert hb.ln_col_rule(37, 32, "atomic") == ("rows", 8 + 2 + 2, 2, 5)
    assert hb.ln_col_rule(33, 512, "atomic") == ("rows", 8 + 2 + 2, 2, 1)
    assert hb.ln_col_rule(9, 513, "atomic") == ("per-element", 9, 9, 1)
    assert hb.ln_col_rule(4100, 64, "atomic") == ("rows", 8 + 2 + 129, 129, 4)
    assert hb.ln_col_rule(4100, 64, "det") == ("colsum_det", 5 + 2 + 242, 0, 3)          # rpb = 17
    assert hb.ln_col_rule(70, 200, "det") == ("colsum_det", 1 + 2 + 70, 0, 1)
    assert hb.ce_loss_rule(70, "atomic") == (8 + 9, 9, 6) and hb.ce_loss_rule(10, "atomic") == (8 + 2, 2, 2) and hb.ce_loss_rule(8, "atomic") == (9, 1, 8)
    assert hb.ce_loss_rule(70, "det") == (11, 0, 2)


def _ln_forward(tag, ops):
    y, stats = hb.model_ln_forward(ops["x"], ops["w"], ops["b"])
    lps = {dt: y.to(hb.cb.DT[dt]) for dt in ("bf16", "f16")}
    hb.verify_ln_forward(f"{tag} fwd", ops, (y, stats, lps), RATIOS["ln"], ASSERTED["ln"])


def _ln_backward(tag, ops):
    stats32 = hb.ln_backward_stats(ops)
    for route in hb.LN_ROUTES:
        dx, dw, db = hb.model_ln_backward(ops["x"], ops["dy"], ops["w"], stats32, ops["dw0"], ops["db0"], route)
        hb.verify_ln_backward(f"{tag} bwd {route}", ops, route, stats32, (dx if route == "atomic" else None, dw, db), RATIOS["ln"], ASSERTED["ln"])


@pytest.mark.parametrize("R,C,off,sc", hb.LN_CASES, ids=hb.LN_IDS)
def test_layernorm_model_passes_and_every_witness_fails(R, C, off, sc):
    ops = hb.draw_ln(R, C, off, sc)
    tag = f"[LN {R}x{C} off {off:g} x {sc:g}]"
    _ln_forward(tag, ops)
    _ln_backward(tag, ops)
    print("worst max |err| / bound so far:", {k: float(f"{v:.3g}") for k, v in RATIOS["ln"].items()})


@pytest.mark.parametrize("R,V,sc,off", hb.CE_CASES, ids=hb.CE_IDS)
def test_cross_entropy_model_passes_and_every_witness_fails(R, V, sc, off):
    ops = hb.draw_ce(R, V, sc, off)
    for name, key in hb.ce_variants(R, V):
        for route in hb.CE_ROUTES:
            for gscale in (1.0, hb.f32(1.0 / R)):
                for out in ("f32", "bf16"):
                    tag = f"[CE {R}x{V} x {sc:g} off {off:g}{name} {route} gscale {gscale:.3g} {out}]"
                    loss, row_loss, grad = hb.model_ce(ops["l"], ops[key], ops["loss0"], gscale, route, out)
                    hb.verify_ce(tag, ops, ops[key], gscale, route, out, (loss, row_loss, grad), RATIOS["ce"], ASSERTED["ce"])
    print("worst max |err| / bound so far:", {k: float(f"{v:.3g}") for k, v in RATIOS["ce"].items()})


def test_every_witness_is_asserted_in_at_least_one_case():
    """a witness that no case resolves would hide a blind bound.  Decided from the fp64 references alone, so this runs every case again with the
    truth itself as the output (it passes every bound with ratio 0 and fails every resolvable witness)."""
    seen = {"ln": set(), "ce": set()}
    for (R, C, off, sc) in hb.LN_CASES:
        ops = hb.draw_ln(R, C, off, sc)
        o = hb.fp64(ops)
        S = hb.RowStats(o["x"])
        y = hb.ln_apply(o["x"], S, o["w"], o["b"])
        hb.verify_ln_forward("truth", ops, (y, torch.cat([S.mu, S.rstd], 1).reshape(-1), {"bf16": y.float().to(torch.bfloat16)}), None, seen["ln"])
        stats32 = hb.ln_backward_stats(ops)
        st = stats32.double().view(R, 2)
        for route in hb.LN_ROUTES:
            hb.verify_ln_backward("truth", ops, route, stats32, hb.ln_backward_ref(o["x"], o["dy"], o["w"], st[:, :1], st[:, 1:], o["dw0"], o["db0"]), None, seen["ln"])
    for (R, V, sc, off) in hb.CE_CASES:
        ops = hb.draw_ce(R, V, sc, off)
        for route in hb.CE_ROUTES:
            for gscale in (1.0, hb.f32(1.0 / R)):
                for out in ("f32", "bf16"):
                    ref = hb.ce_ref(ops["l"].double(), ops["tgt"], gscale)
                    loss = hb.ce_loss_ref(ref["term"], float(ops["loss0"]) if route == "atomic" else 0.0)
                    grad = ref["grad"].to(hb.cb.DT[out])         # (verify_ce wants the output type; one rounding of the truth is inside its bound)
                    hb.verify_ce("truth", ops, ops["tgt"], gscale, route, out, (loss, ref["term"], grad), None, seen["ce"])
    for fam in ("ln", "ce"):
        missing = [w for w in hb.WITNESSES[fam] if w not in seen[fam]]
        print(f"{fam}: asserted somewhere: {sorted(seen[fam])}")
        assert not missing, f"{fam}: no case resolves the witnesses {missing}: the bound is blind to them"


def test_bounds_reject_a_one_pass_variance_and_a_two_bound_mean():
    """the bounds are tight where it matters: at 30 sigma row means a mean two bounds away fails, and so does the rstd of a ONE-pass fp32 variance
    E[x^2] - mu^2 (relative error ~ G mu^2 / var), which the two-pass kernel's dvar = (G + 4 U) var + dmu^2 has no room for"""
    R, C, off, sc = hb.LN_CASES[2]
    assert off == 30.0
    ops = hb.draw_ln(R, C, off, sc)
    x = ops["x"]
    S = hb.RowStats(x.double())
    assert hb.nb.check((S.mu + 0.5 * S.dmu).float(), S.mu, S.dmu)[0]
    assert not hb.nb.check((S.mu + 2.0 * S.dmu).float(), S.mu, S.dmu)[0]
    mean = hb._wave_sum32(x) / C
    one_pass = hb._wave_sum32(x * x) / C - mean * mean
    ok, ratio = hb.nb.check((one_pass + hb.EPS32).rsqrt(), S.rstd, S.drstd)
    print(f"one-pass variance at 30 sigma: max |err| / bound of rstd = {ratio:.3g}")
    assert not ok
