"""CPU: the gate of tests/vq_bounds.py separates a correct fp32 vector quantizer from the planted defects.  An fp32 model of csrc/vq.hip's
arithmetic (the __f*_rn chains, the MFMA's fmaf chain, first-index selection in the order a wave meets its tiles, the leader-row statistics)
must pass the gate on every case of the GPU test, and every witness (ties to the last index, a dropped partial tile, padding rows counted, a
neighbour's wnorm, a lost block of dw, EMA from the old N, EMA and perplexity without their epsilons) must fail it on the case named for it.  The
conditions the cases are chosen for -- coverage of every code, tied pairs at every reduction stage, at most 1 % ambiguous rows, exact lattice
arithmetic, every NV and trip count -- are asserted from the fp64 reference alone.  Run with -s to read every ratio."""
import numpy as np
import pytest

import vq_bounds as vb

RATIOS = {}          # output -> worst max |err| / bound so far (printed, never asserted)
IDS = [vb.case_id(c) for c in vb.CASES]


def test_dispatch_rule_and_the_cases_reach_every_path():
    assert [vb.nv_for(D) for D in (4, 16, 20, 32, 36, 64, 68, 128, 132, 256, 260, 504)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32]
    assert [vb.trips(K) for K in (1, 3, 16, 17, 64, 65, 129, 257, 2048)] == [1, 1, 1, 1, 1, 2, 3, 5, 32]
    assert vb.lds_bytes(504) <= vb.LDS_LIMIT < vb.lds_bytes(508) and vb.lds_bytes(504) == 163216
    assert {vb.nv_for(D) for (_, _, D, _) in vb.CASES} == {1, 2, 4, 8, 16, 32}
    assert {1, 2, 3} <= {vb.trips(K) for (_, K, _, _) in vb.CASES} and max(vb.trips(K) for (_, K, _, _) in vb.CASES) >= 5
    assert {D for (_, _, D, _) in vb.CASES} >= {4, 16, 20, 32, 36, 64, 68, 128, 132, 256, 260, 504}
    assert {K for (_, K, _, _) in vb.CASES} >= {1, 3, 16, 17, 64, 65, 129, 257, 2048}
    assert {M for (M, _, _, _) in vb.CASES} >= {1, 15, 16, 17, 33} and any(M == K + 1 for (M, K, _, _) in vb.CASES)
    assert all(M * K * D <= 10 ** 7 for (M, K, D, _) in vb.CASES)
    for w, c in vb.WITNESSES.items():
        assert c in vb.CASES, w


@pytest.mark.parametrize("c", vb.CASES, ids=IDS)
def test_case_conditions_hold_from_the_reference_alone(c):
    M, K, D, kind = c
    x, W, ref = vb.case(c)
    many = int(((ref.nadm > 1) & ~ref.nanrow).sum())
    print(f"  [{vb.case_id(c)}] rows with more than one admissible code: {many} of {M}")
    assert (ref.nadm[~ref.nanrow] >= 1).all()
    if kind in ("near", "randn", "collapsed", "nan"):
        assert many <= 0.01 * M, f"{many} of {M} rows are ambiguous"
    if kind == "near" and M >= K:               # every wave, trip parity, lane group and accumulator slot decides some row on its own
        assert set(ref.sole[ref.sole >= 0]) == set(range(K))
    if kind == "collapsed":
        assert set(ref.sole) == set(vb.COLLAPSED_CODES) and (ref.sole[:32] == ref.sole[0]).all() and (ref.sole[32:48] == ref.sole[32]).all() and M % 16
    if kind == "nan":
        assert ref.nanrow.sum() == 1 and ref.nanrow[vb.NAN_ROW]
    if kind == "lattice":
        assert ref.lattice_exact()
        off, group, tile = ref.tie_offsets()
        print(f"    tied pairs: {off.size}; offsets 16: {(off == 16).sum()}, 64: {(off == 64).sum()}, >= 128: {(off >= 128).sum() if K > 128 else '-'}, "
              f"one lane group: {group.sum()}, one tile across lane groups: {(tile & ~group).sum()}")
        assert (off == 16).any() and (off == 64).any() and group.any() and (tile & ~group).any()     # cross-wave, next trip, r loop, shuffle
        assert K <= 128 or (off >= 128).any()                                                        # the other register buffer
        assert (ref.first_min >= 16).any() and (K <= 128 or (ref.first_min >= 64).any())        # the winner is not always wave 0's first tile
    if kind == "ladder":
        even, odd = np.arange(M) % 2 == 0, np.arange(M) % 2 == 1
        best2 = np.sort(ref.d64, 1)[:, :2]
        assert (best2[even, 0] == best2[even, 1]).all() and (ref.nadm[even] == 2).all()              # gap 0: the bitwise duplicate
        assert (ref.canon[ref.d64[even].argmin(1)] == ref.d64[even].argmin(1)).all()
        gap = (best2[odd, 1] - best2[odd, 0]) / ref.delta[odd, ref.d64[odd].argmin(1)]
        print(f"    gap / delta on the 8-delta rows: {gap.min():.3g} .. {gap.max():.3g}")
        assert (ref.nadm[odd] == 1).all() and gap.min() > 4 and gap.max() < 16
        win = ref.sole[odd]
        second = np.argsort(ref.d64[odd], 1)[:, 1]
        assert (win < second).any() and (win > second).any()


@pytest.mark.parametrize("c", vb.CASES, ids=IDS)
def test_fp32_model_passes_the_gate(c):
    x, W, ref = vb.case(c)
    got = vb.model_assign(x, W)
    fails = vb.gate_assign(ref, got, RATIOS)
    assert not fails, fails
    det = vb.model_stats_det(x, W, got["idx"])
    fails = vb.gate_stats(ref, got["idx"], *det, True, RATIOS, "det_")
    assert not fails, fails
    if c[3] == "nan":                           # the NaN row leaves every other row's outputs bit for bit
        x2 = x.copy()
        x2[vb.NAN_ROW] = W[3]
        clean = vb.model_assign(x2, W)
        keep = ~ref.nanrow
        assert np.array_equal(clean["idx"][keep], got["idx"][keep]) and np.array_equal(clean["zq"][keep], got["zq"][keep])
        assert got["counts"].sum() == c[0]
    print("worst max |err| / bound so far:", {k: float(f"{v:.3g}") for k, v in RATIOS.items()})


@pytest.mark.parametrize("w", sorted(vb.WITNESSES))
def test_every_assign_witness_fails_on_its_case(w):
    c = vb.WITNESSES[w]
    x, W, ref = vb.case(c)
    fails = vb.gate_assign(ref, vb.model_assign(x, W, defect=w))
    print(f"  witness {w} on {vb.case_id(c)}: {fails}")
    assert fails, f"the planted defect '{w}' passes the gate on {vb.case_id(c)}"
    assert not vb.gate_assign(ref, vb.model_assign(x, W))


def test_further_witnesses_of_the_index_gate():
    """the duplicate rule and the sole-winner rule on their own: the ladder's later duplicate, and a code one 8-delta step away"""
    c = (130, 129, 32, "ladder")
    x, W, ref = vb.case(c)
    idx = vb.model_assign(x, W)["idx"]
    assert not vb.gate_index(ref, idx)
    later = idx.copy()
    later[0] = idx[0] + 64
    assert ref.adm[0, later[0]] and any("duplicate" in f for f in vb.gate_index(ref, later))
    other = idx.copy()
    other[1] = np.argsort(ref.d64[1])[1]
    assert any("inadmissible" in f for f in vb.gate_index(ref, other))
    assert vb.gate_index(ref, np.full_like(idx, 129)) and vb.gate_index(ref, np.full_like(idx, -1))


@pytest.mark.parametrize("e", vb.EMA_CASES, ids=[vb.case_id(e) for e in vb.EMA_CASES])
def test_ema_model_passes_and_witnesses_fail(e):
    o = vb.draw_ema(*e)
    idle = o["counts"] == 0
    assert idle.sum() >= len(idle) // 5 and (idle & (o["N"] == 0)).any() and (len(idle) < 10 or (idle & (o["N"] > 0)).any())
    fails = vb.gate_ema(o, vb.model_ema(o), RATIOS)
    assert not fails, fails
    for w, case in vb.EMA_WITNESSES.items():
        if case == e:
            wf = vb.gate_ema(o, vb.model_ema(o, defect=w))
            print(f"  witness ema {w}: {wf}")
            assert any("ema_cb" in f for f in wf), w
    print("worst max |err| / bound so far:", {k: float(f"{v:.3g}") for k, v in RATIOS.items()})


@pytest.mark.parametrize("p", vb.PPL_CASES, ids=[vb.case_id(p) for p in vb.PPL_CASES])
def test_perplexity_model_passes_and_witness_fails(p):
    counts, M = vb.draw_ppl(*p)
    if p[1] in ("zeros", "one"):
        assert (counts == 0).any()
    if p[1] in ("all", "one"):
        assert counts.max() == M and np.float32(1.0) / np.float32(M) * np.float32(M) != 1.0      # 1 / M rounds: p^ is not 1
    fails = vb.gate_ppl(counts, M, vb.model_ppl(counts, M), RATIOS)
    assert not fails, fails
    for w, case in vb.PPL_WITNESSES.items():
        if case == p:
            assert vb.gate_ppl(counts, M, vb.model_ppl(counts, M, defect=w)), w
    assert vb.gate_ppl(counts, M, np.float32(vb.ppl_ref(counts, M)[0] * (1 + 1e-4)))
    print("worst max |err| / bound so far:", {k: float(f"{v:.3g}") for k, v in RATIOS.items()})


@pytest.mark.parametrize("b", vb.BWD_CASES, ids=[vb.case_id(b) for b in vb.BWD_CASES])
@pytest.mark.parametrize("g_dt", ["f32", "bf16"])
def test_backward_model_passes(b, g_dt):
    o = vb.draw_bwd(*b, g_dt)
    for use_g, use_gl, out_dt in ((True, True, "f32"), (True, True, "bf16"), (False, True, "f32"), (True, False, "f32"), (True, False, "bf16"), (False, True, "bf16")):
        fails = vb.gate_bwd(o, use_g, use_gl, out_dt, vb.model_bwd(o, use_g, use_gl, out_dt), RATIOS)
        assert not fails, (use_g, use_gl, out_dt, fails)
    # witnesses: the factor 2 of the squared error's derivative lost; a truncating bf16 store
    ref, _ = vb.bwd_ref(o, True, True, "f32")
    half = (o["g"].astype(np.float64) + 0.5 * (ref - o["g"])).astype(np.float32)
    assert vb.gate_bwd(o, True, True, "f32", half)
    import conv_bounds as cb
    import torch
    assert vb.gate_bwd(o, True, True, "bf16", cb.truncated(torch.from_numpy(ref), "bf16").float().numpy())
    print("worst max |err| / bound so far:", {k: float(f"{v:.3g}") for k, v in RATIOS.items()})
