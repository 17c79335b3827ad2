"""CPU: the bounds of tests/local_attn_bounds.py separate correct local-window attention arithmetic from the planted defects.  The fp32 model of the
exact path and the hi / lo model of the split-bf16 path (the kernels' tiling, masks, online softmax and summation orders; torch's exp2 / log for the
device functions) must pass every bound at every case of the GPU test; every witness must fail it or be reported as below what the bound resolves
at that shape, and every witness must be asserted in at least one case; every __global__ of csrc/local_attn.hip and the decode kernel must have a
row in the kernel table.  Run with -s to read every ratio."""
import os

import pytest
import torch

import local_attn_bounds as lb
from test_conv_coverage_cpu import CSRC, kernel_names

torch.set_num_threads(min(16, torch.get_num_threads()))

RATIOS = {"exact": {}, "split": {}, "step": {}}      # output -> worst max |err| / bound so far (asserted <= 1 element-wise by the checks themselves)
ASSERTED = {"fwd": set(), "bwd": set(), "arith": set(), "step": set()}


def _report():
    print("worst max |err| / bound so far:", {p: {k: float(f"{v:.3g}") for k, v in r.items()} for p, r in RATIOS.items()})


def test_case_table_reaches_what_it_names():
    g = lb.row_geometry(23, 5)
    assert int(g["T"].max()) == 1 and int(g["nk"].max()) == 10
    g = lb.row_geometry(64, 96)
    assert int(g["lo"].max()) == 0 and int(g["T"].max()) == 1
    g = lb.row_geometry(70, 1)
    assert g["nk"].tolist() == [1] + [2] * 69
    g = lb.row_geometry(150, 70)
    assert g["lo"][139] == 0 and g["lo"][140] == 70 and g["T"][140] == 3           # key tile 0 is walked for queries 128..139 and masked for 140..149
    g = lb.row_geometry(200, 64)
    assert g["lo"][128] == 64 and g["lo"][191] == 64 and g["T"][128] == 2            # tile kt - 1 is whole for every query of the tile
    g = lb.row_geometry(257, 32)
    assert g["lo"][256] == 224 and g["T"][256] == 2 and g["T"][255] == 2             # kt_lo = 3 of the one-row tile 4; lo cuts tile 3 in the middle
    g = lb.row_geometry(321, 128)
    assert g["lo"][256] == 128 and g["T"][256] == 3 and int(g["qt_hi"][64]) == 3     # key tiles 2 .. 4, tile 3 whole; key tile 1 is walked by query tiles 1 .. 3
    g = lb.row_geometry(900, 420)
    assert g["lo"][839] == 0 and g["lo"][840] == 420 and 840 % lb.LT != 0
    assert len(lb.CASES) == len(set(lb.CASES)) and all((N, W, "flat") in lb.CASES for (N, W) in lb.NW)
    for nw in ((150, 70), (200, 64), (257, 32)):
        assert all((nw[0], nw[1], r) in lb.CASES for r in lb.REGIMES)
    assert (513, 1025, 1026) in lb.STEP_CASES and max(N for (_, _, N) in lb.STEP_CASES) == 1026


def test_split_constant_holds_for_split_pair():
    """SPLIT re-derived from split_pair bounds the dropped terms of a three-term product on random and on worst-case operands"""
    gen = torch.Generator().manual_seed(1)
    a = torch.cat([torch.randn(200000, generator=gen), torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -17, 1.0 + 2.0 ** -8 - 2.0 ** -16])])
    b = torch.cat([torch.randn(200000, generator=gen) * 100.0, torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -17, 3.0 + 2.0 ** -7 - 2.0 ** -15])])
    (ah, al), (bh, bl) = lb._split(a), lb._split(b)
    three = ah.double() * bh.double() + ah.double() * bl.double() + al.double() * bh.double()
    exact = a.double() * b.double()
    worst = float(((three - exact).abs() / exact.abs()).max())
    print(f"three-term product: worst dropped part = {worst / 2.0 ** -16:.3f} x 2^-16 (SPLIT = {lb.SPLIT / 2.0 ** -16:.3f} x 2^-16)")
    assert 2.0 ** -16 < worst <= lb.SPLIT          # (more than the 2^-16 that split_bf16.h states)
    plain = float(((ah.double() * bh.double() - exact).abs() / exact.abs()).max())
    assert plain > 100 * lb.SPLIT


@pytest.mark.parametrize("N,W,regime", [c for c in lb.CASES if c[2] != "flat"] + [(150, 70, "flat")], ids=lambda v: str(v))
def test_regimes_are_finite_and_the_bounds_non_degenerate(N, W, regime):
    c = lb.case(N, W, regime)
    s = torch.einsum("blid,bljd->blij", c.ops["q"].double() * lb.SCALE, c.ops["k"].double())
    for n in ("o", "lse"):
        assert bool(torch.isfinite(c.fwd[n]).all()), n
    for n in ("dq", "dk", "dv", "D"):
        assert bool(torch.isfinite(c.bwd[n]).all()), n
    for path in lb.PATHS:
        for n, b in c.bounds[path].items():
            ref = (c.fwd if n in ("o", "lse") else c.bwd)[n]
            assert bool(torch.isfinite(b).all()) and bool((b > 0).all()), (path, n)
            rel = float(b.median() / ref.abs().max())
            print(f"  {c.tag} {path} {n}: median bound / max |ref| = {rel:.3g}")
            assert rel < 1e-2, (path, n, rel)                     # a bound of the output's own size would pass anything
    if regime == "offset":
        assert bool(torch.isinf(torch.exp(s.float())).any())      # an unshifted fp32 exp overflows
    if regime == "peaked":
        assert float(s.std()) > 6.0
    if regime == "rising":                                        # the maximum over the visible keys moves from every key tile to the next
        top = s[0, 0, N - 1].view(-1)[: (N // lb.LT) * lb.LT].view(-1, lb.LT).amax(-1)
        assert bool((top[1:] > top[:-1] + 1.0).all())


def _models(c, path, Z32):
    o = c.ops
    fo, flse = lb.model_forward(o["q"], o["k"], o["v"], c.N, c.W, path, Z32)
    lb.verify_forward(c, path, (fo, flse, fo.to(torch.bfloat16)), RATIOS[path], ASSERTED["fwd"])
    dq, dk, dv, D = lb.model_backward(o["q"], o["k"], o["v"], o["do"], c.out32, c.lse32, c.N, c.W, path, Z32)
    lb.verify_backward(c, path, (dq, dk, dv, D, dv.to(torch.bfloat16)), RATIOS[path], ASSERTED["bwd"])
    return fo, (dq, dk, dv)


def _arithmetic_witnesses(c, Z32, split_o):
    """a plain bf16 product (no hi*lo, lo*hi terms) must fail the split bound; the split model must fail the exact bound"""
    o = c.ops
    po, _ = lb.model_forward(o["q"], o["k"], o["v"], c.N, c.W, "split", Z32, terms=("hh",))
    ok, ratio = lb.nb.check(po, c.fwd["o"], c.bounds["split"]["o"])
    print(f"    witness plain-bf16 product: o max |err| / split bound = {ratio:.3g}")
    assert not ok, f"{c.tag}: a plain bf16 product passes the split bound ({ratio:.3g})"
    ASSERTED["arith"].add("plain-bf16 product")
    ok, ratio = lb.nb.check(split_o, c.fwd["o"], c.bounds["exact"]["o"])
    print(f"    witness split model under the exact bound: o max |err| / exact bound = {ratio:.3g}")
    if not ok:
        ASSERTED["arith"].add("split model under the exact bound")


@pytest.mark.parametrize("N,W,regime", lb.CASES, ids=lb.IDS)
def test_models_pass_and_every_witness_fails(N, W, regime):
    c = lb.case(N, W, regime)
    for path in lb.PATHS:
        fo, _ = _models(c, path, None)
    _arithmetic_witnesses(c, None, fo)
    if regime == "flat":
        # the two paths separate where few keys are visible: every flat case has such rows
        assert not lb.nb.check(fo, c.fwd["o"], c.bounds["exact"]["o"])[0], f"{c.tag}: the split model passes the exact bound"
    _report()


@pytest.mark.parametrize("N,W", lb.DROP_CASES, ids=lb.DROP_IDS)
def test_dropout_models_pass_and_every_witness_fails(N, W):
    c = lb.case(N, W, "flat", True)
    for path in lb.PATHS:
        fo, _ = _models(c, path, c.Z32)
    _arithmetic_witnesses(c, c.Z32, fo)
    _report()


@pytest.mark.parametrize("W,t,N", lb.STEP_CASES, ids=lb.STEP_IDS)
def test_step_model_passes_and_every_witness_fails(W, t, N):
    ops = lb.draw_step(W, t, N)
    out, kt, v = lb.model_step(ops)
    kc, vc = ops["kc"].clone(), ops["vc"].clone()
    kc[:, :, t], vc[:, :, t] = kt, v
    lb.verify_step(ops, (out, kc, vc), RATIOS["step"], ASSERTED["step"])
    _report()


def test_step_poisons_a_read_outside_the_window():
    """the caches hold NaN outside [lo, t): a model that reads one key early gives NaN, which no bound passes"""
    ops = lb.draw_step(5, 12, 13)
    assert ops["lo"] == 5 and bool(torch.isnan(ops["kc"][:, :, 4]).all()) and bool(torch.isnan(ops["kc"][:, :, 12]).all())
    early = dict(ops, lo=4)
    out, _, _ = lb.model_step(early)
    ref = lb.step_ref(ops)
    assert not lb.nb.check(out, ref["out"], lb.step_bounds(ops, ref)[0])[0]


def test_every_witness_is_asserted_in_at_least_one_case():
    """a witness that no case resolves would hide a blind bound.  Decided from the fp64 references alone, so this runs the cases again with the
    truth itself as the output (it passes every bound and fails every resolvable witness)."""
    seen = {"fwd": set(), "bwd": set(), "step": set()}
    todo = [(N, W, r, False) for (N, W, r) in lb.CASES if r == "flat" and N <= 321] + [(N, W, "flat", True) for (N, W) in lb.DROP_CASES[:1]]
    for (N, W, r, drop) in todo:
        c = lb.case(N, W, r, drop)
        o32, dv32 = c.fwd["o"].float(), c.bwd["dv"].float()
        lb.verify_forward(c, "exact", (o32, c.fwd["lse"], o32.to(torch.bfloat16)), None, seen["fwd"])
        lb.verify_backward(c, "exact", (c.bwd["dq"], c.bwd["dk"], dv32, c.bwd["D"], dv32.to(torch.bfloat16)), None, seen["bwd"])
    for (W, t, N) in lb.STEP_CASES[:12]:
        ops = lb.draw_step(W, t, N)
        ref = lb.step_ref(ops)
        kc, vc = ops["kc"].clone(), ops["vc"].clone()
        kc[:, :, t], vc[:, :, t] = ref["kt"].float(), lb.step_heads(ops, torch.float32)[2]
        lb.verify_step(ops, (ref["out"], kc, vc), None, seen["step"])
    # the arithmetic witnesses compare two models: one case each, where the paths separate most (few visible keys)
    c = lb.case(23, 5, "flat")
    fo, _ = lb.model_forward(c.ops["q"], c.ops["k"], c.ops["v"], c.N, c.W, "split")
    ASSERTED["arith"].clear()
    _arithmetic_witnesses(c, None, fo)
    seen["arith"] = set(ASSERTED["arith"])
    for fam, names in lb.WITNESSES.items():
        missing = [w for w in names if w not in seen[fam]]
        print(f"{fam}: asserted somewhere: {sorted(seen[fam])}")
        assert not missing, f"{fam}: no case resolves the witnesses {missing}: the bound is blind to them"


def test_every_local_attention_kernel_has_a_row():
    with open(os.path.join(CSRC, "local_attn.hip")) as fh:
        declared = kernel_names(fh.read())
    with open(os.path.join(CSRC, "performer.hip")) as fh:
        step = [n for n in kernel_names(fh.read()) if n == "local_attn_step_kernel"]
    assert len(declared) == 8 and step == ["local_attn_step_kernel"], (declared, step)      # eight names, four of them templates over MODE 0 / 1
    rows = [k for entry in lb.KERNELS.values() for path in entry.values() for k in path]
    missing = [n for n in declared + step if not any(k == n or k.startswith(n + "<") for k in rows)]
    assert not missing, f"kernels without a row in tests/local_attn_bounds.py KERNELS: {missing}"
    stale = [k for k in rows if k.split("<")[0] not in declared + step]
    assert not stale, f"rows for kernels that no longer exist: {stale}"
    assert len(set(rows)) == 13, sorted(set(rows))                                          # twelve entry points + the decode kernel
    for n in declared:                                                                      # a template kernel needs both of its modes
        if n.startswith("local_attn_q_"):
            assert n + "<0>" in rows and n + "<1>" in rows, n
