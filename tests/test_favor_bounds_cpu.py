"""CPU: the bounds of tests/favor_bounds.py separate correct fused FAVOR+ arithmetic from the planted defects.  The fp32 / split-bf16 model of the
kernels (product orders, second splits, the slab loop, both chunk-state forms, the prefix, the lane orders of the sums) must pass every bound at
every case of the GPU test; every witness must fail it or be reported as below what the bound resolves at that shape, and every witness must be
asserted in at least one case; the conditions on the inputs (ambiguous query rows, the margin of the global key maximum, finite references,
non-degenerate bounds) are checked from the references alone; every __global__ of csrc/favor_fused.hip has a row in the kernel table.  Run with -s
to read every ratio."""
import math
import os

import pytest
import torch

import favor_bounds as fb
from oracle import performer_ref as P
from test_conv_coverage_cpu import CSRC, kernel_names

torch.set_num_threads(min(16, torch.get_num_threads()))

RATIOS = {}                                                  # output -> worst max |err| / bound so far (asserted <= 1 element-wise by the checks themselves)
ASSERTED = {"fwd": set(), "bwd": set(), "arith": set()}
DONE = set()                                                 # the cases that have run in this session


def _report():
    print("worst max |err| / bound so far:", {k: float(f"{v:.3g}") for k, v in RATIOS.items()})


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_case_table_reaches_what_it_names():
    assert len(fb.CASES) == len(set(fb.CASES)) == 17
    for (B, G, N, m) in fb.SHAPES:
        assert m <= 272 and (B * G >= 40) == ((B, G, N, m) == (5, 8, 70, 266))
    ldf = {m: fb.ldf_of(m) for (_, _, _, m) in fb.SHAPES}
    assert ldf[10] == 16 and ldf[16] == 16 and ldf[64] == 64 and ldf[256] == 256 and ldf[266] == 272 and ldf[272] == 272 and ldf[120] == 128
    frags = lambda m, slab0: min(4, (fb.ldf_of(m) - slab0 + 15) >> 4)          # slab_frags
    assert frags(266, 256) == 1 and frags(272, 256) == 1 and frags(256, 192) == 4 and frags(120, 64) == 4 and frags(16, 0) == 1 and frags(10, 0) == 1
    assert [N % 64 for N in (63, 64, 65, 129)] == [63, 0, 1, 1] and (333 + 63) // 64 == 6
    assert fb.routes(5, 8) == [("natural_seq", None)] and [r for r, _ in fb.routes(2, 2)] == ["parallel", "seq"]
    assert {c[:4] for c in fb.NEW_SHAPES} == {(1, 1, 1, 16), (2, 2, 63, 64), (2, 2, 64, 64), (2, 2, 65, 64), (2, 2, 130, 10), (2, 2, 129, 256), (2, 2, 129, 272)}


def test_constants_are_within_their_stated_distance():
    assert abs(fb.C2 - 0.125) <= fb.C2_REL * 0.125 and abs(fb.C2HALF - 0.0625) <= fb.C2_REL * 0.0625
    R, REPS = fb.ratio_consts(266)
    assert abs(R - 266 ** -0.5) <= 2 * fb.U * R and abs(REPS - 1e-4 * 266 ** -0.5) <= 4 * fb.U * REPS


def test_the_backward_reference_is_the_gradient_of_the_oracle():
    """backward_ref restates the kernels' formulas in fp64; with the fp64 stabilisers and the fp64 forward it must agree with autograd through
    oracle/performer_ref.py (where no row is ambiguous, the maximum's derivative is the one-hot the formulas use)"""
    c = fb.case(2, 2, 65, 64)
    pre = dict(offq=c.hq + c.maxq, offk=c.hk, amq=c.argq, gmax=c.gmax64)
    f = fb.forward_ref(c, pre)
    got = fb.backward_ref(c, pre, f["out"], f["inv"], f)
    q, k, v = (c.o64[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
    proj = c.Ps64 / 64 ** -0.25
    cc = 64 ** -0.25

    def soft(x, is_query):                                     # performer_ref.softmax_kernel with the kernels' fp32 constants in place of the exact ones
        dash = x @ c.Ps64.T
        diag = fb.C2HALF * (x ** 2).sum(-1, keepdim=True)
        stab = dash.max(-1, keepdim=True).values if is_query else dash.max()
        return c.R * torch.exp(dash - diag - stab) + c.REPS

    out = P.causal_linear_attention(soft(q, True), soft(k, False), v, eps=fb.DEN_EPS)
    assert float((out.detach() - f["out"]).abs().max()) < 1e-12
    ref = P.causal_linear_attention(P.softmax_kernel(q, proj, True), P.softmax_kernel(k, proj, False), v)      # the oracle itself: the constants differ by a few ulp
    assert float((ref.detach() - f["out"]).abs().max() / f["out"].abs().max()) < 1e-5 and abs(cc * cc / 2 - fb.C2HALF) < 1e-8
    (out * c.o64["dattn"]).sum().backward()
    for name, g in (("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        err = float((got[name] - g).abs().max() / g.abs().max())
        print(f"  {name}: max |formula - autograd| / max |autograd| = {err:.3g}")
        assert err < 1e-10, (name, err)


@pytest.mark.parametrize("B,G,N,m,regime,bf16", fb.CASES, ids=fb.IDS)
def test_model_passes_and_every_witness_fails(B, G, N, m, regime, bf16):
    c = fb.case(B, G, N, m, regime, bf16)
    # ---- conditions on the inputs, from the references alone
    n_amb, rows = int(c.ambiguous.sum()), c.ambiguous.numel()
    # (the issue counted 1/600, 1/666, 7/2800, 2/520, 1/516 with the top-two rule; this rule asks every other feature to clear the two bounds, and
    #  SECOND is part of bdd: recounted here, the cap is the issue's)
    print(f"  {c.tag}: {n_amb} of {rows} query rows are ambiguous; the global key maximum clears every other element by {c.gmax_margin:.3g} beyond the two bounds "
          f"(bound {c.bgmax:.3g})")
    assert n_amb <= fb.AMBIGUOUS_CAP * rows or rows < 100 and n_amb == 0
    assert c.gmax_margin > 0, f"{c.tag}: the global key maximum is ambiguous"
    if regime == "offset":
        b_, n_, g_, _ = c.gmax_where
        assert (b_, n_, g_) == c.planted and n_ == N - 1 and n_ // 64 == c.S - 1 and n_ > 0
    if regime == "hot":
        arg = (c.ddk - c.hk.unsqueeze(-1) - c.gmax64).amin()
        assert float(arg) < -70.0
    # ---- pre-pass
    mp = fb.model_prepass(c)
    pre = fb.verify_prepass(c, (mp["offq"], mp["offk"], mp["amq"], mp["gmax"], mp["gidx"]), RATIOS)
    ok, r = fb.nb.check(mp["ddq"], c.ddq, c.bddq)
    assert ok, r
    plain = fb.model_prepass(c, terms=("hh",))
    ok, r = fb.nb.check(plain["ddq"], c.ddq, c.bddq)
    print(f"    witness plain-bf16 product in the dd GEMM: dd max |err| / bound = {r:.3g}")
    assert not ok
    ASSERTED["arith"].add("plain-bf16 product in the dd GEMM")
    if bf16:                                                   # the two-product path equals the three-product path bit for bit
        full = fb._dd(c.ops["q"], fb._pad_rows(c.ops["Ps"], m), ("lh", "hl", "hh"))[..., :m]
        assert torch.equal(_bits(full), _bits(mp["ddq"]))
    # ---- forward and backward, both chunk-state forms
    st = fb.Stage(c, pre)
    for name, r in st.fwd.items():
        assert bool(torch.isfinite(r).all()), name
    for name, r in st.bwd.items():
        assert bool(torch.isfinite(r).all()), name
    for name, (share, med) in st.shares().items():
        print(f"  {c.tag} {name}: bound > max |ref| on {share:.3g} of the elements; median bound / max |ref| = {med:.3g}")
        cap = fb.SHARE_CAP.get(name, {}).get("N1" if N == 1 else regime, 0.0)
        assert share <= cap and (med < 5e-2 or cap > 0.0), (name, share, med)
    for name, b in (("out", st.bout), ("inv", st.binv), *st.bb.items()):
        assert bool(torch.isfinite(b).all()) and bool((b > 0).all()), name
    for route, seq in fb.routes(B, G):
        seq = True if seq is None else seq
        out, inv, _ = fb.model_forward(c, mp, seq)
        st.verify_forward((out, inv, out.to(torch.bfloat16)), RATIOS, ASSERTED["fwd"])
        dden, dq, dk, dv, tsum = fb.model_backward(c, mp, st.attn32, st.inv32, seq)
        st.verify_backward((dden, dq, dk, dv, tuple(t.to(torch.bfloat16) for t in (dq, dk, dv)), tsum), RATIOS, ASSERTED["bwd"])
    DONE.add((B, G, N, m, regime, bf16))
    _report()


def test_every_witness_is_asserted_in_at_least_one_case():
    """decided from the fp64 references alone: the truth itself as the output passes every bound and fails every resolvable witness"""
    seen = {"fwd": set(), "bwd": set()}
    for key in [(2, 2, 65, 64, "flat", False), (2, 2, 130, 10, "flat", False), (2, 2, 150, 266, "hot", False), (2, 2, 150, 266, "offset", False)]:
        c = fb.case(*key)
        pre = dict(offq=(c.hq + c.maxq).float().double(), offk=c.hk.float().double(), amq=c.argq, gmax=float(torch.tensor(c.gmax64).float()))
        st = fb.Stage(c, pre)
        o32 = st.fwd["out"].float()
        st.verify_forward((o32, st.fwd["inv"], o32.to(torch.bfloat16)), None, seen["fwd"])
        g32 = [st.bwd[n].float() for n in ("dq", "dk", "dv")]
        chunk = (c.N - 1 - torch.arange(c.N)) // 64
        tsum = (st.aux["tk"] @ (chunk[:, None] == torch.arange(c.S)[None, :]).double()).reshape(-1)
        st.verify_backward((st.bwd["dden"], *(st.bwd[n] for n in ("dq", "dk", "dv")), None, tsum), None, seen["bwd"])
        for n, t in zip(("dq", "dk", "dv"), g32):
            fb.lb.assert_rounded_once(f"{c.tag} {n}_lp", t, t.to(torch.bfloat16), seen["bwd"])
    c = fb.case(2, 2, 65, 64)
    ok, _ = fb.nb.check(fb.model_prepass(c, terms=("hh",))["ddq"], c.ddq, c.bddq)
    assert not ok
    seen["arith"] = {"plain-bf16 product in the dd GEMM"}
    for fam, names in fb.WITNESSES.items():
        missing = [w for w in names if w not in seen[fam]]
        print(f"{fam}: asserted somewhere: {sorted(seen[fam])}")
        assert not missing, f"{fam}: no case resolves the witnesses {missing}: the bound is blind to them"


def test_every_fused_favor_kernel_has_a_row():
    with open(os.path.join(CSRC, "favor_fused.hip")) as fh:
        declared = kernel_names(fh.read())
    assert len(declared) == 18, declared
    rows = {k for entry in fb.KERNELS.values() for names in entry.values() for k in names} | set(fb.KERNELS_BY_REFERENCE)
    missing = [n for n in declared if n not in rows]
    assert not missing, f"kernels without a row in tests/favor_bounds.py: {missing}"
    stale = [k for k in rows if k not in declared]
    assert not stale, f"rows for kernels that no longer exist: {stale}"
    assert "not reachable from aligned buffers" in fb.KERNELS_BY_REFERENCE["favor_fdden_kernel"]
    for entry in fb.KERNELS.values():
        for names in entry.values():
            assert names == sorted(names)


def test_recorded_model_ratios_are_the_measured_ones():
    """MEASURED's model column is what the cases above give, to the printed digits (one unit of the last digit is left to a BLAS that adds the fp64
    references in another order).  Runs after the cases; a session that ran only some of them can only stay below the recorded worst."""
    for name, r in RATIOS.items():
        rec = fb.MEASURED["model"][name]
        last = 10.0 ** (math.floor(math.log10(rec)) - 2)
        print(f"  {name}: measured {r:.3g}, recorded {rec:.3g}")
        if len(DONE) == len(fb.CASES):
            assert abs(float(f"{r:.3g}") - rec) <= 1.001 * last, (name, r, rec)
        else:
            assert float(f"{r:.3g}") <= rec + 1.001 * last, (name, r, rec)
    assert len(DONE) < len(fb.CASES) or set(RATIOS) == set(fb.OUTPUTS)
