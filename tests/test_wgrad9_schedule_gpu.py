"""GPU: the nine-tap 3x3x3 weight gradient (conv_wgrad_halo9_kernel<8>) on its default step body against the lock-step body it replaced
(debug.override(wgrad9_lockstep=True)): dw and db bit for bit, the default body under the fp64 bound of tests/conv_bounds.py, and two
deterministic-mode runs equal.  C = 128 in and out (the kernel's layers); every case asserts through the kernel log that the plan picked the
nine-tap kernel.

Shapes.  The first three are small: the launch plan (plan_wgrad, csrc/conv_wgrad.hip) gives a 3x3x3 weight gradient to the nine-tap kernel only
from 512 steps of 8 x 16 voxels at >= 80 % tile efficiency, in blocks of at least 16 steps, so they run under debug.override(wgrad9_force=True)
(SA_DBG_WGRAD9_FORCE), which hands such launches to the nine-tap kernel in blocks of at most three steps:
  * 1 x 3x8x16: 3 steps, exact tiles, two blocks per (kd, half) of 2 and 1 steps -- the one-step block is the prologue-only path;
  * 2 x 5x9x17: ragged H and W at 30 % efficiency -- the zero fill of both operands outside the volume, the never-valid halo rows 180..183 -- 40 steps
    in 14 splits of 3 (the last one 1: nsteps not divisible by steps_per_split), splits that cross the image boundary;
  * 1 x 4x16x40: Wo = 40, the production width with a half-empty third column block, 24 steps.
The two further shapes are the smallest the DEFAULT plan hands to the nine-tap kernel (no force flag: the production split rule):
  * 2 x 65x15x31: ragged H and W, 520 steps in 31 splits of 17 (the last one 10);
  * 1 x 86x16x40: Wo = 40, 516 steps.
conv_wgrad_halo9_kernel<16> is chosen by no shape: only SA_PP_DBG bit 14, read once per process, selects it (tests/test_conv_bounds_gpu.py runs it
in a fresh child), and it keeps the lock-step body.

Operands are multiples of 1/8 in [-2, 2]: every partial sum of the fused bias gradient is then exact in fp32, so db -- added with atomics in
an order that varies from run to run -- can be compared bit for bit as well.
"""
import functools

import pytest
import torch

import conv_bounds as cb

pytestmark = pytest.mark.gpu

DEV = "cuda"
NINE = "conv_wgrad_halo9_kernel<8>"
C = 128
CASES = [
    dict(id="issue_1x3x8x16", N=1, dims=(3, 8, 16), force=True),
    dict(id="issue_2x5x9x17", N=2, dims=(5, 9, 17), force=True),
    dict(id="issue_1x4x16x40", N=1, dims=(4, 16, 40), force=True),
    dict(id="ragged_2x65x15x31", N=2, dims=(65, 15, 31)),
    dict(id="w40_1x86x16x40", N=1, dims=(86, 16, 40)),
]
RUNS = [(c, db) for c in CASES for db in ((True, False) if c["id"] in ("issue_2x5x9x17", "ragged_2x65x15x31") else (True,))]


def _ncdhw(t):
    return t.double().permute(0, 4, 1, 2, 3)


def _grid8(shape, gen, relu=False):
    t = (torch.randn(shape, generator=gen) * 4.0).round().clamp_(-16, 16) / 8.0
    return torch.relu(t) if relu else t


@functools.lru_cache(maxsize=None)
def _data(cid):
    """operands and fp64 references of a case, computed once and shared by its tests (never written to)"""
    case = next(c for c in CASES if c["id"] == cid)
    gen = torch.Generator().manual_seed(1234 + len(cid))
    N, dims = case["N"], case["dims"]
    w = torch.randn(C, C, 3, 3, 3, generator=gen) * 0.05
    b = torch.zeros(C)
    x = _grid8((N, *dims, C), gen, relu=True)
    g = _grid8((N, *dims, C), gen)
    assert torch.equal(cb.rounded(x, "bf16"), x) and torch.equal(cb.rounded(g, "bf16"), g)
    x64, g64 = _ncdhw(x), _ncdhw(g)
    dw = cb.wgrad_ref("conv", x64, g64, w.shape, 1, 1)
    A = cb.wgrad_ref("conv", x64.abs(), g64.abs(), w.shape, 1, 1)
    wit = dw - cb.wgrad_last_plane("conv", x64, g64, w.shape, 1, 1, 3)
    db = g64.sum(dim=(0, 2, 3, 4))
    Ab = g64.abs().sum(dim=(0, 2, 3, 4))
    last = g64[-1:, :, -1].sum(dim=(0, 2, 3))
    return w, b, x, g, (dw, A, wit, db, Ab, last)


def _run(case, with_db, **flags):
    from synthanatomy_amd import _ffi, debug, engine
    w, b, x, g, _ = _data(case["id"])
    op = engine.ConvOp("conv", C, C, 3, 1, 1, w.to(DEV), b.to(DEV), torch.bfloat16)
    dw = torch.zeros(w.shape, device=DEV)
    db = torch.zeros(C, device=DEV) if with_db else None
    if case.get("force"):
        flags = dict(flags, wgrad9_force=True)
    with debug.override(**flags):
        with _ffi.kernel_log() as names:
            op.wgrad(x.to(DEV).to(torch.bfloat16), g.to(DEV).to(torch.bfloat16), dw, db)
            torch.cuda.synchronize()
    return dw, db, sorted(names)


@pytest.mark.parametrize("case,with_db", RUNS, ids=[f"{c['id']}-{'db' if d else 'nodb'}" for c, d in RUNS])
def test_default_body_equals_lockstep_body_and_holds_the_fp64_bound(case, with_db):
    dw, db, names = _run(case, with_db)
    dw_l, db_l, names_l = _run(case, with_db, wgrad9_lockstep=True)
    print(f"[{case['id']}] kernels: {', '.join(names)} | lock-step: {', '.join(names_l)}")
    same_dw = torch.equal(dw, dw_l)
    same_db = (not with_db) or torch.equal(db, db_l)
    print(f"[{case['id']}] dw equal {same_dw} (max |diff| {float((dw - dw_l).abs().max()):.3e}), db equal {same_db}")
    assert any(n.startswith(NINE) for n in names) and any(n.startswith(NINE) for n in names_l), \
        f"{case['id']}: the plan did not pick {NINE}: the log holds {names}"
    assert same_dw, f"{case['id']}: dw differs between the default and the lock-step body"
    assert same_db, f"{case['id']}: db differs between the default and the lock-step body"
    rdw, A, wit, rdb, Ab, last = _data(case["id"])[4]
    cb.assert_bounded(f"[{case['id']}] dw", dw, rdw, A, wit)
    if with_db:
        cb.assert_bounded(f"[{case['id']}] db", db, rdb, Ab, rdb - last)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_two_deterministic_runs_are_equal(case):
    dw0, db0, names = _run(case, True, deterministic=True)
    dw1, db1, _ = _run(case, True, deterministic=True)
    print(f"[{case['id']}] deterministic: kernels {', '.join(names)}")
    assert any(n.startswith(NINE) for n in names), f"{case['id']}: the plan did not pick {NINE}: the log holds {names}"
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1)
