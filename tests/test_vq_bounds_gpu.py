"""GPU: the EMA vector quantizer's kernels (csrc/vq.hip: sa_vq_assign with and without its bf16 output, sa_vq_ema_update, sa_vq_perplexity,
sa_vq_backward, sa_vq_embed; csrc/deterministic.hip: sa_vq_stats_det), called through _ffi the way networks/vqvae/baseline.py calls them, under
the gate of tests/vq_bounds.py: admissible indices from the fp64 distances, then every other output against its fp64 reference for the indices
the kernel returned.  The acceptance threshold is the bound itself.  Run with -s to read every max |err| / bound."""
import numpy as np
import pytest
import torch

import vq_bounds as vb

pytestmark = pytest.mark.gpu

DEV = "cuda"
RATIOS = {}          # output -> worst max |err| / bound so far (printed, never asserted)


def _np(t):
    return t.float().cpu().numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy()


def _dev(a, dt=None):
    t = torch.tensor(np.asarray(a)).to(DEV)          # (a copy: the shared operands are read-only)
    return t if dt is None else t.to(dt)


def _assign(x, W, lp: bool):
    """one sa_vq_assign call on fresh, poisoned outputs and zeroed accumulators: (rc, outputs)"""
    from synthanatomy_amd import _ffi
    lib, st = _ffi.lib(), _ffi.stream()
    (M, D), K = x.shape, W.shape[0]
    rows, cbk = _dev(x), _dev(W)
    idx = torch.full((M,), -7, dtype=torch.int64, device=DEV)
    zq = torch.full((M, D), float("nan"), device=DEV)
    zlp = torch.full((M, D), float("nan"), dtype=torch.bfloat16, device=DEV) if lp else None
    counts, dw, sq = torch.zeros(K, device=DEV), torch.zeros(K, D, device=DEV), torch.zeros(1, device=DEV)
    wn = torch.full((K,), float("nan"), device=DEV)
    rc = lib.sa_vq_assign(_ffi.ptr(rows), _ffi.ptr(cbk), M, K, D, _ffi.ptr(idx), _ffi.ptr(zq), _ffi.ptr(zlp), _ffi.ptr(counts), _ffi.ptr(dw), _ffi.ptr(sq),
                          _ffi.ptr(wn), st)
    torch.cuda.synchronize()
    return rc, dict(idx=_np(idx), zq=_np(zq), zq_lp=_np(zlp) if lp else None, counts=_np(counts), dw=_np(dw), sq=float(sq.item())), (rows, cbk, idx)


def _stats_det(rows, cbk, idx, K):
    from synthanatomy_amd import _ffi
    M, D = rows.shape
    counts, dw, sq, ws = (torch.full(s, float("nan"), device=DEV) for s in ((K,), (K, D), (1,), (K,)))      # overwritten, not accumulated
    _ffi.check(_ffi.lib().sa_vq_stats_det(_ffi.ptr(rows), _ffi.ptr(cbk), _ffi.ptr(idx), M, K, D, _ffi.ptr(counts), _ffi.ptr(dw), _ffi.ptr(sq), _ffi.ptr(ws),
                                          _ffi.stream()), "sa_vq_stats_det")
    torch.cuda.synchronize()
    return _np(counts), _np(dw), float(sq.item())


@pytest.mark.parametrize("c", vb.CASES, ids=[vb.case_id(c) for c in vb.CASES])
def test_assign_and_statistics_within_fp64_bounds(c):
    x, W, ref = vb.case(c)
    rc, plain, _ = _assign(x, W, lp=False)
    assert rc == 0, rc
    fails = vb.gate_assign(ref, plain, RATIOS)
    assert not fails, fails
    rc, got, (rows, cbk, idx) = _assign(x, W, lp=True)
    assert rc == 0, rc
    fails = vb.gate_assign(ref, got, RATIOS)
    assert not fails, fails
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(got["idx"], plain["idx"]) and same(got["zq"], plain["zq"]), "the bf16 output changes the fp32 ones"
    det = _stats_det(rows, cbk, idx, ref.K)
    fails = vb.gate_stats(ref, got["idx"], *det, True, RATIOS, "det_")
    assert not fails, fails
    if c[3] == "nan":                     # the NaN row leaves every other row's index and zq bit for bit, and is counted once
        x2 = x.copy()
        x2[vb.NAN_ROW] = W[3]
        _, clean, _ = _assign(x2, W, lp=False)
        keep = ~ref.nanrow
        assert np.array_equal(clean["idx"][keep], got["idx"][keep]) and np.array_equal(clean["zq"][keep], got["zq"][keep])
        assert got["counts"].sum() == c[0] and det[0].sum() == c[0]
    print("worst max |err| / bound so far:", {k: float(f"{v:.3g}") for k, v in RATIOS.items()})


def test_assign_refuses_rows_the_lds_rule_or_the_float4_loads_cannot_take():
    from synthanatomy_amd import _ffi
    g = np.random.default_rng(0)
    for D, want in ((508, _ffi.SA_EUNSUPPORTED), (6, _ffi.SA_EINVAL)):
        rc, _, _ = _assign(g.standard_normal((3, D), dtype=np.float32), g.standard_normal((5, D), dtype=np.float32), lp=False)
        assert rc == want, (D, rc)


@pytest.mark.parametrize("e", vb.EMA_CASES, ids=[vb.case_id(e) for e in vb.EMA_CASES])
def test_ema_update_within_fp64_bounds(e):
    from synthanatomy_amd import _ffi
    o = vb.draw_ema(*e)
    K, D = o["avg"].shape
    N, avg, counts, dw = (_dev(o[k]) for k in ("N", "avg", "counts", "dw"))
    cbk = torch.full((K, D), float("nan"), device=DEV)
    _ffi.check(_ffi.lib().sa_vq_ema_update(_ffi.ptr(N), _ffi.ptr(avg), _ffi.ptr(cbk), _ffi.ptr(counts), _ffi.ptr(dw), K, D, o["decay"], o["eps"], _ffi.stream()),
               "sa_vq_ema_update")
    torch.cuda.synchronize()
    fails = vb.gate_ema(o, (_np(N), _np(avg), _np(cbk)), RATIOS)
    assert not fails, fails
    print("worst max |err| / bound so far:", {k: float(f"{v:.3g}") for k, v in RATIOS.items()})


@pytest.mark.parametrize("p", vb.PPL_CASES, ids=[vb.case_id(p) for p in vb.PPL_CASES])
def test_perplexity_within_fp64_bound(p):
    from synthanatomy_amd import _ffi
    counts, M = vb.draw_ppl(*p)
    cd, out = _dev(counts), torch.full((1,), float("nan"), device=DEV)
    _ffi.check(_ffi.lib().sa_vq_perplexity(_ffi.ptr(cd), counts.size, M, _ffi.ptr(out), _ffi.stream()), "sa_vq_perplexity")
    torch.cuda.synchronize()
    fails = vb.gate_ppl(counts, M, out.item(), RATIOS)
    assert not fails, fails
    print("worst max |err| / bound so far:", {k: float(f"{v:.3g}") for k, v in RATIOS.items()})


@pytest.mark.parametrize("b", vb.BWD_CASES, ids=[vb.case_id(b) for b in vb.BWD_CASES])
@pytest.mark.parametrize("g_dt", ["f32", "bf16"])
def test_backward_within_fp64_bounds(b, g_dt):
    from synthanatomy_amd import _ffi
    TD = {"f32": torch.float32, "bf16": torch.bfloat16}
    o = vb.draw_bwd(*b, g_dt)
    M, D = o["x"].shape
    rows, cbk, idx, gz, gl = _dev(o["x"]), _dev(o["W"]), _dev(o["idx"].astype(np.int64)), _dev(o["g"], TD[g_dt]), _dev(o["gl"])
    for use_g, use_gl, out_dt in ((True, True, "f32"), (True, True, "bf16"), (False, True, "f32"), (False, True, "bf16"), (True, False, "f32"), (True, False, "bf16")):
        dz = torch.full((M, D), float("nan"), dtype=TD[out_dt], device=DEV)
        _ffi.check(_ffi.lib().sa_vq_backward(_ffi.ptr(rows), _ffi.ptr(cbk), _ffi.ptr(idx), _ffi.ptr(gz) if use_g else None, _ffi.dtype_id(gz.dtype),
                                             _ffi.ptr(gl) if use_gl else None, o["beta"], M, D, _ffi.ptr(dz), _ffi.dtype_id(dz.dtype), _ffi.stream()), "sa_vq_backward")
        torch.cuda.synchronize()
        fails = vb.gate_bwd(o, use_g, use_gl, out_dt, _np(dz), RATIOS)
        assert not fails, (use_g, use_gl, out_dt, fails)
    print("worst max |err| / bound so far:", {k: float(f"{v:.3g}") for k, v in RATIOS.items()})


@pytest.mark.parametrize("out_dt", ["f32", "bf16"])
def test_embed_is_exact_and_clamps(out_dt):
    from synthanatomy_amd import _ffi
    M, K, D = 50, 17, 20
    g = np.random.default_rng(5)
    W = g.standard_normal((K, D), dtype=np.float32)
    idx = g.integers(0, K, M)
    idx[4], idx[M - 1] = -3, K + 5
    cbk, idxd = _dev(W), _dev(idx.astype(np.int64))
    out = torch.full((M, D), float("nan"), dtype={"f32": torch.float32, "bf16": torch.bfloat16}[out_dt], device=DEV)
    _ffi.check(_ffi.lib().sa_vq_embed(_ffi.ptr(cbk), _ffi.ptr(idxd), M, K, D, _ffi.ptr(out), _ffi.dtype_id(out.dtype), _ffi.stream()), "sa_vq_embed")
    torch.cuda.synchronize()
    got, want = _np(out), vb.embed_ref(W, idx, out_dt)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(want[4], vb.embed_ref(W, np.array([0]), out_dt)[0]) and np.array_equal(want[M - 1], vb.embed_ref(W, np.array([K - 1]), out_dt)[0])
