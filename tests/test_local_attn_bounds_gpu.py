"""GPU: the causal local-window attention kernels (csrc/local_attn.hip: sa_local_attn_fwd / _bwd / _fwd_dropout / _bwd_dropout on the exact-fp32 and the
split-bf16 path) and the decode step (csrc/performer.hip: sa_local_attn_step), called through _ffi with the engine's strides and offsets, against
the fp64 reference under the element-wise bounds of tests/local_attn_bounds.py -- every output, the bf16 mirrors, the planted-defect witnesses the same
output must fail.  Input columns outside the addressed head blocks hold NaN; every output buffer starts as NaN and must still hold NaN outside the
written head blocks.  Run with -s to read every max |err| / bound and witness."""
import pytest
import torch

import local_attn_bounds as lb

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(16, torch.get_num_threads()))
DEV = "cuda"
RATIOS = {"exact": {}, "split": {}, "step": {}}      # output -> worst max |err| / bound so far (printed; the checks themselves assert <= 1 element-wise)
SA_EINVAL, SA_EUNSUPPORTED = -1, -2                  # include/synthanatomy_hip.h


def _report():
    print("worst max |err| / bound so far:", {p: {k: float(f"{v:.3g}") for k, v in r.items()} for p, r in RATIOS.items()})


def _all_nan(t):
    return bool(torch.isnan(t.float()).all())


class _Buffers:
    """the operands of a case on the device in the engine's layout (NaN outside the head blocks)"""

    def __init__(self, c):
        st = self.st = lb.strides(c.N)
        o = c.ops
        self.q, self.k, self.v = (lb.pack(o[n], *st[n]).to(DEV) for n in ("q", "k", "v"))
        self.do, self.out = lb.pack(o["do"], *st["o"]).to(DEV), lb.pack(c.out32, *st["o"]).to(DEV)
        self.lse = lb.pack_rows(c.lse32).to(DEV)

    def strides3(self):
        from synthanatomy_amd import _ffi
        st = self.st
        return (_ffi.ptr(self.q), *st["q"], _ffi.ptr(self.k), *st["k"], _ffi.ptr(self.v), *st["v"])


def _forward(c, buf, path, entry, p=None):
    """one forward call: (o, lse, o_lp) as [B, L, N, ..] on the CPU, after the layout checks"""
    from synthanatomy_amd import _ffi, debug
    lib, B, N = _ffi.lib(), c.B, c.N
    so, oo = buf.st["o"]
    o, lse = torch.full((B * N, so), float("nan"), device=DEV), torch.full((B * N * lb.L,), float("nan"), device=DEV)
    o_lp = torch.full((B * N, so), float("nan"), dtype=torch.bfloat16, device=DEV)
    with debug.override(local_attn_exact=path == "exact"), _ffi.kernel_log() as names:
        if entry == "fwd":
            rc = lib.sa_local_attn_fwd(*buf.strides3(), _ffi.ptr(o), so, oo, _ffi.ptr(lse), B, N, lb.L, c.W, lb.DH, _ffi.ptr(o_lp), _ffi.stream())
        else:
            rc = lib.sa_local_attn_fwd_dropout(*buf.strides3(), _ffi.ptr(o), so, oo, _ffi.ptr(lse), B, N, lb.L, c.W, lb.DH, _ffi.ptr(o_lp), p,
                                               lb.DROP["seed"], lb.DROP["site"], _ffi.stream())
        _ffi.check(rc, entry)
        torch.cuda.synchronize()
    assert sorted(names) == lb.KERNELS[entry][path], names
    o, lse, o_lp = o.cpu(), lse.cpu(), o_lp.cpu()
    assert _all_nan(lb.outside(o, oo)) and _all_nan(lb.outside(o_lp, oo)), f"{c.tag} {path}: the forward wrote outside the head blocks of o"
    return lb.unpack(o, B, N, oo), lb.unpack_rows(lse, B, N), lb.unpack(o_lp, B, N, oo)


def _backward(c, buf, path, entry, p=None):
    """one backward call that is given c.out32 / c.lse32: (dq, dk, dv, D, dv_lp)"""
    from synthanatomy_amd import _ffi, debug
    lib, B, N = _ffi.lib(), c.B, c.N
    st = buf.st
    nan = lambda s, dt=torch.float32: torch.full((B * N, s), float("nan"), dtype=dt, device=DEV)
    dq, dk, dv, dv_lp = nan(st["q"][0]), nan(st["k"][0]), nan(st["v"][0]), nan(st["v"][0], torch.bfloat16)
    D = torch.full((B * N * lb.L,), float("nan"), device=DEV)
    args = (*buf.strides3(), _ffi.ptr(buf.out), _ffi.ptr(buf.do), *st["o"], _ffi.ptr(buf.lse), _ffi.ptr(dq), _ffi.ptr(dk), _ffi.ptr(dv), _ffi.ptr(D),
            B, N, lb.L, c.W, lb.DH, _ffi.ptr(dv_lp))
    with debug.override(local_attn_exact=path == "exact"), _ffi.kernel_log() as names:
        if entry == "bwd":
            rc = lib.sa_local_attn_bwd(*args, _ffi.stream())
        else:
            rc = lib.sa_local_attn_bwd_dropout(*args, p, lb.DROP["seed"], lb.DROP["site"], _ffi.stream())
        _ffi.check(rc, entry)
        torch.cuda.synchronize()
    assert sorted(names) == lb.KERNELS[entry][path], names
    dq, dk, dv, dv_lp, D = dq.cpu(), dk.cpu(), dv.cpu(), dv_lp.cpu(), D.cpu()
    for name, t, key in (("dq", dq, "q"), ("dk", dk, "k"), ("dv", dv, "v"), ("dv_lp", dv_lp, "v")):
        assert _all_nan(lb.outside(t, st[key][1])), f"{c.tag} {path}: the backward wrote outside the head blocks of {name}"
    u = lambda t, key: lb.unpack(t, B, N, st[key][1])
    return u(dq, "q"), u(dk, "k"), u(dv, "v"), lb.unpack_rows(D, B, N), u(dv_lp, "v")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("N,W,regime", lb.CASES, ids=lb.IDS)
def test_kernels_within_fp64_bound(N, W, regime):
    c = lb.case(N, W, regime)
    buf = _Buffers(c)
    for path in lb.PATHS:
        lb.verify_forward(c, path, _forward(c, buf, path, "fwd"), RATIOS[path])
        lb.verify_backward(c, path, _backward(c, buf, path, "bwd"), RATIOS[path])
    _report()


@pytest.mark.parametrize("N,W", lb.DROP_CASES, ids=lb.DROP_IDS)
def test_dropout_kernels_within_fp64_bound(N, W):
    c = lb.case(N, W, "flat", True)
    buf = _Buffers(c)
    for path in lb.PATHS:
        lb.verify_forward(c, path, _forward(c, buf, path, "fwd_dropout", lb.DROP["p"]), RATIOS[path])
        lb.verify_backward(c, path, _backward(c, buf, path, "bwd_dropout", lb.DROP["p"]), RATIOS[path])
    _report()


@pytest.mark.parametrize("N,W", lb.DROP_CASES, ids=lb.DROP_IDS)
def test_dropout_entry_points_at_p0_give_the_bits_of_the_plain_ones(N, W):
    c = lb.case(N, W, "flat")
    buf = _Buffers(c)
    for path in lb.PATHS:
        for a, b in zip(_forward(c, buf, path, "fwd"), _forward(c, buf, path, "fwd_dropout", 0.0)):
            assert torch.equal(_bits(a), _bits(b)), f"{c.tag} {path}: forward"
        for a, b in zip(_backward(c, buf, path, "bwd"), _backward(c, buf, path, "bwd_dropout", 0.0)):
            assert torch.equal(_bits(a), _bits(b)), f"{c.tag} {path}: backward"


def test_the_debug_switch_selects_a_different_kernel():
    """the split kernel's o fails the EXACT bound where the exact kernel's o passes it: rows with few visible keys, where the exact path's chain is
    a handful of roundings and the split operands have lost their bits beyond hi + lo"""
    c = lb.case(23, 5, "flat")
    buf = _Buffers(c)
    exact_o = _forward(c, buf, "exact", "fwd")[0]
    split_o = _forward(c, buf, "split", "fwd")[0]
    ok_e, r_e = lb.nb.check(exact_o, c.fwd["o"], c.bounds["exact"]["o"])
    ok_s, r_s = lb.nb.check(split_o, c.fwd["o"], c.bounds["exact"]["o"])
    print(f"  {c.tag} o under the exact bound: exact kernel {r_e:.3g}, split kernel {r_s:.3g}")
    assert ok_e and not ok_s, (r_e, r_s)


@pytest.mark.parametrize("W,t,N", lb.STEP_CASES, ids=lb.STEP_IDS)
def test_decode_step_within_fp64_bound(W, t, N):
    from synthanatomy_amd import _ffi
    ops = lb.draw_step(W, t, N)
    B, inner = ops["B"], ops["inner"]
    qkv, cosb, sinb, kc, vc = (ops[n].to(DEV) for n in ("qkv", "cos", "sin", "kc", "vc"))
    pos = torch.tensor([t], dtype=torch.int32, device=DEV)
    out = torch.full((B, inner), float("nan"), device=DEV)
    g0 = lb.G * lb.DH
    with _ffi.kernel_log() as names:
        _ffi.check(_ffi.lib().sa_local_attn_step(_ffi.ptr(qkv), 3 * inner, g0, _ffi.ptr(qkv), 3 * inner, inner + g0, _ffi.ptr(qkv), 3 * inner, 2 * inner + g0,
                                                 _ffi.ptr(cosb), _ffi.ptr(sinb), _ffi.ptr(kc), _ffi.ptr(vc), _ffi.ptr(pos), B, N, lb.L, W, lb.DH, _ffi.ptr(out),
                                                 inner, g0, _ffi.stream()), "sa_local_attn_step")
        torch.cuda.synchronize()
    assert sorted(names) == lb.KERNELS["step"]["exact"], names
    out = out.cpu()
    assert _all_nan(out[:, :g0]) and int(pos.item()) == t
    lb.verify_step(ops, (out[:, g0:].reshape(B, lb.L, lb.DH), kc.cpu(), vc.cpu()), RATIOS["step"])
    _report()


def test_fill_la_refuses_what_the_header_says_it_refuses():
    """N * max(stride) * 4 >= 2^31 -> SA_EUNSUPPORTED; a stride or offset that is no multiple of 4 -> SA_EINVAL.  Both return before any launch: the
    buffers are tiny, the oversized N / stride are integers only."""
    from synthanatomy_amd import _ffi
    lib = _ffi.lib()
    t = torch.zeros(4096, device=DEV)
    p = _ffi.ptr(t)

    def fwd(N=4, qs=128, qo=0, ks=128, ko=0, vs=128, vo=0, os_=128, oo=0):
        with _ffi.kernel_log() as names:
            rc = lib.sa_local_attn_fwd(p, qs, qo, p, ks, ko, p, vs, vo, p, os_, oo, p, 1, N, 2, 4, 64, None, _ffi.stream())
        assert names == [], names
        return rc

    def bwd(N=4, vs=128, oo=0):
        with _ffi.kernel_log() as names:
            rc = lib.sa_local_attn_bwd(p, 128, 0, p, 128, 0, p, vs, 0, p, p, 128, oo, p, p, p, p, p, 1, N, 2, 4, 64, None, _ffi.stream())
        assert names == [], names
        return rc

    big = (1 << 29) // 576                                  # N * 576 * 4 just below 2^31 at `big`, at or above it at big + 1
    assert big * 576 * 4 < 1 << 31 <= (big + 1) * 576 * 4
    assert fwd(N=big + 1, vs=576) == SA_EUNSUPPORTED and bwd(N=big + 1, vs=576) == SA_EUNSUPPORTED
    assert fwd(N=(1 << 29) // 128, qs=128) == SA_EUNSUPPORTED          # exactly 2^31
    for kw in (dict(qs=130), dict(qo=2), dict(ks=129), dict(ko=1), dict(vs=131), dict(vo=3), dict(os_=134), dict(oo=6)):
        assert fwd(**kw) == SA_EINVAL, kw
    assert bwd(oo=2) == SA_EINVAL
    torch.cuda.synchronize()
    assert bool((t == 0).all())
