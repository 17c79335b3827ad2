"""GPU: the fused FAVOR+ kernels (csrc/favor_fused.hip) through the C ABI -- sa_favor_fused_proj_tiles, _prepass, _fwd, _bwd -- in the engine's layout
(q | k | v head blocks inside wider rows whose foreign columns hold NaN), against the fp64 references under the element-wise bounds of
tests/favor_bounds.py: the pre-pass outputs, out, inv, attn_lp, dden, the per-block partial sums, dq, dk, dv, their bf16 mirrors and the row the
fix-up rewrites, with the planted-defect witnesses the same output must fail.  Every case runs both forms of the chunk states (or the dispatcher's
own sequential route at B G >= 40) and the backward with the forward's states and with state_fwd = NULL; the launches are asserted by name.  Output
buffers start as NaN and must still hold those bits outside the global heads' columns.  Run with -s to read every max |err| / bound."""
import contextlib
import struct

import pytest
import torch

import favor_bounds as fb

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(16, torch.get_num_threads()))
DEV = "cuda"
LOCAL_COLS = 64                                              # one local-window head's columns behind the global heads
RATIOS = {}                                                  # output -> worst max |err| / bound so far (the checks themselves assert <= 1 element-wise)


def _report():
    print("worst max |err| / bound so far:", {k: float(f"{v:.3g}") for k, v in RATIOS.items()})


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _untouched(t, G):
    """the columns behind the global heads still hold the NaN bits the buffer started with"""
    rest = fb.outside(t.cpu(), G)
    want = torch.full_like(rest, float("nan"))
    view = torch.int32 if t.dtype == torch.float32 else torch.int16
    return torch.equal(rest.contiguous().view(view), want.view(view))


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16 if t.dtype == torch.bfloat16 else t.dtype)


class _Device:
    """the operands of a case on the device, the projection tiles and the pre-pass outputs"""

    def __init__(self, c):
        from synthanatomy_amd import _ffi
        self.c = c
        lib, st = _ffi.lib(), _ffi.stream()
        B, G, N, m = c.B, c.G, c.N, c.m
        self.inner = inner = G * fb.DH + LOCAL_COLS
        self.stride = stride = 3 * inner
        self.R = R = B * N
        qkv = torch.full((R, stride), float("nan"))
        for n, name in enumerate(("q", "k", "v")):
            qkv[:, n * inner: n * inner + G * fb.DH] = fb.pack(c.ops[name], G * fb.DH, 0)
        self.qkv = qkv.to(DEV)
        self.q, self.k, self.v = (self.qkv[:, n * inner: (n + 1) * inner] for n in range(3))
        self.ps = c.ops["Ps"].to(DEV)
        self.tiles = torch.empty(5 * 16384, dtype=torch.uint8, device=DEV)
        with _ffi.kernel_log() as names:
            _ffi.check(lib.sa_favor_fused_proj_tiles(_ffi.ptr(self.ps), m, _ffi.ptr(self.tiles), st))
            torch.cuda.synchronize()
        assert sorted(names) == fb.KERNELS["proj_tiles"]["parallel"], names
        self.flag = int(self.tiles[-16:].view(torch.int32)[0])
        assert self.flag == (0 if c.bf16 else 1), f"{c.tag}: flag word {self.flag}"
        self.offq, self.offk = _nan((R * G,)), _nan((R * G,))
        self.amq = torch.full((R * G,), -1, dtype=torch.int32, device=DEV)
        self.gws = torch.zeros(1, dtype=torch.int64, device=DEV)
        with _ffi.kernel_log() as names:
            _ffi.check(lib.sa_favor_fused_prepass(_ffi.ptr(self.q), _ffi.ptr(self.k), stride, G, _ffi.ptr(self.tiles), _ffi.ptr(self.offq), _ffi.ptr(self.amq),
                                                  _ffi.ptr(self.offk), _ffi.ptr(self.gws), R * G, m, fb.DH, st))
            torch.cuda.synchronize()
        assert sorted(names) == fb.KERNELS["prepass"]["parallel"], names
        self.da = fb.pack(c.ops["dattn"], inner, 0).to(DEV)
        self.nst = lib.sa_favor_fused_state_bytes(B, N, G, m) // 4

    def prepass_outputs(self):
        """(offq, offk, amq [B, G, N], gmax value, gmax flat index): pack_max's order-preserving bits above, the inverted index below"""
        c = self.c
        word = int(self.gws.cpu()[0]) & 0xFFFFFFFFFFFFFFFF
        u = word >> 32
        u = (u & 0x7FFFFFFF) if (u & 0x80000000) else (~u & 0xFFFFFFFF)
        gval = struct.unpack("<f", struct.pack("<I", u))[0]
        gidx = 0xFFFFFFFF - (word & 0xFFFFFFFF)
        un = lambda t: fb.unpack_rows(t.cpu(), c.B, c.G, c.N)
        return un(self.offq), un(self.offk), un(self.amq), gval, gidx

    def forward(self, route):
        from synthanatomy_amd import _ffi
        c, lib = self.c, _ffi.lib()
        B, G, N, m, R, inner = c.B, c.G, c.N, c.m, self.R, self.inner
        state = torch.zeros(self.nst, device=DEV)
        attn, attn_lp, inv = _nan((R, inner)), _nan((R, inner), torch.bfloat16), _nan((R * G,))
        with _ffi.kernel_log() as names:
            _ffi.check(lib.sa_favor_fused_fwd(_ffi.ptr(self.q), _ffi.ptr(self.k), _ffi.ptr(self.v), self.stride, _ffi.ptr(self.tiles), _ffi.ptr(self.ps), _ffi.ptr(self.offq),
                                              _ffi.ptr(self.offk), _ffi.ptr(self.gws), _ffi.ptr(attn), inner, _ffi.ptr(inv), 1e-6, B, N, G, m, _ffi.ptr(state),
                                              _ffi.ptr(attn_lp), None, _ffi.stream()))
            torch.cuda.synchronize()
        assert sorted(names) == fb.KERNELS["fwd"][route], names
        assert _untouched(attn, G) and _untouched(attn_lp, G), f"{c.tag}: the forward wrote outside the global heads' columns"
        return (fb.unpack(attn.cpu(), B, G, N), fb.unpack_rows(inv.cpu(), B, G, N), fb.unpack(attn_lp.cpu(), B, G, N)), state

    def backward(self, route, attn32, inv32, state_fwd):
        """one sa_favor_fused_bwd that is given attn32 / inv32 (and the forward's states, or NULL)"""
        from synthanatomy_amd import _ffi
        c, lib = self.c, _ffi.lib()
        B, G, N, m, R, inner, stride = c.B, c.G, c.N, c.m, self.R, self.inner, self.stride
        attn = fb.pack(attn32, inner, 0).to(DEV)
        inv = fb.pack_rows(inv32).to(DEV)
        dqkv, dqkv_lp = _nan((R, stride)), _nan((R, stride), torch.bfloat16)
        dq, dk, dv = (dqkv[:, n * inner: (n + 1) * inner] for n in range(3))
        dq_lp, dk_lp, dv_lp = (dqkv_lp[:, n * inner: (n + 1) * inner] for n in range(3))
        ws, dden, tsum = torch.zeros(self.nst, device=DEV), _nan((R * G,)), _nan((B * G * c.S,))
        with _ffi.kernel_log() as names:
            _ffi.check(lib.sa_favor_fused_bwd(_ffi.ptr(self.q), _ffi.ptr(self.k), _ffi.ptr(self.v), stride, _ffi.ptr(self.tiles), _ffi.ptr(self.ps), _ffi.ptr(self.offq),
                                              _ffi.ptr(self.amq), _ffi.ptr(self.offk), _ffi.ptr(self.gws), _ffi.ptr(self.da), _ffi.ptr(attn), inner, _ffi.ptr(inv),
                                              _ffi.ptr(dq), _ffi.ptr(dk), _ffi.ptr(dv), B, N, G, m, None if state_fwd is None else _ffi.ptr(state_fwd), _ffi.ptr(ws),
                                              _ffi.ptr(dden), _ffi.ptr(tsum), _ffi.ptr(dq_lp), _ffi.ptr(dk_lp), _ffi.ptr(dv_lp), None, _ffi.stream()))
            torch.cuda.synchronize()
        assert sorted(names) == fb.KERNELS["bwd_state_null" if state_fwd is None else "bwd_state_kept"][route], names
        for name, t in (("dq", dq), ("dk", dk), ("dv", dv), ("dq_lp", dq_lp), ("dk_lp", dk_lp), ("dv_lp", dv_lp)):
            assert _untouched(t, G), f"{c.tag}: the backward wrote outside the global heads' columns of {name}"
        u = lambda t: fb.unpack(t.cpu(), B, G, N)
        return fb.unpack_rows(dden.cpu(), B, G, N), u(dq), u(dk), u(dv), (u(dq_lp), u(dk_lp), u(dv_lp)), tsum.cpu()


@pytest.mark.parametrize("B,G,N,m,regime,bf16", fb.CASES, ids=fb.IDS)
def test_kernels_within_fp64_bound(B, G, N, m, regime, bf16):
    from synthanatomy_amd import debug
    c = fb.case(B, G, N, m, regime, bf16)
    dev = _Device(c)
    pre = fb.verify_prepass(c, dev.prepass_outputs(), RATIOS)
    st = fb.Stage(c, pre)
    for route, seq in fb.routes(B, G):
        with (contextlib.nullcontext() if seq is None else debug.override(favor_seq_always=seq)):
            fwd, state = dev.forward(route)
            st.verify_forward(fwd, RATIOS)
            kept = dev.backward(route, st.attn32, st.inv32, state)
            st.verify_backward(kept, RATIOS)
            rebuilt = dev.backward(route, st.attn32, st.inv32, None)
        flat = lambda r: (r[0], r[1], r[2], r[3], *r[4], r[5])
        for name, a, b in zip(("dden", "dq", "dk", "dv", "dq_lp", "dk_lp", "dv_lp", "tsum"), flat(kept), flat(rebuilt)):
            assert torch.equal(_bits(a), _bits(b)), f"{c.tag} {route}: {name} differs between the forward's states and state_fwd = NULL"
    _report()

