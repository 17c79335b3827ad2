"""ff_dropout / attn_dropout of the Performer on the GPU (reference run_transformer.py:83-84, src/networks/transformers/performer.py:95-96,212-213):
the counter-based masks of csrc/dropout.h against their Python restatement, the local-window attention dropout kernels on both arithmetic paths against an
fp64 band softmax with the replayed mask, and the whole network (fp32 and bf16 modes, ReZero and pre-LayerNorm) against oracle/performer_ref.py pieces
with the replayed masks of every site."""
import glob
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dropout_ref import keep_mask, scaled_mask  # noqa: E402
from oracle import performer_ref as P  # noqa: E402


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------ the keep function
def test_dropout_mask_matches_restatement():
    from synthanatomy_amd import _ffi
    lib, st = _ffi.lib(), _ffi.stream()
    n = 100003
    out = torch.empty(n, device="cuda")
    masks = {}
    for p in (0.1, 0.5):
        for seed, site in ((0x0123456789ABCDEF, 0), (0x0123456789ABCDEF, 1), (7, 0)):
            _ffi.check(lib.sa_dropout_mask(_ffi.ptr(out), n, p, seed, site, 1, st), "sa_dropout_mask")
            got = out.cpu().numpy()
            ref = scaled_mask(seed, site, (n,), p)
            assert np.array_equal(got, ref), (p, seed, site)
            frac = float((got > 0).mean())
            assert abs(frac - (1 - p)) < 4 * math.sqrt(p * (1 - p) / n), (p, frac)
            masks[(p, seed, site)] = got > 0
        _ffi.check(lib.sa_dropout_mask(_ffi.ptr(out), n, p, 7, 0, 0, st), "sa_dropout_mask")
        assert np.array_equal(out.cpu().numpy(), keep_mask(7, 0, 0, n, p).astype(np.float32))
    keys = list(masks)
    for i in range(len(keys)):
        for j in range(i + 1, len(keys)):
            if keys[i][0] == keys[j][0]:
                assert not np.array_equal(masks[keys[i]], masks[keys[j]]), (keys[i], keys[j])
    assert lib.sa_dropout_mask(_ffi.ptr(out), n, 1.0, 0, 0, 1, st) == _ffi.SA_EINVAL


# ------------------------------------------------------------------------------------------------ local-window attention kernels
@pytest.fixture(params=["split-bf16", "exact-fp32"])
def la_path(request):
    from synthanatomy_amd import debug
    with debug.override(local_attn_exact=request.param == "exact-fp32"):
        yield request.param


def _band_dropout_ref(q, k, v, W, Z):
    """fp64: softmax over the causal window (one window back), times the scaled keep mask Z [B, L, N, N], times v"""
    n, e = q.shape[-2], q.shape[-1]
    dots = torch.einsum("...ie,...je->...ij", q, k) * (e ** -0.5)
    i = torch.arange(n)[:, None]
    j = torch.arange(n)[None, :]
    lo = (i // W - 1).clamp(min=0) * W
    allowed = (j <= i) & (j >= lo)
    dots = dots.masked_fill(~allowed, float("-inf"))
    pr = dots.softmax(dim=-1)
    return (pr * Z) @ v, torch.logsumexp(dots, dim=-1)


@pytest.mark.parametrize("N,W", [(102, 40), (130, 70), (200, 64), (64, 96)])
def test_local_attention_dropout_kernels_against_fp64_band(N, W, la_path):
    from synthanatomy_amd import _ffi
    lib, st = _ffi.lib(), _ffi.stream()
    torch.manual_seed(N + W)
    B, L, dh, p, seed, site = 2, 2, 64, 0.3, 0x5EED5EED12345678, 6
    q, k, v, do = (torch.randn(B, L, N, dh, dtype=torch.float64) for _ in range(4))
    Z = torch.from_numpy(scaled_mask(seed, site, (B, L, N, N), p)).double()
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    ref, ref_lse = _band_dropout_ref(qr, kr, vr, W, Z)
    (ref * do).sum().backward()
    pack = lambda t: t.permute(0, 2, 1, 3).reshape(B * N, L * dh).float().contiguous().cuda()
    unpack = lambda t: t.view(B, N, L, dh).permute(0, 2, 1, 3)
    qd, kd, vd, dod = pack(q), pack(k), pack(v), pack(do)
    o, o0 = torch.empty_like(qd), torch.empty_like(qd)
    lse, lse0 = torch.empty(B * N * L, device="cuda"), torch.empty(B * N * L, device="cuda")
    s = L * dh
    _ffi.check(lib.sa_local_attn_fwd_dropout(_ffi.ptr(qd), s, 0, _ffi.ptr(kd), s, 0, _ffi.ptr(vd), s, 0, _ffi.ptr(o), s, 0, _ffi.ptr(lse), B, N, L, W, dh, None,
                                             p, seed, site, st), "sa_local_attn_fwd_dropout")
    _ffi.check(lib.sa_local_attn_fwd(_ffi.ptr(qd), s, 0, _ffi.ptr(kd), s, 0, _ffi.ptr(vd), s, 0, _ffi.ptr(o0), s, 0, _ffi.ptr(lse0), B, N, L, W, dh, None, st),
               "sa_local_attn_fwd")
    dq, dk, dv = torch.empty_like(qd), torch.empty_like(qd), torch.empty_like(qd)
    Db = torch.empty(B * N * L, device="cuda")
    _ffi.check(lib.sa_local_attn_bwd_dropout(_ffi.ptr(qd), s, 0, _ffi.ptr(kd), s, 0, _ffi.ptr(vd), s, 0, _ffi.ptr(o), _ffi.ptr(dod), s, 0, _ffi.ptr(lse),
                                             _ffi.ptr(dq), _ffi.ptr(dk), _ffi.ptr(dv), _ffi.ptr(Db), B, N, L, W, dh, None, p, seed, site, st),
               "sa_local_attn_bwd_dropout")
    torch.cuda.synchronize()
    assert torch.allclose(lse, lse0, rtol=1e-6, atol=1e-6)          # lse is the undropped softmax's
    assert _rel(lse.view(B, N, L).permute(0, 2, 1), ref_lse) < 1e-5
    assert _rel(unpack(o), ref) < 1e-4, _rel(unpack(o), ref)
    for name, got, r in (("dq", dq, qr.grad), ("dk", dk, kr.grad), ("dv", dv, vr.grad)):
        assert _rel(unpack(got), r) < 2e-4, (name, _rel(unpack(got), r))
    assert not torch.allclose(o, o0)


# ------------------------------------------------------------------------------------------------ the network
SHAPE = (2, 3, 4)
N_SEQ = 24


def _cfg(rezero, local):
    return P.PerformerConfig(num_tokens=33, max_seq_len=N_SEQ, dim=32, depth=2, heads=4, dim_head=64, local_attn_heads=local, local_window_size=6,
                             spatial_shape=SHAPE, use_rezero=rezero)


def _net(cfg, st, dtype, pf, pa):
    from synthanatomy_amd.networks.transformers.img2seq_ordering import Ordering
    from synthanatomy_amd.networks.transformers.performer import Performer
    o = Ordering("raster_scan", 3, (1,) + SHAPE, (False,) * 3, (), ())
    net = Performer(num_tokens=33, max_seq_len=N_SEQ, dim=32, depth=2, heads=4, ordering=o, dim_head=64, local_attn_heads=cfg.local_attn_heads,
                    local_window_size=6, use_rezero=cfg.use_rezero, spatial_position_emb="absolute", spatial_shape=SHAPE, feature_redraw_interval=None,
                    compute_dtype=dtype, ff_dropout=pf, attn_dropout=pa)
    missing, unexpected = net.load_state_dict({k: v.clone() for k, v in st.items()}, strict=False)
    assert not unexpected, unexpected
    return net.cuda().train(), o


def _state(cfg):
    st = P.init_state(cfg, seed=5, spatial_index_len=N_SEQ - 1)
    for k in st:
        if k.endswith(".g"):
            st[k] = torch.tensor(0.4)
    return st


def _ref_self_attention(st, p, cfg, x, Zloc):
    b, n, _ = x.shape
    h, gh = cfg.heads, cfg.heads - cfg.local_attn_heads
    q = F.linear(x, st[p + ".to_q.weight"], st.get(p + ".to_q.bias"))
    k = F.linear(x, st[p + ".to_k.weight"], st.get(p + ".to_k.bias"))
    v = F.linear(x, st[p + ".to_v.weight"], st.get(p + ".to_v.bias"))
    q, k, v = (t.reshape(b, n, h, cfg.dim_head).permute(0, 2, 1, 3) for t in (q, k, v))
    outs = []
    if gh > 0:      # FAVOR+ heads: no dropout (performer_pytorch FastAttention)
        proj = st[p + ".fast_attention.projection_matrix"]
        outs.append(P.causal_linear_attention(P.softmax_kernel(q[:, :gh], proj, True), P.softmax_kernel(k[:, :gh], proj, False), v[:, :gh]))
    if gh < h:      # LocalAttention(dropout=attn_dropout): dropout(softmax(dots)) @ v
        ql, kl, vl = q[:, gh:], k[:, gh:], v[:, gh:]
        e = ql.shape[-1]
        cos, sin = P.rotary_tables(n, e)
        ql, kl = P.apply_rotary(ql, cos, sin), P.apply_rotary(kl, cos, sin)
        dots = torch.einsum("...ie,...je->...ij", ql, kl) * (e ** -0.5)
        i = torch.arange(n)[:, None]
        j = torch.arange(n)[None, :]
        lo = (i // cfg.local_window_size - 1).clamp(min=0) * cfg.local_window_size
        dots = dots.masked_fill(~((j <= i) & (j >= lo)), -torch.finfo(dots.dtype).max)
        outs.append((dots.softmax(dim=-1) * Zloc) @ vl)
    out = torch.cat(outs, dim=1).permute(0, 2, 1, 3).reshape(b, n, h * cfg.dim_head)
    return F.linear(out, st[p + ".to_out.weight"], st.get(p + ".to_out.bias"))


def _ref_forward(st, cfg, tok, seqs, seed, pf, pa):
    """oracle/performer_ref.forward with the three dropout sites of every layer replayed from `seed` (sites 4 i + 0 / 1 / 2)"""
    x = P.embed(st, cfg, tok, seqs)
    b, n, d = x.shape
    L = cfg.local_attn_heads
    for i in range(cfg.depth):
        p = f"performer.net.layers.{i}"
        Zff = torch.from_numpy(scaled_mask(seed, 4 * i, (b, n, 4 * d), pf))
        Zout = torch.from_numpy(scaled_mask(seed, 4 * i + 1, (b, n, d), pa))
        Zloc = torch.from_numpy(scaled_mask(seed, 4 * i + 2, (b, L, n, n), pa)) if L else None
        xa = x if cfg.use_rezero else F.layer_norm(x, (d,), st[p + ".0.norm.weight"], st[p + ".0.norm.bias"])
        Fa = _ref_self_attention(st, p + ".0.fn", cfg, xa, Zloc) * Zout
        x = x + Fa * st[p + ".0.g"] if cfg.use_rezero else x + Fa
        xf = x if cfg.use_rezero else F.layer_norm(x, (d,), st[p + ".1.norm.weight"], st[p + ".1.norm.bias"])
        q = p + ".1.fn.fn"
        Ff = F.linear(F.gelu(F.linear(xf, st[q + ".w1.weight"], st[q + ".w1.bias"])) * Zff, st[q + ".w2.weight"], st[q + ".w2.bias"])
        x = x + Ff * st[p + ".1.g"] if cfg.use_rezero else x + Ff
    x = F.layer_norm(x, (d,), st["norm.weight"], st["norm.bias"])
    return F.linear(x, st["to_out.weight"], st["to_out.bias"])


def _step(net, tok, tgt, seed):
    from synthanatomy_amd.losses.transformer import CELoss
    net.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    out = net(tok)
    loss = CELoss()(out.transpose(1, 2), tgt)
    loss.backward()
    torch.cuda.synchronize()
    return out, loss


@pytest.mark.parametrize("rezero,local", [(True, 2), (False, 2), (True, 4), (False, 0)])
def test_fp32_network_with_dropout_matches_restatement(rezero, local):
    cfg = _cfg(rezero, local)
    st = _state(cfg)
    pf, pa = 0.2, 0.3
    net, o = _net(cfg, st, torch.float32, pf, pa)
    g = torch.Generator().manual_seed(9)
    tok = torch.randint(0, 33, (2, N_SEQ), generator=g)
    tgt = torch.randint(0, 32, (2, N_SEQ), generator=g)
    out, _ = _step(net, tok.cuda(), tgt.cuda(), 11)
    seed = net.last_dropout_seed
    assert seed is not None
    seqs = P.spatial_index_sequences(SHAPE, o.get_sequence_ordering())
    leaf = {k: v.clone().requires_grad_(True) for k, v in st.items() if "projection_matrix" not in k}
    stt = dict(st)
    stt.update(leaf)
    ref = _ref_forward(stt, cfg, tok, seqs, seed, pf, pa)
    P.ce_loss(ref, tgt).backward()
    assert _rel(out, ref) < 1e-3, _rel(out, ref)
    # the same network without the masks is far away: the dropout is on
    with torch.no_grad():
        assert _rel(out, P.forward(st, cfg, tok, seqs)) > 1e-2
    params = dict(net.named_parameters())
    checked = 0
    for k, p in leaf.items():
        if k in params and p.grad is not None and float(p.grad.abs().max()) > 0:
            assert params[k].grad is not None, k
            assert _rel(params[k].grad, p.grad) < 3e-3, (k, _rel(params[k].grad, p.grad))
            checked += 1
    assert checked > 15


@pytest.mark.parametrize("rezero", [True, False])
def test_bf16_network_with_dropout_against_fp32(rezero):
    cfg = _cfg(rezero, 2)
    st = _state(cfg)
    net32, _ = _net(cfg, st, torch.float32, 0.2, 0.3)
    net16, _ = _net(cfg, st, torch.bfloat16, 0.2, 0.3)
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(0, 33, (2, N_SEQ), generator=g).cuda()
    tgt = torch.randint(0, 32, (2, N_SEQ), generator=g).cuda()
    o32, _ = _step(net32, tok, tgt, 21)
    o16, _ = _step(net16, tok, tgt, 21)
    assert net32.last_dropout_seed == net16.last_dropout_seed
    assert _rel(o16, o32) < 2e-2, _rel(o16, o32)
    p32, p16 = dict(net32.named_parameters()), dict(net16.named_parameters())
    for k in p32:
        if p32[k].grad is not None and float(p32[k].grad.abs().max()) > 0:
            assert _rel(p16[k].grad, p32[k].grad) < 6e-2, (k, _rel(p16[k].grad, p32[k].grad))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_eval_is_the_identity(dtype):
    cfg = _cfg(True, 2)
    st = _state(cfg)
    net, _ = _net(cfg, st, dtype, 0.2, 0.3)
    net0, _ = _net(cfg, st, dtype, 0.0, 0.0)
    tok = torch.randint(0, 33, (2, N_SEQ), generator=torch.Generator().manual_seed(4)).cuda()
    net.eval()
    net0.eval()
    with torch.no_grad():
        a, b = net(tok), net0(tok)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert net.last_dropout_seed is None


def test_seeded_steps_are_reproducible():
    from synthanatomy_amd import debug
    cfg = _cfg(True, 2)
    st = _state(cfg)
    net, _ = _net(cfg, st, torch.bfloat16, 0.1, 0.1)
    g = torch.Generator().manual_seed(8)
    tok = torch.randint(0, 33, (2, N_SEQ), generator=g).cuda()
    tgt = torch.randint(0, 32, (2, N_SEQ), generator=g).cuda()
    was = debug.deterministic()
    debug.set_deterministic(True)
    try:
        runs = []
        for seed in (0, 0, 1):
            _, loss = _step(net, tok, tgt, seed)
            runs.append((loss.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}))
    finally:
        debug.set_deterministic(was)
    (l0, g0), (l1, g1), (l2, g2) = runs
    assert torch.equal(l0, l1) and all(torch.equal(g0[k], g1[k]) for k in g0)
    assert not torch.equal(l0, l2) and any(not torch.equal(g0[k], g2[k]) for k in g0)


def test_run_transformer_trains_with_dropout(tmp_path):
    import run_transformer
    proj = str(tmp_path) + "/"
    codes = tmp_path / "codes"
    codes.mkdir()
    rng = np.random.default_rng(0)
    for i in range(4):
        np.save(codes / f"s{i}_quantization_0.npy", rng.integers(0, 64, size=(4, 6, 4)).astype(np.uint16))
    code_dir = str(codes) + "/*_quantization_0.npy"
    tr = ["--project_directory=" + proj, "--experiment_name=drop", "--vocab_size=64", "--n_embd=64", "--n_layers=2", "--n_head=2", "--local_attn_heads=1",
          "--local_window_size=24", "--use_rezero=True", "--spatial_position_emb=absolute", "--feature_redraw_interval=1", "--batch_size=2",
          "--eval_batch_size=2", "--log_every=1", "--learning_rate=1e-3", "--ordering_type=hilbert_curve", "--ff_dropout=0.1", "--attn_dropout=0.1"]
    run_transformer.run(tr + ["--training_subjects=" + code_dir, "--validation_subjects=" + code_dir, "--mode=training", "--epochs=2", "--checkpoint_every=1"])
    ck = glob.glob(proj + "drop/performer/checkpoints/checkpoint_epoch=2.pt")
    assert ck
    sd = torch.load(ck[0], map_location="cpu", weights_only=False)
    assert all(torch.isfinite(v).all() for v in sd["network"].values() if v.is_floating_point())
