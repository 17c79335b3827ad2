"""GPU: generalized (ReLU) attention -- csrc/favor_generalized.hip and its wiring through training, sampling, healing and the CLI -- against the fp64
restatement of tests/generalized_ref.py (OUR restatement of performer-pytorch 1.0.11 generalized_kernel; parity with upstream is unpinned).

Bounds are the ones the softmax map is already held to: 2e-5 (split-bf16 projection, test_projection_kernels_against_matmul: the map is 1-Lipschitz, the
mask selects terms, so the projection's bound carries over), REL = 1e-3 on logits / 3e-3 on gradients (test_forward_and_gradients_match_oracle), 3e-2 on
throughput-mode logits, 5e-2 on bf16 gradients.  Outputs are pre-filled with NaN so that untouched memory shows."""
import glob

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from generalized_ref import as_softmax_kernel, generalized_kernel  # noqa: E402
from oracle import performer_ref as P  # noqa: E402

REL = 1e-3
NAN = float("nan")


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def _eps32():
    return torch.tensor(1e-3, dtype=torch.float32, device="cuda")


def _ffi():
    from synthanatomy_amd import _ffi
    return _ffi, _ffi.lib(), _ffi.stream()


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("rows,m,LDF", [(1, 266, 272), (130, 100, 112), (77, 256, 256)])
def test_elementwise_pair_is_bitwise(rows, m, LDF):
    F, lib, st = _ffi()
    torch.manual_seed(rows + m)
    dd = torch.randn(rows, LDF, device="cuda")
    flat = dd.view(-1)
    flat[::7] = 0.0
    flat[1::11] = 1e-12         # relu(dd) + 1e-3f rounds to 1e-3f: the stored feature says "not above the kink"
    flat[2::13] = -1e-12
    flat[3::17] = -0.0
    assert bool((dd < 0).any()) and bool((dd == 0).any())
    feat = torch.full((rows, LDF), NAN, device="cuda")
    F.check(lib.sa_favor_generalized_features_fwd(F.ptr(dd), F.ptr(feat), rows, m, LDF, st))
    want = torch.relu(dd) + _eps32()
    assert want.dtype == torch.float32 and torch.equal(feat[:, :m], want[:, :m])
    assert LDF == m or float(feat[:, m:].abs().max()) == 0.0
    assert bool((feat[:, :m][dd[:, :m] == 1e-12] == _eps32()).all())
    dfeat = torch.randn(rows, LDF, device="cuda")
    dfeat[:, m:] = 7.0          # padded gradient columns must not leak
    ddd = torch.full((rows, LDF), NAN, device="cuda")
    F.check(lib.sa_favor_generalized_features_bwd(F.ptr(dfeat), F.ptr(feat), F.ptr(ddd), rows, m, LDF, st))
    assert torch.equal(ddd[:, :m], dfeat[:, :m] * (feat[:, :m] > _eps32()))
    assert LDF == m or float(ddd[:, m:].abs().max()) == 0.0
    # the mask comes from the stored feature, whatever the padded columns of it hold
    feat2 = feat.clone()
    feat2[:, m:] = 0.5
    ddd2 = torch.full((rows, LDF), NAN, device="cuda")
    F.check(lib.sa_favor_generalized_features_bwd(F.ptr(dfeat), F.ptr(feat2), F.ptr(ddd2), rows, m, LDF, st))
    assert torch.equal(ddd2, ddd)


SHAPES = [(1, 266, 272, 1), (130, 266, 272, 2), (1000, 100, 112, 1), (77, 256, 256, 1)]


@pytest.mark.parametrize("rows,m,LDF,heads", SHAPES)
def test_fused_forward_against_fp64(rows, m, LDF, heads):
    F, lib, st = _ffi()
    torch.manual_seed(rows + m)
    wide, R = heads * 64 + 32, rows // heads             # head blocks live in a wider matrix
    xw = torch.randn(2, R, wide, device="cuda")          # two operands, R * wide elements apart
    P_ = torch.randn(m, 64, device="cuda") * 0.35
    single = []
    for gi in range(2):
        feat = torch.full((rows, LDF), NAN, device="cuda")
        F.check(lib.sa_favor_generalized_project_features(F.ptr(xw[gi]), wide, heads, F.ptr(P_), F.ptr(feat), rows, m, LDF, 64, 1, 0, 0, st))
        x = xw[gi, :, :heads * 64].reshape(rows, 64)
        ref = torch.relu(x.double() @ P_.double().t()) + 1e-3
        err = _rel(feat[:, :m], ref)
        print(f"  operand {gi}: max relative error {err:.3g}")
        assert err < 2e-5
        assert LDF == m or float(feat[:, m:].abs().max()) == 0.0
        single.append(feat)
    both = torch.full((2, rows, LDF), NAN, device="cuda")
    F.check(lib.sa_favor_generalized_project_features(F.ptr(xw), wide, heads, F.ptr(P_), F.ptr(both), rows, m, LDF, 64, 2, R * wide, rows * LDF, st))
    assert torch.equal(both[0], single[0]) and torch.equal(both[1], single[1])


@pytest.mark.parametrize("rows,m,LDF,heads", SHAPES)
def test_fused_backward_against_fp64(rows, m, LDF, heads):
    F, lib, st = _ffi()
    torch.manual_seed(rows + m + 1)
    wide, R = heads * 64 + 32, rows // heads
    eps = _eps32()
    P_ = torch.randn(m, 64, device="cuda") * 0.35
    # feat is an INPUT here: random above the kink, a planted share exactly AT 1e-3f (mask 0) and some one ulp above it (mask 1)
    feat = torch.rand(2, rows, LDF, device="cuda") + eps
    flat = feat.view(-1)
    flat[::3] = eps
    flat[1::5] = torch.nextafter(eps, torch.tensor(1.0, device="cuda"))
    feat[:, :, m:] = 0.5        # above the kink in the padded columns, with 7.0 as their gradient: only the column test keeps them out
    dfeat = torch.randn(2, rows, LDF, device="cuda")
    dfeat[:, :, m:] = 7.0
    assert bool((feat[:, :, :m] == eps).any()) and bool((feat[:, :, :m] > eps).any())
    single = []
    for gi in range(2):
        dxw = torch.full((R, wide), NAN, device="cuda")
        F.check(lib.sa_favor_generalized_project_bwd(F.ptr(dfeat[gi]), F.ptr(feat[gi]), F.ptr(P_), F.ptr(dxw), wide, heads, rows, m, LDF, 64, 1, 0, 0, st))
        ref = (dfeat[gi, :, :m].double() * (feat[gi, :, :m] > eps).double()) @ P_.double()
        err = _rel(dxw[:, :heads * 64].reshape(rows, 64), ref)
        print(f"  operand {gi}: max relative error {err:.3g}")
        assert err < 2e-5
        assert bool(torch.isnan(dxw[:, heads * 64:]).all())        # nothing outside the head blocks is touched
        single.append(dxw)
    both = torch.full((2, R, wide), NAN, device="cuda")
    F.check(lib.sa_favor_generalized_project_bwd(F.ptr(dfeat), F.ptr(feat), F.ptr(P_), F.ptr(both), wide, heads, rows, m, LDF, 64, 2, rows * LDF, R * wide, st))
    for gi in range(2):
        assert torch.equal(both[gi, :, :heads * 64], single[gi][:, :heads * 64]) and bool(torch.isnan(both[gi, :, heads * 64:]).all())


@pytest.mark.parametrize("B,G,m,LDF,N", [(2, 2, 266, 272, 37), (1, 3, 100, 112, 70)])
def test_step_kernel_against_the_quadratic_form(B, G, m, LDF, N):
    """N sequential calls of the decode step against the fp64 quadratic form of the rule at every position; REL is the bound this suite holds logits to
    (tests/test_performer_gpu.py), per position against that position's largest output."""
    F, lib, st = _ffi()
    torch.manual_seed(B + N)
    inner = (G + 1) * 64                                # one more head block behind the global heads, as a layer with a local head has
    qkv = torch.randn(N, B, 3 * inner, device="cuda")
    P_ = torch.randn(m, 64, device="cuda") * 0.35
    pos = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run():
        dd = torch.zeros(2, B * G, LDF, device="cuda")
        E = torch.zeros(B * G, LDF * 64, device="cuda")
        Ez = torch.zeros(B * G, LDF, device="cuda")
        out = torch.full((N, B, inner), NAN, device="cuda")
        for t in range(N):
            F.check(lib.sa_favor_generalized_step(F.ptr(qkv[t]), 3 * inner, 0, F.ptr(qkv[t]), 3 * inner, inner, F.ptr(qkv[t]), 3 * inner, 2 * inner, F.ptr(P_),
                                                  B, G, 64, m, LDF, F.ptr(dd), F.ptr(E), F.ptr(Ez), F.ptr(pos), F.ptr(out[t]), inner, 0, st))
        return out, E, Ez

    out, E, Ez = run()
    q, k, v = (qkv[:, :, i * inner: i * inner + G * 64].reshape(N, B, G, 64).permute(1, 2, 0, 3).double().cpu() for i in range(3))
    # generalized_kernel folds dim_head^-1/4 into the data; the kernel takes a projection matrix that carries it already
    phi_q, phi_k = (generalized_kernel(t, P_.double().cpu() * 64 ** 0.25) for t in (q, k))
    ref = P.causal_linear_attention(phi_q, phi_k, v)                      # [B, G, N, 64]
    got = out[:, :, :G * 64].reshape(N, B, G, 64).permute(1, 2, 0, 3)
    worst = max(_rel(got[:, :, t], ref[:, :, t]) for t in range(N))
    print(f"  worst position: max relative error {worst:.3g}")
    assert worst < REL
    assert bool(torch.isnan(out[:, :, G * 64:]).all())
    assert _rel(Ez[:, :m], phi_k.sum(2).reshape(B * G, m)) < 1e-5 and (LDF == m or float(Ez[:, m:].abs().max()) == 0.0)
    assert LDF == m or float(E.view(B * G, LDF, 64)[:, m:].abs().max()) == 0.0
    out2, E2, Ez2 = run()                                                 # a second run from fresh state: bitwise
    assert torch.equal(out2[:, :, :G * 64], out[:, :, :G * 64]) and torch.equal(E2, E) and torch.equal(Ez2, Ez)


def test_step_kernel_argument_errors():
    F, lib, st = _ffi()
    t = torch.zeros(4096, device="cuda")
    pos = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(q=t, B=1, G=1, dh=64, m=16, LDF=16, pos_=pos):
        return lib.sa_favor_generalized_step(F.ptr(q), 192, 0, F.ptr(t), 192, 64, F.ptr(t), 192, 128, F.ptr(t), B, G, dh, m, LDF, F.ptr(t), F.ptr(t), F.ptr(t),
                                             F.ptr(pos_), F.ptr(t), 64, 0, st)

    assert call() == 0
    assert call(q=None) == F.SA_EINVAL and call(pos_=None) == F.SA_EINVAL and call(B=0) == F.SA_EINVAL and call(G=-1) == F.SA_EINVAL and call(m=0) == F.SA_EINVAL
    assert call(dh=32) == F.SA_EUNSUPPORTED and call(m=273, LDF=288) == F.SA_EUNSUPPORTED
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ networks
def _build(cfg, st, dtype=torch.float32, rezero=True, generalized=True):
    from synthanatomy_amd.networks.transformers.img2seq_ordering import Ordering
    from synthanatomy_amd.networks.transformers.performer import Performer
    o = Ordering("raster_scan", 3, (1,) + tuple(cfg.spatial_shape), (False,) * 3, (), ())
    net = Performer(num_tokens=cfg.num_tokens, max_seq_len=cfg.max_seq_len, dim=cfg.dim, depth=cfg.depth, heads=cfg.heads, ordering=o,
                    dim_head=cfg.dim_head, local_attn_heads=cfg.local_attn_heads, local_window_size=cfg.local_window_size, use_rezero=rezero,
                    spatial_position_emb="absolute", spatial_shape=cfg.spatial_shape, feature_redraw_interval=None, compute_dtype=dtype,
                    generalized_attention=generalized)
    missing, unexpected = net.load_state_dict({k: v.clone() for k, v in st.items()}, strict=False)
    assert not unexpected, unexpected
    assert all(("spatial_indices_sequence" in k or "inv_freq" in k or "calls_since" in k) for k in missing), missing
    return net.cuda(), o


def _gates(st, value):
    for k in st:
        if k.endswith(".g"):
            st[k] = torch.tensor(value)  # the 1e-3 init would hide errors behind the residual path
    return st


def _step(net, tok, tgt):
    """one training forward + backward: (logits, loss, gradients by name)"""
    from synthanatomy_amd.losses.transformer import CELoss
    net.zero_grad(set_to_none=True)
    out = net(tok.cuda())
    loss = CELoss()(out.transpose(1, 2), tgt.cuda())
    loss.backward()
    torch.cuda.synchronize()
    return out.detach(), loss.detach(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("rezero,B,shape,window,local", [(True, 2, (2, 3, 4), 6, 2), (False, 1, (3, 3, 5), 64, 1), (True, 3, (2, 2, 5), 7, 4), (True, 2, (2, 3, 3), 5, 0)])
def test_fp32_network_matches_the_restated_oracle(monkeypatch, rezero, B, shape, window, local):
    """the four configurations and bounds of test_forward_and_gradients_match_oracle with generalized_attention=True; the oracle runs the restated map"""
    from synthanatomy_amd import debug
    monkeypatch.setattr(P, "softmax_kernel", as_softmax_kernel)
    n = int(np.prod(shape))
    cfg = P.PerformerConfig(num_tokens=33, max_seq_len=n, dim=32, depth=2, heads=4, dim_head=64, local_attn_heads=local, local_window_size=window,
                            spatial_shape=shape, use_rezero=rezero)
    st = P.init_state(cfg, seed=n)
    if rezero:
        _gates(st, 0.4)
    net, o = _build(cfg, st, rezero=rezero)
    net.train()
    seqs = P.spatial_index_sequences(shape, o.get_sequence_ordering())
    torch.manual_seed(0)
    tok = torch.randint(0, 33, (B, n))
    tgt = torch.randint(0, 32, (B, n))
    leaf = {k: v.clone().requires_grad_(True) for k, v in st.items() if "projection_matrix" not in k}
    stt = dict(st)
    stt.update(leaf)
    ref = P.forward(stt, cfg, tok, seqs)
    ref_loss = P.ce_loss(ref, tgt)
    ref_loss.backward()
    out, loss, grads = _step(net, tok, tgt)
    assert out.shape == (B, n, 33)
    print(f"  logits: max relative error {_rel(out, ref):.3g}")
    assert _rel(out, ref) < REL
    assert abs(loss.item() - ref_loss.item()) < 1e-4 * abs(ref_loss.item()) + 1e-6
    worst = ("", 0.0)
    for k, p in leaf.items():
        if p.grad is None:
            continue
        assert k in grads, k
        e = _rel(grads[k], p.grad)
        if e > worst[1]:
            worst = (k, e)
    print(f"  worst gradient: {worst}")
    assert worst[1] < 3e-3, worst
    if local == 4:
        # no global heads: nothing generalized runs, the network IS the softmax network (fixed-order reductions, so that a step is repeatable at all)
        soft, _ = _build(cfg, st, rezero=rezero, generalized=False)
        soft.train()
        with debug.override(deterministic=True):
            a, b = _step(net, tok, tgt), _step(soft, tok, tgt)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2].keys() == b[2].keys() and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    else:
        monkeypatch.undo()
        with torch.no_grad():
            soft_ref = P.forward(st, cfg, tok, seqs)
        assert _rel(out, soft_ref) > 5 * REL           # the generalized map is not the softmax map in disguise (the two oracles differ by about 2e-2 here)


def _aggregate(got, ref):
    num = sum(float((got[k].double() - ref[k].double()).pow(2).sum()) for k in ref)
    den = sum(float(ref[k].double().pow(2).sum()) for k in ref)
    return (num / den) ** 0.5


def test_throughput_network_follows_the_restatement_and_the_fp32_mode(monkeypatch):
    """The shape, state and bound (3e-2) of test_bf16_projections_close_to_fp32_oracle for the eval logits.  Gradients (ReZero gates at 0.4, so that the
    attention matters): the aggregate relative error over all parameters against the fp32-mode gradients of the same network is held to 5e-2, the bound bf16
    gradients are given per parameter; bf16 rounding of q / k flips ReLU masks near zero, which the softmax map has no counterpart for, so the softmax
    network's figure at the same shape and seed is printed next to it."""
    shape = (2, 3, 4)
    cfg = P.PerformerConfig(num_tokens=33, max_seq_len=24, dim=64, depth=2, heads=4, dim_head=64, local_attn_heads=2, local_window_size=8, spatial_shape=shape)
    st = P.init_state(cfg, seed=5)
    net, o = _build(cfg, st, dtype=torch.bfloat16)
    seqs = P.spatial_index_sequences(shape, o.get_sequence_ordering())
    torch.manual_seed(1)
    tok = torch.randint(0, 33, (2, 24))
    tgt = torch.randint(0, 32, (2, 24))
    with torch.no_grad():
        out = net.eval()(tok.cuda())
    monkeypatch.setattr(P, "softmax_kernel", as_softmax_kernel)
    err = _rel(out, P.forward(st, cfg, tok, seqs))
    monkeypatch.undo()
    print(f"  eval logits: max relative error {err:.3g}")
    assert err < 3e-2
    figures = {}
    for generalized in (True, False):
        stg = _gates(dict(st), 0.4)
        grads = [_step(_build(cfg, stg, dtype=dt, generalized=generalized)[0].train(), tok, tgt)[2] for dt in (torch.bfloat16, torch.float32)]
        figures[generalized] = _aggregate(grads[0], grads[1])
    print(f"  aggregate gradient error, throughput against fp32 mode: generalized {figures[True]:.4g}, softmax {figures[False]:.4g}")
    assert figures[True] < 5e-2, figures


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_training_step_is_bitwise_repeatable(dtype):
    """two training steps from the same state: bitwise equal loss and gradients in both modes (the generalized kernels use no atomics; the rest of the
    network takes its fixed-order reductions).  N = 125: two 64-position chunks per scan, four blocks of 128 rows per projection launch."""
    from synthanatomy_amd import debug
    shape, n = (5, 5, 5), 125
    cfg = P.PerformerConfig(num_tokens=33, max_seq_len=n, dim=64, depth=2, heads=4, dim_head=64, local_attn_heads=2, local_window_size=16, spatial_shape=shape)
    st = _gates(P.init_state(cfg, seed=2), 0.4)
    torch.manual_seed(4)
    tok = torch.randint(0, 33, (2, n))
    tgt = torch.randint(0, 32, (2, n))
    net, _ = _build(cfg, st, dtype=dtype)
    net.train()
    with debug.override(deterministic=True):
        a, b = _step(net, tok, tgt), _step(net, tok, tgt)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    assert len(a[2]) >= 20 and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    assert all(bool(torch.isfinite(g).all()) for g in a[2].values()) and float(a[2]["performer.net.layers.0.0.fn.to_q.weight"].abs().max()) > 0


def _decided_state(cfg, shape, o):
    """the first state seed, from 7 on, at which every arg-max of the oracle's greedy chain clears its runner-up by 2 * REL * max |logit| -- in the ORACLE's
    numbers alone (chosen on the CPU, as tests/test_healing_gpu.py chooses its planted cases): only then is equality of the chains a fair demand"""
    seqs = P.spatial_index_sequences(shape, o.get_sequence_ordering())
    n = int(np.prod(shape))
    for seed in range(7, 27):
        st = _gates(P.init_state(cfg, seed=seed), 0.7)      # ReZero gates start at 1e-3: make the attention matter
        x = torch.full((3, 1), 18, dtype=torch.long)
        rows = []
        for _ in range(n):
            rows.append(P.forward(st, cfg, x, seqs)[:, -1])
            x = torch.cat((x, rows[-1].argmax(-1, keepdim=True)), 1)
        rows = torch.stack(rows, 1).double()
        top2 = rows.topk(2, dim=-1).values
        if float((top2[..., 0] - top2[..., 1]).min()) > 2 * REL * float(rows.abs().max()):
            return st, seqs, x[:, 1:]
    raise AssertionError("no state seed in 7..26 decides every step of the greedy chain by the bound")


@pytest.mark.parametrize("rezero,shape,window,local,use_graph", [(True, (2, 3, 4), 5, 1, True), (False, (3, 2, 5), 7, 2, False), (True, (2, 2, 6), 64, 0, True),
                                                                 (True, (2, 3, 5), 4, 3, False)])
def test_stateful_decoding_equals_the_quadratic_loop(monkeypatch, rezero, shape, window, local, use_graph):
    """the parametrisation and demands of test_stateful_sampler_equals_the_quadratic_loop with generalized_attention=True (greedy chains of the O(N) decoder,
    the reference loop and the oracle are EQUAL), and heal(threshold=None): its likelihood map against the cross-entropy of the training forward"""
    from synthanatomy_amd.networks.transformers.img2seq_ordering import Ordering
    monkeypatch.setattr(P, "softmax_kernel", as_softmax_kernel)
    n = int(np.prod(shape))
    cfg = P.PerformerConfig(num_tokens=19, max_seq_len=n, dim=32, depth=2, heads=4, dim_head=64, local_attn_heads=local, local_window_size=window,
                            spatial_shape=shape, use_rezero=rezero)
    o = Ordering("raster_scan", 3, (1,) + shape, (False,) * 3, (), ())
    st, seqs, chain = _decided_state(cfg, shape, o)
    net, _ = _build(cfg, st, rezero=rezero)
    assert all("smax" not in s and "V1" not in s and set(s) == {"dd", "E", "Ez", "kc", "vc"} for s in (l.new_state(3, n, "cuda") for l in net._chain.layers))
    prefix = torch.full((3, 1), 18, dtype=torch.long, device="cuda")
    quad = net.sample(prefix, sample=False, stateful=False)
    fast = net.sample(prefix, sample=False, stateful=True, use_graph=use_graph)
    assert fast.shape == (3, *shape)
    assert torch.equal(fast, quad)
    again = net.sample(prefix, sample=False)          # default = stateful; a second run must not see the first one's state
    assert torch.equal(again, quad)
    assert torch.equal(fast.cpu(), chain[:, o.get_revert_sequence_ordering()].reshape(3, *shape))
    smp = net.sample(prefix, sample=True, top_k=5, temperature=0.9)
    assert int(smp.min()) >= 0 and int(smp.max()) <= 18
    # score only: the codes come back and the likelihood map is the cross-entropy of the parallel (training) forward on the same codes
    codes = torch.randint(0, 18, (3, *shape), generator=torch.Generator().manual_seed(11))
    body = codes.reshape(3, -1)[:, o.get_sequence_ordering()]
    x_in = torch.cat((torch.full((3, 1), 18, dtype=torch.long), body[:, :-1]), 1).cuda()
    with torch.no_grad():
        logits = net.eval()(x_in).float().contiguous()
    want = torch.nn.functional.cross_entropy(logits.double().transpose(1, 2), body.cuda(), reduction="none")
    bound = 2 * REL * float(logits.abs().max())
    for how in (dict(use_graph=use_graph), dict(stateful=False)):
        healed, nll, replaced = net.heal(codes.cuda(), **how)
        assert torch.equal(healed.cpu(), codes) and not bool(replaced.any())
        err = float((nll.reshape(3, -1)[:, o.get_sequence_ordering()].double() - want).abs().max())
        print(f"  {how}: max |nll - cross-entropy| = {err:.3g}, bound {bound:.3g}")
        assert err <= bound, (how, err, bound)


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_chain_trains_resumes_samples_and_heals(tmp_path, capsys):
    """run_transformer.py with --generalized_attention=True: two epochs, one more from the checkpoint, inference, healing; the files have the shapes and dtypes
    the softmax run writes, and the checkpoint loads into a fresh generalized network"""
    import run_transformer as RT
    from synthanatomy_amd.utils.general import check_for_checkpoints, create_folder_structure, load_network_state
    proj = str(tmp_path) + "/"
    shape = (2, 3, 4)
    flags = dict(project_directory=proj, vocab_size=16, n_embd=64, n_layers=2, n_head=4, local_attn_heads=2, local_window_size=8, use_rezero=True,
                 spatial_position_emb="absolute", feature_redraw_interval=None, batch_size=2, eval_batch_size=2, log_every=1, learning_rate=1e-3,
                 spatial_shape=shape, checkpoint_every=1)
    syn = ["--training_subjects=synthetic:4", "--validation_subjects=synthetic:4"]
    written = {}
    for exp, generalized in (("gen", True), ("soft", False)):
        fl = dict(flags, experiment_name=exp, generalized_attention=generalized)
        tr = [f"--{k}={str(v).replace(' ', '')}" for k, v in fl.items()] + syn
        ck = proj + exp + "/performer/checkpoints/checkpoint_epoch={}.pt"
        RT.run(tr + ["--mode=training", "--epochs=2"])
        assert glob.glob(ck.format(2)) and not glob.glob(ck.format(3))
        capsys.readouterr()
        RT.run(tr + ["--mode=training", "--epochs=3"])
        assert glob.glob(ck.format(3)) and "resumed from" in capsys.readouterr().out
        RT.run(tr + ["--mode=inference"])
        RT.run(tr + ["--mode=healing", "--resample_threshold=0.5"])
        out = proj + exp + "/performer/outputs/"
        written[exp] = {f[len(out):]: np.load(f) for f in sorted(glob.glob(out + "*/*.npy"))}
        if generalized:
            cfg = create_folder_structure(dict(RT.DEFAULTS, **fl, mode="inference", network="performer", conditionings=None))
            net, _ = RT.build(cfg, shape, torch.device("cuda", 0))
            assert all(l.generalized for l in net._chain.layers)
            res, _ = load_network_state(net, check_for_checkpoints(cfg))
            assert not res.unexpected_keys and not res.missing_keys
    assert len(written["gen"]) == 4 * 4 and written["gen"].keys() == written["soft"].keys()
    for name, a in written["gen"].items():
        b = written["soft"][name]
        assert a.shape == b.shape == shape and a.dtype == b.dtype, name
        if name.endswith("_nll.npy"):
            assert np.isfinite(a).all() and (a >= 0).all()
        elif name.endswith("_resampled.npy"):
            assert set(np.unique(a)) <= {0, 1}
        else:
            assert a.max() <= 16
