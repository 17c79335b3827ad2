"""GPU: Performer.heal -- likelihood maps and token healing on the O(N) decoder -- on the tiny networks of test_stateful_sampler_equals_the_quadratic_loop,
against the CPU oracle (oracle/performer_ref.py) over the growing prefix, against sample() in the always-replace limit, and between the two paths.

Bound of a score: BOUND = 2 * REL * max |oracle logit| with REL = 1e-3 of tests/test_performer_gpu.py: a logit error of REL * max moves the log-sum-exp
and the gathered logit by at most that much each.  Every decision the tests rely on (a score against log tau, a replaced position's arg-max against the
runner-up) clears that bound in the ORACLE's numbers, which the tests assert before they look at the device."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import performer_ref as P  # noqa: E402

REL = 1e-3
V, BOS, B = 19, 18, 3
# (rezero, shape, window, local heads, use_graph)
NETS = [(True, (2, 3, 4), 5, 1, True), (False, (3, 2, 5), 7, 2, False), (True, (3, 2, 5), 5, 0, True), (True, (2, 3, 4), 7, 2, False)]
IDS = [f"{'rezero' if r else 'prenorm'}-{'x'.join(map(str, s))}-w{w}-l{l}-{'graph' if g else 'eager'}" for (r, s, w, l, g) in NETS]


def _ordering(shape):
    from synthanatomy_amd.networks.transformers.img2seq_ordering import Ordering
    return Ordering("raster_scan", 3, (1,) + tuple(shape), (False,) * 3, (), ())


@functools.lru_cache(maxsize=None)
def _state(rezero, shape, window, local, seed):
    n = int(np.prod(shape))
    cfg = P.PerformerConfig(num_tokens=V, max_seq_len=n, dim=32, depth=2, heads=4, dim_head=64, local_attn_heads=local, local_window_size=window,
                            spatial_shape=shape, use_rezero=rezero)
    st = P.init_state(cfg, seed=seed)
    for k in st:   # ReZero gates start at 1e-3: make the attention matter
        if k.endswith(".g"):
            st[k] = torch.full_like(st[k], 0.7)
    o = _ordering(shape)
    return cfg, st, o, P.spatial_index_sequences(shape, o.get_sequence_ordering())


def _net(rezero, shape, window, local, seed):
    from synthanatomy_amd.networks.transformers.performer import Performer
    cfg, st, o, _ = _state(rezero, shape, window, local, seed)
    net = Performer(num_tokens=V, max_seq_len=cfg.max_seq_len, dim=32, depth=2, heads=4, ordering=o, dim_head=64, local_attn_heads=local,
                    local_window_size=window, use_rezero=rezero, spatial_position_emb="absolute", spatial_shape=shape, feature_redraw_interval=None)
    net.load_state_dict({k: v.clone() for k, v in st.items()}, strict=False)
    return net.cuda()


def _to_seq(grid, o):
    return grid.reshape(grid.shape[0], -1)[:, o.get_sequence_ordering()]


def _to_grid(seq, o, shape):
    return seq[:, o.get_revert_sequence_ordering()].reshape(seq.shape[0], *shape)


def _oracle_rows(st, cfg, seqs, body, conds=None, ctype="none"):
    """last-row logits of the oracle over the growing prefix [BOS, body[:, :t]], t = 0 .. n-1: [B, n, V] -- the quadratic loop's statement"""
    bos = torch.full((body.shape[0], 1), BOS, dtype=torch.long)
    return torch.stack([P.forward(st, cfg, torch.cat((bos, body[:, :t]), 1), seqs, conds, ctype)[:, -1] for t in range(body.shape[1])], 1)


def _oracle_greedy(st, cfg, seqs, n, conds=None, ctype="none"):
    """(greedy chain [B, n], its last-row logits [B, n, V])"""
    x = torch.full((B, 1), BOS, dtype=torch.long)
    rows = []
    for _ in range(n):
        rows.append(P.forward(st, cfg, x, seqs, conds, ctype)[:, -1])
        x = torch.cat((x, rows[-1].argmax(-1, keepdim=True)), 1)
    return x[:, 1:], torch.stack(rows, 1)


def _plant(st, cfg, seqs, n, conds=None, ctype="none"):
    """The greedy chain g with the first, the middle and the last position of every row overwritten by the least probable code there, and a threshold
    between the planted tokens' probabilities and the chain's.  Returns None unless -- in the oracle's numbers alone -- every decision (planted: below
    log tau; the chain's tokens: above) and every planted position's arg-max over its runner-up clears BOUND."""
    g, rows = _oracle_greedy(st, cfg, seqs, n, conds, ctype)
    bound = 2 * REL * float(rows.abs().max())
    lp = torch.log_softmax(rows.double(), -1)
    where = torch.zeros(B, n, dtype=torch.bool)
    where[:, [0, n // 2, n - 1]] = True
    low = lp[..., :BOS].argmin(-1)                                  # a code, not the BOS id
    corrupted = torch.where(where, low, g)
    lp_g = lp.gather(2, g[..., None]).squeeze(-1)
    lp_low = lp.gather(2, low[..., None]).squeeze(-1)[where]
    log_tau = 0.5 * (float(lp_g.min()) + float(lp_low.max()))
    top2 = rows.double().topk(2, dim=-1).values
    gap = (top2[..., 0] - top2[..., 1])[where]
    ok = float(lp_g.min()) - log_tau > bound and log_tau - float(lp_low.max()) > bound and float(gap.min()) > bound
    return dict(g=g, corrupted=corrupted, where=where, tau=float(np.exp(log_tau)), log_tau=log_tau, bound=bound, lp_g=lp_g, lp_low=lp_low, gap=gap) if ok else None


@functools.lru_cache(maxsize=None)
def _planted_case(rezero, shape, window, local):
    """the first seed of the network's state, from 7 on, at which the plant-and-heal case clears its bounds in the oracle: chosen on the CPU"""
    n = int(np.prod(shape))
    for seed in range(7, 27):
        cfg, st, o, seqs = _state(rezero, shape, window, local, seed)
        case = _plant(st, cfg, seqs, n)
        if case is not None:
            return seed, case
    raise AssertionError("no state seed in 7..26 separates the planted tokens from the greedy chain by the bound")


def _assert_clears(case):
    assert float(case["lp_g"].min()) - case["log_tau"] > case["bound"] and case["log_tau"] - float(case["lp_low"].max()) > case["bound"]
    assert float(case["gap"].min()) > case["bound"]


@pytest.mark.parametrize("rezero,shape,window,local,use_graph", NETS, ids=IDS)
def test_score_only_equals_the_oracle_over_the_growing_prefix(rezero, shape, window, local, use_graph):
    cfg, st, o, seqs = _state(rezero, shape, window, local, 7)
    net = _net(rezero, shape, window, local, 7)
    codes = torch.randint(0, BOS, (B, *shape), generator=torch.Generator().manual_seed(11))
    rows = _oracle_rows(st, cfg, seqs, _to_seq(codes, o))
    want = -torch.log_softmax(rows.double(), -1).gather(2, _to_seq(codes, o)[..., None]).squeeze(-1)
    bound = 2 * REL * float(rows.abs().max())
    for how in (dict(stateful=True, use_graph=use_graph), dict(), dict(stateful=False)):
        healed, nll, replaced = net.heal(codes.cuda(), **how)
        assert healed.dtype == torch.int64 and nll.dtype == torch.float32 and replaced.dtype == torch.bool
        assert healed.shape == nll.shape == replaced.shape == (B, *shape)
        assert torch.equal(healed.cpu(), codes) and not bool(replaced.any())
        err = float((_to_seq(nll.cpu().double(), o) - want).abs().max())
        print(f"  {how}: max |nll - oracle| = {err:.3g}, bound {bound:.3g}")
        assert err <= bound, (how, err, bound)


@pytest.mark.parametrize("rezero,shape,window,local,use_graph", NETS, ids=IDS)
def test_always_replacing_is_sampling(rezero, shape, window, local, use_graph):
    net = _net(rezero, shape, window, local, 7)
    codes = torch.randint(0, BOS, (B, *shape), generator=torch.Generator().manual_seed(12)).cuda()
    prefix = torch.full((B, 1), BOS, dtype=torch.long, device="cuda")
    healed, nll, replaced = net.heal(codes, threshold=2.0, sample=False, use_graph=use_graph)
    assert torch.equal(healed, net.sample(prefix, sample=False, use_graph=use_graph)) and bool(replaced.all()) and bool(torch.isfinite(nll).all())
    for s in (0, 1):
        torch.manual_seed(s)
        healed, _, replaced = net.heal(codes, threshold=2.0, sample=True, top_k=5, temperature=0.9, use_graph=use_graph)
        torch.manual_seed(s)
        assert torch.equal(healed, net.sample(prefix, sample=True, top_k=5, temperature=0.9, use_graph=use_graph)) and bool(replaced.all())


@pytest.mark.parametrize("rezero,shape,window,local,use_graph", NETS, ids=IDS)
def test_planted_tokens_are_healed_and_nothing_else(rezero, shape, window, local, use_graph):
    """also the two paths against each other under greedy draws, and a second call that must not see the first one's state"""
    seed, case = _planted_case(rezero, shape, window, local)
    _assert_clears(case)
    cfg, st, o, seqs = _state(rezero, shape, window, local, seed)
    net = _net(rezero, shape, window, local, seed)
    corrupted = _to_grid(case["corrupted"], o, shape).cuda()
    want, where = _to_grid(case["g"], o, shape), _to_grid(case["where"], o, shape)
    assert int(where.sum()) >= 2 * B and not torch.equal(corrupted.cpu(), want)
    fast = net.heal(corrupted, threshold=case["tau"], sample=False, stateful=True, use_graph=use_graph)
    assert torch.equal(fast[0].cpu(), want) and torch.equal(fast[2].cpu(), where)
    quad = net.heal(corrupted, threshold=case["tau"], sample=False, stateful=False)
    again = net.heal(corrupted, threshold=case["tau"], sample=False)
    for other in (quad, again):
        assert torch.equal(other[0], fast[0]) and torch.equal(other[2], fast[2])
        assert float((other[1] - fast[1]).abs().max()) <= case["bound"]
    clean = net.heal(want.cuda(), threshold=case["tau"], sample=False, use_graph=use_graph)      # the chain itself: nothing to heal
    assert torch.equal(clean[0].cpu(), want) and not bool(clean[2].any())


@pytest.mark.parametrize("ctype", ["bos_replacement", "prepending"])
def test_conditioned_healing_on_both_paths(ctype):
    import test_conditioning_gpu as C
    g = torch.Generator().manual_seed(5)
    case = None
    for seed in range(13, 33):
        net, st, cfg, o, seqs = C._net_and_state(ctype, C.NCOND, V, seed, 0.7, cond_scale=4.0 if ctype == "prepending" else 1.0)
        conds = [torch.randint(0, k, (B, 1), generator=g) for k in C.NCOND]
        case = _plant(st, cfg, seqs, C.N, conds, ctype)
        if case is not None:
            break
    assert case is not None, "no state seed in 13..32 separates the planted tokens from the greedy chain by the bound"
    _assert_clears(case)
    cd = [c.cuda() for c in conds]
    corrupted = _to_grid(case["corrupted"], o, C.SHAPE).cuda()
    want, where = _to_grid(case["g"], o, C.SHAPE), _to_grid(case["where"], o, C.SHAPE)
    fast = net.heal(corrupted, conditioning=cd, threshold=case["tau"], sample=False, stateful=True)
    eager = net.heal(corrupted, conditioning=cd, threshold=case["tau"], sample=False, stateful=True, use_graph=False)
    quad = net.heal(corrupted, conditioning=cd, threshold=case["tau"], sample=False, stateful=False)
    for out in (fast, eager, quad):
        assert torch.equal(out[0].cpu(), want) and torch.equal(out[2].cpu(), where)
    prefix = torch.full((B, 1), BOS, dtype=torch.long, device="cuda")
    assert torch.equal(net.heal(corrupted, conditioning=cd, threshold=2.0, sample=False, stateful=True)[0],
                       net.sample(prefix, conditioning=cd, sample=False, stateful=True))


def test_rotary_heals_on_the_reference_loop_only():
    from synthanatomy_amd.networks.transformers.performer import Performer
    shape = (2, 2, 3)
    torch.manual_seed(0)
    net = Performer(num_tokens=V, max_seq_len=12, dim=32, depth=1, heads=2, ordering=_ordering(shape), dim_head=64, local_attn_heads=1, local_window_size=4,
                    use_rezero=True, spatial_position_emb="absolute", spatial_shape=shape, feature_redraw_interval=None, rotary_position_emb=True).cuda()
    codes = torch.randint(0, BOS, (2, *shape), generator=torch.Generator().manual_seed(1)).cuda()
    with pytest.raises(NotImplementedError):
        net.heal(codes, stateful=True)
    for how in (dict(stateful=False), dict()):
        healed, nll, replaced = net.heal(codes, **how)
        assert torch.equal(healed, codes) and not bool(replaced.any()) and bool(torch.isfinite(nll).all()) and bool((nll > 0).all())
