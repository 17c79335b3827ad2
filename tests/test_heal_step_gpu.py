"""GPU: sa_heal_step alone (csrc/performer.hip: heal_step_kernel) -- the score against the fp64 log-softmax inside the derived bound of
tests/heal_bounds.py, the three decision regimes (never, always = sa_sample_step itself, a threshold in between), the draw rule of the replaced
entries, and the edge cases.  Shapes: those of test_sample_step_kernel_matches_the_torch_decision (one element per thread, several, a ragged last
thread, both grid modes)."""
import pytest
import torch

import heal_bounds as hlb

pytestmark = pytest.mark.gpu

TOTAL, SHAPES, DRAWS = hlb.TOTAL, hlb.SHAPES, hlb.DRAWS
NLL_FILL, REP_FILL = -7.0, 170
EINVAL = -1
_top_k, _case, _middle_threshold = hlb.top_k_of, hlb.case, hlb.middle_threshold


def _torch_decisions(c, V, temperature, top_k, do_sample, us):
    """per step: (probs [B, V] after temperature and cut, the token the torch expressions of the sampler choose), on the device as the sampler's test"""
    out = []
    for s, l in enumerate(c["logits"]):
        scaled = l.cuda() / temperature
        if top_k:
            kth = torch.topk(scaled, top_k, dim=-1).values[:, -1:]
            scaled = scaled.masked_fill(scaled < kth, float("-inf"))
        probs = torch.softmax(scaled, dim=-1)
        if do_sample:
            cdf = probs.cumsum(-1)
            ix = (cdf < us[s][:, None] * cdf[:, -1:]).sum(-1).clamp(max=V - 1)
        else:
            ix = probs.argmax(-1)
        out.append((probs, ix))
    return out


def _run(c, B, V, P_, temperature, top_k, per_row, do_sample, log_threshold, sampler=False, seq0=None):
    """TOTAL - 1 launches of sa_heal_step (or sa_sample_step) from position 0; pos, ticket and tok are checked after every launch"""
    from synthanatomy_amd import _ffi
    lib = _ffi.lib()
    seq = (c["seq0"] if seq0 is None else seq0).clone().cuda()
    nll = torch.full((B, TOTAL), NLL_FILL, device="cuda")
    rep = torch.full((B, TOTAL), REP_FILL, dtype=torch.uint8, device="cuda")
    posbuf = torch.zeros(2, dtype=torch.int32, device="cuda")
    pos, ticket = posbuf[:1], posbuf[1:]
    tok = torch.zeros(B, dtype=torch.int64, device="cuda")
    table = c["table"].cuda()
    toks = []
    for step in range(TOTAL - 1):
        logits = c["logits"][step].cuda()
        u = table if per_row else table[step].contiguous()
        head = (_ffi.ptr(logits), B, V, float(temperature), _ffi.ptr(u), B if per_row else 0, do_sample, top_k)
        tail = (_ffi.ptr(pos), _ffi.ptr(ticket) if per_row else None, _ffi.ptr(tok), _ffi.stream())
        if sampler:
            _ffi.check(lib.sa_sample_step(*head, _ffi.ptr(seq), TOTAL, P_, *tail), "sa_sample_step")
        else:
            _ffi.check(lib.sa_heal_step(*head, float(log_threshold), _ffi.ptr(seq), TOTAL, P_, _ffi.ptr(nll), _ffi.ptr(rep), *tail), "sa_heal_step")
        torch.cuda.synchronize()
        assert int(pos) == step + 1 and int(ticket) == 0
        assert torch.equal(tok, seq[:, step + 1])
        toks.append(tok.clone())
    return dict(seq=seq, nll=nll, rep=rep, toks=torch.stack(toks), pos=int(pos), ticket=int(ticket), us=[table[s] for s in range(TOTAL - 1)])


def _check_scores(tag, c, temperature, P_, out, seq0=None):
    """every decided position inside its bound; positions < P (and column 0, which no step decides) keep the fill value"""
    seq0 = c["seq0"] if seq0 is None else seq0
    assert bool((out["nll"][:, :P_] == NLL_FILL).all()) and bool((out["rep"][:, :P_] == REP_FILL).all())
    for s in range(P_ - 1, TOTAL - 1):
        hlb.verify_nll(f"{tag} step {s}", c["logits"][s], seq0[:, s + 1], temperature, out["nll"][:, s + 1])


params = pytest.mark.parametrize("B,V,per_row,P_,temperature,k",
                                 [(B, V, per_row, P_, t, k) for (B, V) in SHAPES for per_row in (False, True) for P_ in (1, 2) for (t, k) in DRAWS])


@params
def test_threshold_never_scores_and_leaves_the_sequence(B, V, per_row, P_, temperature, k):
    """log_threshold = -inf: nll inside the derived bound of the fp64 log-softmax of the RAW logits (the witnesses -- scaled logits scored, the sum
    without its last pass -- outside it), seq unchanged, replaced all zero, the prefix columns untouched"""
    top_k = _top_k(V, k)
    c = _case(B, V, temperature, top_k)
    for do_sample in (0, 1):
        out = _run(c, B, V, P_, temperature, top_k, per_row, do_sample, float("-inf"))
        assert torch.equal(out["seq"].cpu(), c["seq0"])
        assert bool((out["rep"][:, P_:] == 0).all())
        _check_scores(f"{B}x{V} T{temperature} k{top_k}", c, temperature, P_, out)


@params
def test_threshold_always_is_the_sampler(B, V, per_row, P_, temperature, k):
    """log_threshold = 1: seq, tok, pos and ticket EQUAL sa_sample_step's on the same logits and uniforms, greedy and sampled; the scores are those of the
    tokens that were there"""
    top_k = _top_k(V, k)
    c = _case(B, V, temperature, top_k)
    for do_sample in (0, 1):
        out = _run(c, B, V, P_, temperature, top_k, per_row, do_sample, 1.0)
        smp = _run(c, B, V, P_, temperature, top_k, per_row, do_sample, None, sampler=True)
        assert torch.equal(out["seq"], smp["seq"]) and torch.equal(out["toks"], smp["toks"])
        assert (out["pos"], out["ticket"]) == (smp["pos"], smp["ticket"])
        assert bool((out["rep"][:, P_:] == 1).all())
        _check_scores(f"{B}x{V} T{temperature} k{top_k}", c, temperature, P_, out)


@params
def test_threshold_in_between_decides_by_the_score(B, V, per_row, P_, temperature, k):
    """replaced == (nll_ref > -log tau) on every decided position -- no row is within 100 bounds of the threshold, asserted from the fp64 reference -- and
    a replaced entry obeys the sampler's draw rule: the torch arg-max (greedy); never a token the cut removed and at most one cdf-boundary mismatch per
    case (sampled); an entry that is not replaced keeps its token"""
    top_k = _top_k(V, k)
    c, cut = _middle_threshold(B, V, temperature, top_k, P_)
    assert bool(((c["nll"][:, P_ - 1:] + cut).abs() > 100 * c["bnd"][:, P_ - 1:]).all())
    want = (c["nll"] > -cut)                       # [B, TOTAL - 1], column s = position s + 1
    assert 0 < int(want[:, P_ - 1:].sum()) < want[:, P_ - 1:].numel()
    mism = 0
    for do_sample in (0, 1):
        out = _run(c, B, V, P_, temperature, top_k, per_row, do_sample, cut)
        dec = _torch_decisions(c, V, temperature, top_k, do_sample, [u.cuda() for u in out["us"]])
        rep, seq = out["rep"].cpu(), out["seq"].cpu()
        assert torch.equal(rep[:, P_:], want[:, P_ - 1:].to(torch.uint8))
        assert torch.equal(seq[:, :P_], c["seq0"][:, :P_])
        for s in range(P_ - 1, TOTAL - 1):
            w = want[:, s]
            probs, ix = dec[s][0].cpu(), dec[s][1].cpu()
            assert torch.equal(seq[~w, s + 1], c["seq0"][~w, s + 1])
            if do_sample:
                assert bool((probs.gather(1, seq[:, s + 1:s + 2])[w] > 0).all())
                mism += int((seq[w, s + 1] != ix[w]).sum())
            else:
                assert torch.equal(seq[w, s + 1], ix[w]), s
        _check_scores(f"{B}x{V} T{temperature} k{top_k}", c, temperature, P_, out)
    assert mism <= 1, mism


@pytest.mark.parametrize("per_row", [False, True])
def test_a_token_outside_the_vocabulary_scores_inf_and_is_replaced(per_row):
    B, V, P_ = 6, 2049, 1
    c = _case(B, V, 1.0, 0)
    seq0 = c["seq0"].clone()
    seq0[1, 3], seq0[4, 5], seq0[2, 8] = V, -1, 2 ** 40
    out = _run(c, B, V, P_, 1.0, 0, per_row, 0, float("-inf"), seq0=seq0)
    assert torch.equal(out["seq"].cpu(), seq0) and bool((out["rep"][:, P_:] == 0).all())
    for (b, n) in ((1, 3), (4, 5), (2, 8)):
        assert float(out["nll"][b, n]) == float("inf")
    _check_scores("bad tokens", c, 1.0, P_, out, seq0=seq0)
    out = _run(c, B, V, P_, 1.0, 0, per_row, 0, -1e30, seq0=seq0)          # any threshold at all: only the three are below it
    rep = out["rep"][:, P_:].cpu()
    assert int(rep.sum()) == 3 and bool(rep[1, 2]) and bool(rep[4, 4]) and bool(rep[2, 7])
    dec = _torch_decisions(c, V, 1.0, 0, 0, None)
    for (b, n) in ((1, 3), (4, 5), (2, 8)):
        assert int(out["seq"][b, n]) == int(dec[n - 1][1][b])


def test_argument_errors():
    from synthanatomy_amd import _ffi
    lib = _ffi.lib()
    B, V = 2, 19
    logits = torch.zeros(B, V, device="cuda")
    u = torch.zeros(TOTAL, B, device="cuda")
    seq = torch.zeros(B, TOTAL, dtype=torch.int64, device="cuda")
    nll = torch.zeros(B, TOTAL, device="cuda")
    rep = torch.zeros(B, TOTAL, dtype=torch.uint8, device="cuda")
    posbuf = torch.zeros(2, dtype=torch.int32, device="cuda")
    tok = torch.zeros(B, dtype=torch.int64, device="cuda")

    def call(**kw):
        a = dict(logits=_ffi.ptr(logits), B=B, V=V, temperature=1.0, u=_ffi.ptr(u), u_stride=B, do_sample=1, top_k=0, log_threshold=-1.0, seq=_ffi.ptr(seq),
                 total=TOTAL, P=1, nll=_ffi.ptr(nll), replaced=_ffi.ptr(rep), pos=_ffi.ptr(posbuf[:1]), ticket=_ffi.ptr(posbuf[1:]), tok=_ffi.ptr(tok))
        a.update(kw)
        return lib.sa_heal_step(*a.values(), _ffi.stream())

    for bad in (dict(logits=None), dict(seq=None), dict(nll=None), dict(replaced=None), dict(pos=None), dict(tok=None), dict(u=None), dict(V=0), dict(B=0),
                dict(temperature=0.0), dict(temperature=-1.0), dict(P=0), dict(total=0)):
        assert call(**bad) == EINVAL, bad
    assert call() == 0 and call(u=None, do_sample=0) == 0
    torch.cuda.synchronize()
    assert int(posbuf[0]) == 2 and int(posbuf[1]) == 0
