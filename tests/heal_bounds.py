"""Element-wise fp64 error bound of the score sa_heal_step writes (csrc/performer.hip: heal_step_kernel), its planted-defect witnesses and an fp32 model
of the kernel's arithmetic.  The rule is head_bounds' cross-entropy rule (head_bounds.ce_ref is the fp64 reference) with the addition chain of THIS
kernel, which is not a wave's: one block of 1 024 threads owns a row, thread t adds its ept = ceil(V / 1024) contiguous logits' exponentials in order,
wave_sum's six butterfly levels follow, and every thread adds the 16 wave totals in order:

    L = ceil(V / 1024) + 6 + 15                                      (head_bounds.wave_chain is ceil(V / 64) + 6: smaller at V = 19, larger at 16 384)

With U = 2^-24, G = L U, E = 2 (expf, logf), m the row maximum, s = sum exp(l - m), p the softmax, x the token scored:

    ds / s = G + E U + U sum_c p_c |l_c - m| + V TINY + 4 U^2 |m|
    dlse   = ds / s + E U |log s| + U |lse|
    dnll   = dlse + U |lse - l_x|

4 U^2 |m|: the kernel shifts by the raw logit at the arg-max of the SCALED row.  Scaling by 1 / T rounds, so two raw logits within 2 U |m| of each
other can tie after it and the lowest index wins: the shift m' is then below m by at most 2 U |m|, which moves every |l_c - m| by that much, i.e. the
sum of exponentials' relative error by at most U * 2 U |m| (doubled for the rounding of m' - m itself).  lse = m' + log sum exp(l - m') is exact in m'.

A token outside [0, V) scores +inf exactly.  Measured on the MI355X over every case of tests/test_heal_step_gpu.py: MEASURED below.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import head_bounds as hb

U, E, TINY = hb.U, hb.E, hb.TINY

MEASURED = dict(nll=0.396)     # worst max |err| / bound on the MI355X over every case of tests/test_heal_step_gpu.py (the fp32 model on the CPU: the same cases)


def heal_chain(V: int) -> int:
    """longest addition chain of heal_step_kernel's sum over a row of V logits"""
    return -(-V // 1024) + 6 + 15


def last_pass(V: int):
    """mask [V] of the columns a sum without its last pass misses: the last element of every thread's run (ept > 1), or the last wave's columns"""
    ept = -(-V // 1024)
    v = torch.arange(V)
    return (v % ept == ept - 1) if ept > 1 else (v >= hb.last_stride(V))


def nll_ref(l, x, drop_last_pass: bool = False):
    """fp64 score of tokens x [R] under logits l [R, V] (fp64): dict as head_bounds.ce_ref, `term` = nll with +inf where x lies outside [0, V)"""
    R, V = l.shape
    ref = hb.ce_ref(l, x, 1.0)
    if drop_last_pass:
        e = torch.exp(l - ref["m"])
        e[:, last_pass(V)] = 0.0
        ref["s"] = e.sum(1, keepdim=True)
        ref["lse"] = ref["m"] + torch.log(ref["s"])
        ref["term"] = (ref["lse"] - ref["lt"]).view(R)
    ref["term"] = torch.where(ref["valid"], ref["term"], torch.full((R,), float("inf"), dtype=l.dtype))
    return ref


def nll_bound(l, ref):
    """dnll [R] of nll_ref's truth (1e-300 where the score is +inf: exact)"""
    R, V = l.shape
    m, s, lse, p, lt, valid = ref["m"], ref["s"], ref["lse"], ref["p"], ref["lt"], ref["valid"]
    zero = torch.zeros_like(l)
    ds = heal_chain(V) * U + E * U + U * torch.where(p > 0, p * (l - m).abs(), zero).sum(1, keepdim=True) + V * TINY + 4 * U * U * m.abs()
    dlse = ds + E * U * torch.log(s).abs() + U * lse.abs()
    return torch.where(valid, (dlse + U * (lse - lt).abs()).view(R), torch.zeros(R, dtype=l.dtype)) + 1e-300


def model_nll(l, x, temperature: float = 1.0):
    """heal_step_kernel's score in fp32 torch arithmetic, operation by operation (l fp32 [R, V]; the shift is the raw logit at the scaled arg-max)"""
    R, V = l.shape
    ept = -(-V // 1024)
    scaled = l * torch.tensor(1.0 / temperature, dtype=torch.float32)
    m = l.gather(1, scaled.argmax(1, keepdim=True))
    pad = torch.zeros(R, 1024 * ept, dtype=torch.float32)
    pad[:, :V] = torch.exp(l - m)
    pad = pad.view(R, 1024, ept)
    acc = torch.zeros(R, 1024, dtype=torch.float32)
    for e in range(ept):
        acc = acc + pad[:, :, e]
    acc = acc.view(R, 16, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, lane ^ o]
    s = acc[:, 0, 0]
    for w in range(1, 16):
        s = s + acc[:, w, 0]
    valid = (x >= 0) & (x < V)
    score = (m.view(R) + torch.log(s)) - l.gather(1, x.clamp(0, V - 1).view(R, 1)).view(R)
    return torch.where(valid, score, torch.full((R,), float("inf"), dtype=torch.float32))


def verify_nll(tag: str, l32, x, temperature: float, got, ratios=None, asserted=None):
    """got [R] (scores of tokens x under the fp32 logits l32) inside the bound of the fp64 truth; the witnesses -- the SCALED logits scored, the sum
    without its last pass -- outside wherever their defect leaves it; +inf exactly where x lies outside [0, V)"""
    l = l32.double().cpu()
    x = x.cpu()
    got = got.detach().cpu()
    ref = nll_ref(l, x)
    ok = ref["valid"]
    assert bool(torch.isposinf(got[~ok]).all()), f"{tag}: a token outside [0, V) must score +inf"
    wit = {"no last pass": nll_ref(l, x, drop_last_pass=True)["term"][ok]}
    if temperature != 1.0:
        wit["scaled logits scored"] = nll_ref(l / temperature, x)["term"][ok]
    hb.within(f"{tag} nll", got[ok], ref["term"][ok], nll_bound(l, ref)[ok], wit, ratios, asserted)
    return ref


# ------------------------------------------------------------------------------------------------------------------------------ cases
# the shapes of test_sample_step_kernel_matches_the_torch_decision: one element per thread, several, a ragged last thread; nine positions
TOTAL = 9
SHAPES = [(3, 19), (6, 2049), (17, 1000), (5, 16384)]
DRAWS = [(1.0, 0), (0.7, 0), (0.9, -1)]        # (temperature, top_k); -1: 5 at V = 19, else 40


def top_k_of(V, k):
    return (5 if V == 19 else 40) if k < 0 else k


@functools.lru_cache(maxsize=None)
def case(B, V, temperature, top_k, seed=0):
    """fresh logits per step (on a coarse grid with planted ties when top-k is on, as the sampler's test), the tokens already there, the uniforms, and the
    fp64 scores of those tokens with their bounds: [TOTAL - 1] lists indexed by step, which decides position step + 1.  Nothing here comes from a kernel."""
    g = torch.Generator().manual_seed(1000 * seed + B + V + top_k)
    seq0 = torch.randint(0, V, (B, TOTAL), generator=g)
    table = torch.rand(TOTAL, B, generator=g)
    logits = []
    for _ in range(TOTAL - 1):
        l = torch.randn(B, V, generator=g) * 3
        if top_k:
            l = (l * 8).round() / 8
            l[0, :3] = 0.0
            l[0, 1] = -0.0
        logits.append(l)
    refs = [nll_ref(l.double(), seq0[:, s + 1]) for s, l in enumerate(logits)]
    nll = torch.stack([r["term"] for r in refs], 1)                                    # [B, TOTAL - 1]: column s is position s + 1
    bnd = torch.stack([nll_bound(l.double(), r) for l, r in zip(logits, refs)], 1)
    return dict(seq0=seq0, table=table, logits=logits, nll=nll, bnd=bnd)


def middle_threshold(B, V, temperature, top_k, P_):
    """(case, log_threshold as the c_float the kernel gets): -log tau halfway between the two middle scores of the decided positions, with the seed chosen
    on the CPU so that NO decided row lies within 100 x its bound of it -- from the fp64 reference alone"""
    for seed in range(20):
        c = case(B, V, temperature, top_k, seed)
        nll, bnd = c["nll"][:, P_ - 1:], c["bnd"][:, P_ - 1:]
        srt = nll.flatten().sort().values
        cut = float(np.float32(-0.5 * float(srt[srt.numel() // 2 - 1] + srt[srt.numel() // 2])))      # log tau
        if bool(((nll + cut).abs() > 100 * bnd).all()):
            return c, cut
    raise AssertionError("no seed in 0..19 keeps every score 100 bounds away from the threshold")
