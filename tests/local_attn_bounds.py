"""Element-wise fp64 error bounds for the causal local-window attention kernels (csrc/local_attn.hip + csrc/local_attn_split.h: forward, dq, dk / dv,
each on the exact-fp32 and on the split-bf16 path, each with and without dropout -- twelve __global__ entry points) and for the decode step
(csrc/performer.hip: local_attn_step_kernel), the planted-defect witnesses that an output must fail, and fp32 / split-bf16 models of the kernels'
arithmetic (tests/test_local_attn_bounds_cpu.py holds the models to the same bounds; tests/test_local_attn_bounds_gpu.py holds the kernels to them).
The bodies co-launched by csrc/favor_fused.hip are the same __device__ bodies (local_attn_q_split_body / local_attn_kv_split_body); they stay tied
to these launches, bit for bit, by tests/test_favor_fused_gpu.py::test_colaunched_local_heads_equal_separate_launches.

The operands are drawn in fp32 on the CPU, so the fp64 reference sees exactly the kernel's operands.  Query i sees the keys lo_i <= j <= i with
lo_i = max(0, (i // W - 1) W); the scale is 64^-1/2 = 0.125, a power of two: q * scale and the final dq * scale are exact.  Notation: s = scale q.k,
m the row maximum, P the softmax, Z the scaled keep mask of tests/dropout_ref.py (1 without dropout), nk_i = i - lo_i + 1 the keys of a query,
nq_j the queries of a key, T_i the key tiles the query's block walks (kt_lo .. kt_hi of its 64-query tile), A_ij = scale sum_d |q_id| |k_jd|.

Constants, from the code:
    U = 2^-24                one fp32 rounding.
    chain(n)                 an accumulator that n non-zero terms are added to: n U on the exact path (mfma_f32_16x16x4f32 is an fma chain; adding
                             an exact zero -- a masked probability, a row beyond N -- is exact, so only the visible keys count), 3 n U on the split
                             path (three bf16 products per term; each mfma_f32_16x16x32_bf16 is allowed one rounding per product, the worst order).
                             The 64 steps of q.k and of dP = dO.v are dense: chain(64).
    SPLIT = 3 * 2^-16 (1 + 2^-7)   per product of two split operands, re-derived from split_pair: hi = bf16(x) leaves |x - hi| <= 2^-8 |x| (8-bit
                             significand, round to nearest even: half an ulp of 2^-7), x - hi is exact in fp32, lo = bf16(x - hi) leaves
                             |r| <= 2^-16 |x|.  With a = ah + al + ra:  a b - (ah bh + ah bl + al bh) = al bl + ra b + (ah + al) rb, three terms
                             of at most 2^-16 |a| |b| (1 + 2^-8) each.  It applies to both GEMMs of every kernel: P and dS are split as well
                             (acc_to_operand).  The bf16 products themselves are exact in fp32.
    group_sum                sixteen values per lane, then two shuffles: min(18, nk) roundings; l_run * alpha + ls: two more per later tile.
    __expf(x)                the compiler's header defines it as exp2(fl(0x1.715476p+0 * x)) on V_EXP_F32: the instruction is specified to 1 ulp
                             (EXP_E = 2: a relative 2 U), the rounded product and the constant (0.22 U off log2 e) put 1.25 U |x| on the argument;
                             with the rounding of x = s - m itself: EXP_ARG = 2.25, a relative 2.25 U |x|.  A result below TINY = 2^-126 may be flushed.
    __logf(x)                the header maps it to the full-precision logf (no fast-math in the build): LOG_E = 2, as tests/head_bounds.py takes it.
    1.01                     every bound is first order; SECOND = 1.01 covers the products of two error terms (the largest, ds at the peaked split
                             cases, is 3e-3: that fraction of the first-order term).

Forward.  Every weight w_j = exp(s_j - m_t) prod alpha reaches the numerator and the denominator with the SAME relative error
    ec_ij = ds_ij + EXP_E U + EXP_ARG U (m_i - s_ij) + (T_i - 1) EXP_E U,       ds_ij = (chain(64) + SPLIT) A_ij
(the arguments of p and of the later alphas telescope to m_i - s_ij; m itself is a common factor and cancels; the first alpha is exp(-1e30 - m) = 0
and a fully masked tile's is exp(0) = 1, both exact).  A common relative error e_j moves o by sum_j P_j e_j (Z_j v_j - o), so
    do_id  = sum_j P_ij ec_ij |Z_ij v_jd - o_id| + (chain(nk_i) + (T_i - 1 + drop) U + SPLIT) sum_j P_ij Z_ij |v_jd| + |o_id| (cl_i + 2) U
    dlse_i = sum_j P_ij ec_ij + cl_i U + LOG_E U |lse_i - m_i| + U |lse_i|,      cl_i = min(18, nk_i) + 2 (T_i - 1)
(acc *= alpha: one rounding per later tile; p *= z: one; 1 / l_run and the product with it: two).  o_lp must EQUAL the kernel's own o rounded once.

Backward, from the fp32 out and lse the kernel is GIVEN (the fp64 forward rounded once), so it is bounded in isolation from the forward:
P = exp(s - lse), D = rowsum(dO out), dP = dO.v, dS = P (Z dP - D), dq = scale dS k, dk = dS^T (scale q), dv = (P Z)^T dO.
    dD_i   = 19 U sum_d |dO_id out_id|                                    (the product, sixteen per lane, two shuffles)
    eP_ij  = ds_ij + EXP_E U + EXP_ARG U |s_ij - lse_i|
    ddP_ij = (chain(64) + SPLIT) sum_d |dO_id| |v_jd|
    ddS_ij = P_ij (eP_ij |t_ij| + Z_ij ddP_ij + dD_i + drop U |Z_ij dP_ij| + 2 U |t_ij|) + TINY |t_ij|,       t = Z dP - D
    ddq_id = scale (sum_j ddS_ij |k_jd| + (chain(nk_i) + SPLIT) sum_j |dS_ij| |k_jd|)
    ddk_jd = sum_i ddS_ij scale |q_id| + (chain(nq_j) + SPLIT) sum_i |dS_ij| scale |q_id|
    ddv_jd = sum_i P_ij Z_ij eP_ij |dO_id| + (chain(nq_j) + drop U + SPLIT) sum_i P_ij Z_ij |dO_id|
dv_lp must EQUAL the kernel's own dv rounded once.

Decode step (one block per batch row and head; keys lo .. t with lo = max(0, (t // W - 1) W), nk = t - lo + 1):
    sq = (q cos + rot(q) sin) * rsqrt(64):  dsq_d = 0.125 * 2 U (|q cos| + |rot(q) sin|) + 3 U |sq_d|;   kc[t] likewise without the scale: 2 U (...)
    ds_j = 64 U sum_d |sq_d k_jd| + sum_d dsq_d |k_jd| (+ sum_d |sq_d| dkc_d for j = t);    ep_j = ds_j + EXP_E U + EXP_ARG U (m - s_j)
    dout_d = sum_j P_j ep_j |v_jd - out_d| + (ceil(nk / 16) + 16) U sum_j P_j |v_jd| + |out_d| (ceil(nk / 1024) + 6 + 16 + 1) U
vc[t] is a copy: equal.  Every other cache row stays bitwise as it was; the caches hold NaN outside [lo, t), so a read outside the window poisons out.

Terms that differ from the derivation this work started from, and why:
  * the score error enters o as ds |Z v - o|, not ds |v|: an error common to numerator and denominator cancels.  Without it the exact bound of a row
    with one key (o = v exactly) is 2 * 64 U A |v|, and the split path's 2^-16 |v| passes it: the debug switch could select nothing unnoticed.
  * chains count the VISIBLE keys / queries, not 64 per tile, for the same reason: rows with few keys are where the two paths separate.
  * split_bf16.h states the dropped terms as <= 2^-16 |a| |b|.  That is one of the three: random operands reach 1.99 * 2^-16
    (test_split_constant_holds_for_split_pair), the worst case is 3 * 2^-16.  SPLIT is the re-derived constant, not the header's.
  * __expf carries EXP_ARG U |x| on top of its ulp: the argument is multiplied by a rounded log2 e before the instruction.  At the peaked cases
    (x down to -100) a flat 2 U would be missed by the kernels and the model alike.

A witness is asserted to fail wherever its planted defect leaves the bound of the truth on at least one element; where it does not, no output
could tell the two apart: printed, not asserted (decided from the two references alone).  WITNESSES lists them; tests/test_local_attn_bounds_cpu.py
fails unless each is asserted in at least one case.

Worst max |err| / bound over every case (the acceptance threshold is the bound itself, ratio <= 1; MEASURED below):
%(table)s
The exact model reproduces the exact kernels' figures to the printed digits: the MFMA is the fma chain the model walks.  The split model sums each
MFMA's 32 products exactly and rounds once; its D takes the exact path's lane order (the split kernel adds four products per step).  kc sits at
0.876 at W = 5, t = 12 (0.65 .. 0.83 elsewhere): its bound is the three roundings of k cos + rot(k) sin themselves, nothing else.
Under the EXACT bound the split kernel's o is at 27 on (23, 5) where the exact kernel's is at 0.205: the debug switch selects another kernel.
o_lp and dv_lp equal the kernel's own o and dv rounded once on every element of every case, both paths.
"""
from __future__ import annotations

import functools

import torch

import conv_bounds as cb
import norm_bounds as nb
from dropout_ref import scaled_mask

U = cb.U32
TINY = 2.0 ** -126
EXP_E, EXP_ARG, LOG_E = 2.0, 2.25, 2.0
SPLIT = 3 * 2.0 ** -16 * (1 + 2.0 ** -7)
SECOND = 1.01
LT, DH, SCALE = 64, 64, 0.125
G, L = 1, 2                               # one FAVOR+ head in front of the two local heads: the engine's column blocks
PATHS = {"exact": dict(chain=1, prod=0.0), "split": dict(chain=3, prod=SPLIT)}
DROP = dict(p=0.3, seed=0x5EED5EED12345678, site=6)

# worst max |err| / bound per output: the models on the CPU, the kernels on the MI355X (tests/test_local_attn_bounds_gpu.py, every case)
MEASURED = dict(
    model=dict(exact=dict(o=0.371, lse=0.0737, D=0.087, dq=0.1, dk=0.152, dv=0.143),
               split=dict(o=0.214, lse=0.0617, D=0.087, dq=0.0567, dk=0.0584, dv=0.0784), step=dict(out=0.0251, kc=0.876)),
    mi355x=dict(exact=dict(o=0.371, lse=0.0737, D=0.087, dq=0.1, dk=0.152, dv=0.143),
                split=dict(o=0.214, lse=0.0624, D=0.0617, dq=0.0567, dk=0.0584, dv=0.0784), step=dict(out=0.0251, kc=0.876)),
)

# (N, W): what each reaches is in CASE_NOTES; every pair runs `flat`, REGIME_CASES also run the other regimes; DROP_CASES run dropout as well
NW = [(23, 5), (64, 96), (70, 1), (150, 70), (200, 64), (257, 32), (321, 128), (900, 420)]
CASE_NOTES = {
    (23, 5): "one tile, many windows; a wave with rows on both sides of N; two waves with no row",
    (64, 96): "W > N; exactly one full tile; the diagonal tile is never unmasked",
    (70, 1): "W = 1: keys i-1 .. i",
    (150, 70): "W no multiple of the tile; queries 140..149 have lo = 70: key tile 0 is fully masked for those lanes, visible to others of the wave",
    (200, 64): "W == LT: the wave-uniform unmasked branch for tile kt-1; the last tile has 8 rows",
    (257, 32): "W < LT: the lower bound cuts inside a key tile and kt_lo > 0; the last tile has 1 row",
    (321, 128): "W = 2 LT: three key tiles per query tile with an unmasked middle; the kv walk spans three query tiles",
    (900, 420): "the product's window; the second window boundary at 840 lies inside a tile (B = 1)",
}
REGIMES = ("flat", "peaked", "offset", "rising")
REGIME_CASES = [(150, 70), (200, 64), (257, 32)]
DROP_CASES = [(150, 70), (200, 64)]
CASES = [(N, W, "flat") for (N, W) in NW] + [(N, W, r) for (N, W) in REGIME_CASES for r in REGIMES[1:]]
IDS = [f"{N}x{W}-{r}" for (N, W, r) in CASES]
DROP_IDS = [f"{N}x{W}-p0.3" for (N, W) in DROP_CASES]

# kernel table: entry point -> path -> the launches it must dispatch (tests/test_local_attn_bounds_cpu.py: every __global__ of csrc/local_attn.hip
# and local_attn_step_kernel has a row; tests/test_local_attn_bounds_gpu.py asserts the names through _ffi.kernel_log)
KERNELS = {
    "fwd": dict(exact=["local_attn_q_kernel<0>"], split=["local_attn_q_split_kernel<0>"]),
    "bwd": dict(exact=["local_attn_kv_kernel", "local_attn_q_kernel<1>"], split=["local_attn_kv_split_kernel", "local_attn_q_split_kernel<1>"]),
    "fwd_dropout": dict(exact=["local_attn_q_drop_kernel<0>"], split=["local_attn_q_split_drop_kernel<0>"]),
    "bwd_dropout": dict(exact=["local_attn_kv_drop_kernel", "local_attn_q_drop_kernel<1>"],
                        split=["local_attn_kv_split_drop_kernel", "local_attn_q_split_drop_kernel<1>"]),
    "step": dict(exact=["local_attn_step_kernel"], split=["local_attn_step_kernel"]),
}

# decode step: (W, t, N)
STEP_CASES = [(W, t, 2 * W + 3) for W in (5, 64, 420) for t in (0, W - 1, W, 2 * W - 1, 2 * W, 2 * W + 2)] + [(513, 1025, 1026)]
STEP_IDS = [f"W{W}-t{t}-N{N}" for (W, t, N) in STEP_CASES]

WITNESSES = {
    "fwd": ("lower bound one key early", "lower bound one key late", "diagonal key dropped", "key i+1 admitted", "two windows of look-back",
            "last head dimension missing", "v of row j+1", "v of head h+1", "first key of the next batch visible", "scale omitted",
            "lse of the dropped softmax", "truncated store"),
    "bwd": ("D omitted", "dq without the final scale", "dk missing the following window", "dk/dv missing the last query tile", "Z not applied to dP",
            "mask of element e+1", "lower bound one key early", "diagonal key dropped", "truncated store"),
    "arith": ("plain-bf16 product", "split model under the exact bound"),
    "step": ("current key dropped", "lower bound one key late", "unrotated key", "scale omitted"),
}


def batch_of(N: int) -> int:
    return 1 if N >= 900 else 2


# ------------------------------------------------------------------------------------------------------------------------------ geometry
def row_geometry(N: int, W: int):
    """per query i: lo_i, nk_i, T_i (key tiles the block of its 64-query tile walks); per key j: nq_j, first query tile NOT walked by its key tile's
    block (kv kernel: qt = kt .. hi / LT)"""
    i = torch.arange(N)
    lo = (i // W - 1).clamp(min=0) * W
    q0 = (i // LT) * LT
    kt_lo = ((q0 // W - 1).clamp(min=0) * W) // LT
    kt_hi = torch.clamp(q0 + LT - 1, max=N - 1) // LT
    hi = torch.clamp((i // W + 2) * W - 1, max=N - 1)
    last_key = torch.clamp(q0 + LT - 1, max=N - 1)
    qt_hi = torch.clamp((last_key // W + 2) * W - 1, max=N - 1) // LT
    return dict(lo=lo, nk=(i - lo + 1), T=(kt_hi - kt_lo + 1), hi=hi, nq=(hi - i + 1), qt_hi=qt_hi)


def band(N: int, W: int, lo_shift: int = 0, hi_shift: int = 0, back: int = 1, drop_diag: bool = False):
    """allowed[i, j]; the keyword arguments plant one mask defect each (rows that a defect would empty keep their diagonal key)"""
    i, j = torch.arange(N)[:, None], torch.arange(N)[None, :]
    lo = (i // W - back).clamp(min=0) * W + lo_shift
    ok = (j >= torch.minimum(lo, i)) & (j <= i + hi_shift)
    if drop_diag:
        ok = ok & ((j < i) | (i == 0))
    return ok


# ------------------------------------------------------------------------------------------------------------------------------ operands
def draw(N: int, W: int, regime: str, seed: int = 0):
    """q, k, v, dout [B, L, N, 64] in fp32 on the CPU"""
    B = batch_of(N)
    gen = torch.Generator().manual_seed(seed + 131 * N + 7 * W + REGIMES.index(regime))
    q, k, v, do = (torch.randn(B, L, N, DH, generator=gen) for _ in range(4))
    if regime == "peaked":
        q = q * 8.0                                         # scores ~ N(0, 64)
    elif regime == "offset":
        q[..., 0], k[..., 0] = 40.0, 20.0                   # + 100 on every score: an unshifted exp overflows
    elif regime == "rising":
        q[..., 1] = 8.0
        k[..., 1] = torch.arange(N, dtype=torch.float32) / 16.0       # + j / 16 per key: the running maximum moves on every key tile
    return dict(q=q, k=k, v=v, do=do)


def drop_mask(B: int, N: int):
    """Z [B, L, N, N]: element index ((b L + h) N + i) N + j"""
    return torch.from_numpy(scaled_mask(DROP["seed"], DROP["site"], (B, L, N, N), DROP["p"]))


def strides(N: int):
    """the engine's layout: (stride, offset) of q, k, v, o"""
    inner = (G + L) * DH
    return dict(q=(L * DH + DH, DH), k=(L * DH, 0), v=(3 * inner, G * DH), o=(inner, G * DH))


def pack(t, stride: int, off: int, fill=float("nan"), dtype=torch.float32):
    """[B, L, N, 64] -> rows [B N, stride] with the head blocks at column `off`, `fill` elsewhere"""
    B, L_, N, _ = t.shape
    out = torch.full((B * N, stride), fill, dtype=dtype)
    out[:, off: off + L_ * DH] = t.permute(0, 2, 1, 3).reshape(B * N, L_ * DH).to(dtype)
    return out


def unpack(rows, B: int, N: int, off: int):
    return rows[:, off: off + L * DH].reshape(B, N, L, DH).permute(0, 2, 1, 3)


def outside(rows, off: int):
    """everything of packed rows that no head block covers"""
    return torch.cat([rows[:, :off], rows[:, off + L * DH:]], 1)


def pack_rows(t):
    """[B, L, N] -> [B N L] (lse, D)"""
    return t.permute(0, 2, 1).reshape(-1).contiguous()


def unpack_rows(t, B: int, N: int):
    return t.reshape(B, N, L).permute(0, 2, 1)


# ------------------------------------------------------------------------------------------------------------------------------ fp64 references
def forward_ref(q, k, v, mask, Z=None, scale: float = SCALE, extra=None, dropped_lse: bool = False):
    """fp64 band softmax.  extra = (k_x, v_x [B, L, 1, 64], rows [N] bool): one more key that `rows` see (witness: the next batch's first key)"""
    s = torch.einsum("blid,bljd->blij", q * scale, k)
    mask = mask.expand(s.shape) if mask.dim() < 4 else mask
    if extra is not None:
        kx, vx, rows = extra
        s = torch.cat([s, torch.einsum("blid,bljd->blij", q * scale, kx)], -1)
        mask = torch.cat([mask, rows.view(1, 1, -1, 1).expand(*s.shape[:3], 1)], -1)
        v = torch.cat([v, vx], 2)
        Z = None if Z is None else torch.cat([Z, torch.ones_like(Z[..., :1])], -1)
    sm = s.masked_fill(~mask, float("-inf"))
    m = sm.amax(-1, keepdim=True)
    e = torch.exp(sm - m)
    l = e.sum(-1, keepdim=True)
    P = e / l
    lse = (m + torch.log(l)).squeeze(-1)
    if dropped_lse:
        lse = (m + torch.log((e * Z).sum(-1, keepdim=True))).squeeze(-1)
    o = (P if Z is None else P * Z) @ v
    return dict(s=s, m=m.squeeze(-1), P=P, lse=lse, o=o, mask=mask)


def forward_bounds(q, k, v, ref, N: int, W: int, path: str, Z=None):
    """(bound of o [B, L, N, 64], bound of lse [B, L, N])"""
    c = PATHS[path]
    g = row_geometry(N, W)
    nk, T = g["nk"].double(), g["T"].double()
    P, s, m, o, lse, mask = ref["P"], ref["s"], ref["m"], ref["o"], ref["lse"], ref["mask"]
    A = torch.einsum("blid,bljd->blij", (q * SCALE).abs(), k.abs())
    zero = torch.zeros_like(s)
    gap = torch.where(mask, m.unsqueeze(-1) - s, zero)
    ec = (64 * c["chain"] * U + c["prod"]) * A + EXP_E * U + EXP_ARG * U * gap + ((T - 1) * EXP_E * U).view(1, 1, N, 1)
    Pec = P * ec
    common = torch.empty_like(o)
    for d in range(DH):
        x = v[..., d].unsqueeze(2) if Z is None else Z * v[..., d].unsqueeze(2)
        common[..., d] = (Pec * (x - o[..., d: d + 1]).abs()).sum(-1)
    drop = 0.0 if Z is None else 1.0
    PZ = P if Z is None else P * Z
    cl = torch.clamp(nk, max=18.0) + 2 * (T - 1)
    chain_o = ((c["chain"] * nk + T - 1 + drop) * U + c["prod"]).view(1, 1, N, 1)
    floor = 2 * nk.view(1, 1, N, 1) * TINY * v.abs().amax()
    bo = common + chain_o * (PZ @ v.abs()) + o.abs() * ((cl + 2) * U).view(1, 1, N, 1) + floor
    blse = Pec.sum(-1) + cl * U + LOG_E * U * (lse - m).abs() + U * lse.abs() + nk * TINY
    return SECOND * bo + 1e-300, SECOND * blse + 1e-300


def backward_ref(q, k, v, do, out, lse, mask, Z=None, no_D: bool = False, no_Z_dP: bool = False, kv_mask=None, unscaled_dq: bool = False):
    """fp64 (dq, dk, dv, D) from the out / lse the kernel is given.  kv_mask: the (query, key) pairs the dk / dv walk reaches (witnesses)."""
    qs = q * SCALE
    s = torch.einsum("blid,bljd->blij", qs, k)
    zero = torch.zeros_like(s)
    P = torch.where(mask, torch.exp(s - lse.unsqueeze(-1)), zero)
    D = (do * out).sum(-1)
    dP = do @ v.transpose(-1, -2)
    ZdP = dP if (Z is None or no_Z_dP) else Z * dP
    t = ZdP - (zero if no_D else D.unsqueeze(-1))
    dS = P * t
    PZ = P if Z is None else P * Z
    dq = (dS @ k) * (1.0 if unscaled_dq else SCALE)
    dSk, PZk = (dS, PZ) if kv_mask is None else (torch.where(kv_mask, dS, zero), torch.where(kv_mask, PZ, zero))
    return dict(dq=dq, dk=dSk.transpose(-1, -2) @ qs, dv=PZk.transpose(-1, -2) @ do, D=D, s=s, P=P, dP=dP, t=t, dS=dS, PZ=PZ)


def backward_bounds(q, k, v, do, out, lse, ref, N: int, W: int, path: str, Z=None):
    """bounds of dq, dk, dv [B, L, N, 64] and D [B, L, N]"""
    c = PATHS[path]
    g = row_geometry(N, W)
    nk, nq = g["nk"].double().view(1, 1, N, 1), g["nq"].double().view(1, 1, N, 1)
    drop = 0.0 if Z is None else 1.0
    s, P, dP, t, dS, PZ = ref["s"], ref["P"], ref["dP"], ref["t"], ref["dS"], ref["PZ"]
    qs = (q * SCALE).abs()
    dense = 64 * c["chain"] * U + c["prod"]
    A = torch.einsum("blid,bljd->blij", qs, k.abs())
    dD = 19 * U * (do * out).abs().sum(-1)
    eP = dense * A + EXP_E * U + EXP_ARG * U * torch.where(P > 0, (s - lse.unsqueeze(-1)).abs(), torch.zeros_like(s))
    ddP = dense * (do.abs() @ v.abs().transpose(-1, -2))
    ZdP = dP if Z is None else Z * dP
    Zf = 1.0 if Z is None else Z
    ddS = P * (eP * t.abs() + Zf * ddP + dD.unsqueeze(-1) + drop * U * ZdP.abs() + 2 * U * t.abs()) + TINY * t.abs()
    bdq = SCALE * (ddS @ k.abs() + (c["chain"] * nk * U + c["prod"]) * (dS.abs() @ k.abs()))
    bdk = ddS.transpose(-1, -2) @ qs + (c["chain"] * nq * U + c["prod"]) * (dS.abs().transpose(-1, -2) @ qs)
    bdv = (PZ * eP).transpose(-1, -2) @ do.abs() + ((c["chain"] * nq + drop) * U + c["prod"]) * (PZ.transpose(-1, -2) @ do.abs()) + nq * TINY * do.abs().amax()
    return dict(dq=SECOND * bdq + 1e-300, dk=SECOND * bdk + 1e-300, dv=SECOND * bdv + 1e-300, D=SECOND * dD + 1e-300)


# ------------------------------------------------------------------------------------------------------------------------------ one case: truth, bounds, witnesses
class Case:
    """everything of one (N, W, regime, dropout) that does not depend on the output under test: the fp64 truth, the fp32 out / lse the backward is
    given, both paths' bounds and every witness.  Built once (case()) and shared, never written to."""

    def __init__(self, N: int, W: int, regime: str, dropout: bool):
        self.N, self.W, self.regime, self.dropout, self.B = N, W, regime, dropout, batch_of(N)
        B = self.B
        self.ops = draw(N, W, regime)
        o = {n: t.double() for n, t in self.ops.items()}
        q, k, v, do = o["q"], o["k"], o["v"], o["do"]
        self.Z32 = drop_mask(B, N) if dropout else None
        Z = self.Z = None if self.Z32 is None else self.Z32.double()
        g = self.geo = row_geometry(N, W)
        mask = band(N, W)
        self.fwd = forward_ref(q, k, v, mask, Z)
        self.out32, self.lse32 = self.fwd["o"].float(), self.fwd["lse"].float()
        out, lse = self.out32.double(), self.lse32.double()
        self.bwd = backward_ref(q, k, v, do, out, lse, mask, Z)
        self.bounds = {}
        for path in PATHS:
            bo, blse = forward_bounds(q, k, v, self.fwd, N, W, path, Z)
            self.bounds[path] = dict(o=bo, lse=blse, **backward_bounds(q, k, v, do, out, lse, self.bwd, N, W, path, Z))
        # ---- forward witnesses: name -> dict(o, lse)
        f = lambda **kw: forward_ref(kw.pop("q", q), k, kw.pop("v", v), kw.pop("mask", mask), Z, **kw)
        q63 = q.clone()
        q63[..., DH - 1] = 0.0
        last_tile = torch.arange(N) >= LT * ((N - 1) // LT)
        wf = {
            "lower bound one key early": f(mask=band(N, W, lo_shift=-1)),
            "lower bound one key late": f(mask=band(N, W, lo_shift=1)),
            "diagonal key dropped": f(mask=band(N, W, drop_diag=True)),
            "key i+1 admitted": f(mask=band(N, W, hi_shift=1)),
            "two windows of look-back": f(mask=band(N, W, back=2)),
            "last head dimension missing": f(q=q63),
            "v of row j+1": f(v=torch.roll(v, -1, 2)),
            "v of head h+1": f(v=torch.roll(v, -1, 1)),
            "first key of the next batch visible": f(extra=(torch.roll(k, -1, 0)[:, :, :1], torch.roll(v, -1, 0)[:, :, :1], last_tile)),
            "scale omitted": f(scale=1.0),
        }
        if dropout:
            wf["lse of the dropped softmax"] = f(dropped_lse=True)
        self.wit_o = {n: r["o"] for n, r in wf.items() if n != "lse of the dropped softmax"}
        self.wit_lse = {n: r["lse"] for n, r in wf.items() if n not in ("v of row j+1", "v of head h+1")}
        # ---- backward witnesses: name -> dict(dq, dk, dv, D)
        bk = lambda **kw: backward_ref(q, k, v, do, out, lse, kw.pop("mask", mask), kw.pop("Z", Z), **kw)
        i, j = torch.arange(N)[:, None], torch.arange(N)[None, :]
        next_window = i <= (j // W + 1) * W - 1                                 # kv walk that stops one window early
        walked = i < LT * torch.maximum(g["qt_hi"], torch.arange(N) // LT + 1)[None, :]    # ... one query tile early (the key's own tile stays)
        wb = {
            "D omitted": bk(no_D=True),
            "dq without the final scale": bk(unscaled_dq=True),
            "dk missing the following window": bk(kv_mask=next_window),
            "dk/dv missing the last query tile": bk(kv_mask=walked),
            "lower bound one key early": bk(mask=band(N, W, lo_shift=-1)),
            "diagonal key dropped": bk(mask=band(N, W, drop_diag=True)),
        }
        if dropout:
            wb["Z not applied to dP"] = bk(no_Z_dP=True)
            wb["mask of element e+1"] = bk(Z=torch.roll(Z.reshape(-1), -1, 0).reshape(Z.shape))
        skip = dict(dq=("dk missing the following window", "dk/dv missing the last query tile"), dk=("dq without the final scale",),
                    dv=("D omitted", "dq without the final scale", "Z not applied to dP"))          # (defects that cannot reach the output)
        self.wit_bwd = {o_: {n: r[o_] for n, r in wb.items() if n not in skip[o_]} for o_ in ("dq", "dk", "dv")}
        self.wit_bwd["D"] = {}
        self.fwd = {n: self.fwd[n] for n in ("o", "lse")}                       # keep the outputs only
        self.bwd = {n: self.bwd[n] for n in ("dq", "dk", "dv", "D")}

    @property
    def tag(self):
        return f"[{self.N}x{self.W} {self.regime}{' p=0.3' if self.dropout else ''}]"


@functools.lru_cache(maxsize=4)
def case(N: int, W: int, regime: str, dropout: bool = False) -> Case:
    return Case(N, W, regime, dropout)


# ------------------------------------------------------------------------------------------------------------------------------ checks
def within(what: str, got, ref, bnd, witnesses, ratios=None, asserted=None):
    """norm_bounds.assert_within; the names of the witnesses it asserts (the planted defect leaves the bound of the truth somewhere, decided from
    the two references alone) are added to `asserted`"""
    if asserted is not None:
        for name, wit in witnesses.items():
            if not float(((wit - ref).abs() / bnd).max()) <= 1.0:
                asserted.add(name)
    nb.assert_within(what, got, ref, bnd, witnesses, ratios)


def assert_rounded_once(what: str, y32, y_lp, asserted=None):
    """y_lp is the kernel's own fp32 output rounded once to bf16 -- equality; the witness (a truncating store) must differ"""
    y32, y_lp = y32.detach().cpu(), y_lp.detach().cpu()
    assert y_lp.dtype == torch.bfloat16 and y_lp.shape == y32.shape
    want = y32.to(torch.bfloat16)
    n = int((y_lp.float() != want.float()).sum())
    print(f"  {what}: {n} of {y32.numel()} elements differ from the fp32 output rounded once to bf16")
    assert n == 0, f"{what}: {n} of {y32.numel()} elements differ from the fp32 output rounded once to bf16"
    trunc = cb.truncated(y32.double(), "bf16").to(torch.bfloat16)
    if int((trunc.float() != want.float()).sum()):
        if asserted is not None:
            asserted.add("truncated store")
        assert not torch.equal(y_lp.float(), trunc.float())


def verify_forward(c: Case, path: str, got, ratios=None, asserted=None):
    """got = (o [B, L, N, 64], lse [B, L, N], o_lp or None) of one forward call"""
    o, lse, o_lp = got
    b = c.bounds[path]
    within(f"{c.tag} {path} o", o, c.fwd["o"], b["o"], c.wit_o, ratios, asserted)
    within(f"{c.tag} {path} lse", lse, c.fwd["lse"], b["lse"], c.wit_lse, ratios, asserted)
    if o_lp is not None:
        assert_rounded_once(f"{c.tag} {path} o_lp", o, o_lp, asserted)


def verify_backward(c: Case, path: str, got, ratios=None, asserted=None):
    """got = (dq, dk, dv [B, L, N, 64], D [B, L, N], dv_lp or None) of one backward call that was given c.out32 / c.lse32"""
    dq, dk, dv, D, dv_lp = got
    b = c.bounds[path]
    for name, t in (("D", D), ("dq", dq), ("dk", dk), ("dv", dv)):
        within(f"{c.tag} {path} {name}", t, c.bwd[name], b[name], c.wit_bwd[name], ratios, asserted)
    if dv_lp is not None:
        assert_rounded_once(f"{c.tag} {path} dv_lp", dv, dv_lp, asserted)


# ------------------------------------------------------------------------------------------------------------------------------ models of the kernels' arithmetic
_LOG2E = torch.tensor(float.fromhex("0x1.715476p+0"), dtype=torch.float32)
_ORDER = torch.tensor([f * 16 + g_ * 4 + r for f in range(4) for r in range(4) for g_ in range(4)])      # MFMA k order of the second GEMM: (f, r), then the lane group


def _exp32(x):
    """__expf: exp2 of the rounded product with the fp32 log2 e"""
    return torch.exp2(_LOG2E * x)


def _fma(a, b, acc):
    """fp32 fma: the product of two fp32 values is exact in fp64"""
    return (acc.double() + a.double() * b.double()).float()


def _split(x):
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def _gemm(acc, X, Y, path: str, terms=("lh", "hl", "hh")):
    """acc [.., M, n] + X [.., M, 64] @ Y [.., 64, n] the way the path evaluates it.  exact: an fma chain over the 64 steps in order.  split: hi / lo
    of both operands, per 32-step block the products lo*hi, hi*lo, hi*hi, each MFMA's 32 exact products summed exactly and added with one fp32
    rounding.  terms = ("hh",): a plain bf16 product (witness)."""
    if path == "exact":
        for d in range(X.shape[-1]):
            acc = _fma(X[..., d: d + 1], Y[..., d: d + 1, :], acc)
        return acc
    (Xh, Xl), (Yh, Yl) = _split(X), _split(Y)
    part = {"lh": (Xl, Yh), "hl": (Xh, Yl), "hh": (Xh, Yh)}
    for ks in range(X.shape[-1] // 32):
        sl = slice(32 * ks, 32 * ks + 32)
        for tname in terms:
            a, b = part[tname]
            acc = (acc.double() + a[..., sl].double() @ b[..., sl, :].double()).float()
    return acc


def _gemm_keys(acc, Pm, V, path: str, terms=("lh", "hl", "hh")):
    """the second GEMM of a tile: acc [.., M, 64] + Pm [.., M, 64 rows of the tile] @ V [.., 64, 64], rows in the MFMA's k order on the exact path"""
    if path == "exact":
        return _gemm(acc, Pm[..., _ORDER], V[..., _ORDER, :], path)
    return _gemm(acc, Pm, V, path, terms)


def _group_sum(p):
    """p [.., 64 elements of a tile] -> the sum in a lane group's order: lane g adds its sixteen values (f, r), then the two shuffles"""
    x = p.reshape(*p.shape[:-1], 4, 4, 4).transpose(-3, -2)            # [.., g, f, r]
    x = x.reshape(*p.shape[:-1], 4, 16)
    part = torch.zeros_like(x[..., 0])
    for e in range(16):
        part = part + x[..., e]
    part = part + part[..., [1, 0, 3, 2]]
    return (part + part[..., [2, 3, 0, 1]])[..., 0]


def _padded(t, Np: int, dim: int = 2):
    shape = list(t.shape)
    shape[dim] = Np - shape[dim]
    return torch.cat([t, torch.zeros(shape, dtype=t.dtype)], dim)


def _tiles(N: int, W: int):
    nt = -(-N // LT)
    Np = nt * LT
    i = torch.arange(Np)
    q0 = (i // LT) * LT
    kt_lo = ((q0 // W - 1).clamp(min=0) * W) // LT
    kt_hi = torch.clamp(q0 + LT - 1, max=N - 1) // LT
    lo = (i // W - 1).clamp(min=0) * W
    last_key = torch.clamp(q0 + LT - 1, max=N - 1)
    qt_hi = torch.clamp((last_key // W + 2) * W - 1, max=N - 1) // LT
    return nt, Np, i, kt_lo, kt_hi, lo, qt_hi


def _allowed(i, j, lo_i, N):
    """la_allowed for query rows i [R] (lower bounds lo_i [R]) x keys j [64]"""
    return (j[None, :] <= i[:, None]) & (j[None, :] >= lo_i[:, None]) & (j[None, :] < N) & (i[:, None] < N)


def _zpad(Z, Np):
    return None if Z is None else _padded(_padded(Z, Np, 2), Np, 3)


def model_forward(q, k, v, N: int, W: int, path: str, Z=None, terms=("lh", "hl", "hh")):
    """local_attn_q_exact<0> / local_attn_q_split_body<0> in fp32 torch arithmetic, key tile by key tile: (o, lse)"""
    B = q.shape[0]
    nt, Np, i, kt_lo, kt_hi, lo, _ = _tiles(N, W)
    qs, k, v, Z = _padded(q * SCALE, Np), _padded(k, Np), _padded(v, Np), _zpad(Z, Np)
    m_run = torch.full((B, L, Np), -1e30, dtype=torch.float32)
    l_run = torch.zeros(B, L, Np)
    acc = torch.zeros(B, L, Np, DH)
    for kt in range(nt):
        r = ((kt_lo <= kt) & (kt <= kt_hi)).nonzero().squeeze(1)
        if r.numel() == 0:
            continue
        j = kt * LT + torch.arange(LT)
        K, V = k[:, :, j], v[:, :, j]
        s = _gemm(torch.zeros(B, L, r.numel(), LT), qs[:, :, r], K.transpose(-1, -2), path, terms)
        s = s.masked_fill(~_allowed(i[r], j, lo[r], N), float("-inf"))
        m_new = torch.maximum(m_run[:, :, r], s.amax(-1).clamp(min=-1e30))
        alpha = _exp32(m_run[:, :, r] - m_new)
        p = _exp32(s - m_new.unsqueeze(-1))
        l_run[:, :, r] = l_run[:, :, r] * alpha + _group_sum(p)
        m_run[:, :, r] = m_new
        if Z is not None:
            p = p * Z[:, :, r][..., j]
        acc[:, :, r] = _gemm_keys(acc[:, :, r] * alpha.unsqueeze(-1), p, V, path, terms)
    o = acc * (1.0 / l_run).unsqueeze(-1)
    return o[:, :, :N], (m_run + torch.log(l_run))[:, :, :N]


def model_backward(q, k, v, do, out, lse, N: int, W: int, path: str, Z=None, terms=("lh", "hl", "hh")):
    """local_attn_q_*<1> then local_attn_kv_* (which reads the D the first wrote) in fp32 torch arithmetic: (dq, dk, dv, D)"""
    B = q.shape[0]
    nt, Np, i, kt_lo, kt_hi, lo, qt_hi = _tiles(N, W)
    qs, k, v, do, out, lse, Z = _padded(q * SCALE, Np), _padded(k, Np), _padded(v, Np), _padded(do, Np), _padded(out, Np), _padded(lse, Np), _zpad(Z, Np)
    prod = (do * out).reshape(B, L, Np, 16, 4)                      # lane g adds d = 4 dd + g in order, then the two shuffles
    part = torch.zeros(B, L, Np, 4)
    for dd in range(16):
        part = part + prod[..., dd, :]
    part = part + part[..., [1, 0, 3, 2]]
    D = (part + part[..., [2, 3, 0, 1]])[..., 0]
    acc = torch.zeros(B, L, Np, DH)
    for kt in range(nt):
        r = ((kt_lo <= kt) & (kt <= kt_hi)).nonzero().squeeze(1)
        if r.numel() == 0:
            continue
        j = kt * LT + torch.arange(LT)
        K, V = k[:, :, j], v[:, :, j]
        zero = torch.zeros(B, L, r.numel(), LT)
        s = _gemm(zero, qs[:, :, r], K.transpose(-1, -2), path, terms)
        dp = _gemm(zero, do[:, :, r], V.transpose(-1, -2), path, terms)
        p = _exp32(s.masked_fill(~_allowed(i[r], j, lo[r], N), float("-inf")) - lse[:, :, r].unsqueeze(-1))
        zdp = dp if Z is None else Z[:, :, r][..., j] * dp
        acc[:, :, r] = _gemm_keys(acc[:, :, r], p * (zdp - D[:, :, r].unsqueeze(-1)), K, path, terms)
    dq = acc * SCALE
    dk, dv = torch.zeros(B, L, Np, DH), torch.zeros(B, L, Np, DH)
    ktile = i // LT
    for qt in range(nt):
        r = ((ktile <= qt) & (qt <= qt_hi)).nonzero().squeeze(1)   # the key rows whose block walks query tile qt
        if r.numel() == 0:
            continue
        iq = qt * LT + torch.arange(LT)
        Q, Gd = qs[:, :, iq], do[:, :, iq]
        zero = torch.zeros(B, L, r.numel(), LT)
        s = _gemm(zero, k[:, :, r], Q.transpose(-1, -2), path, terms)          # [key rows, queries of the tile]
        dp = _gemm(zero, v[:, :, r], Gd.transpose(-1, -2), path, terms)
        ok = _allowed(iq, i[r], lo[iq], N).transpose(0, 1)
        p = _exp32(s.masked_fill(~ok, float("-inf")) - lse[:, :, iq].unsqueeze(2))
        if Z is None:
            ds = p * (dp - D[:, :, iq].unsqueeze(2))
        else:
            z = Z[:, :, iq][..., r].transpose(-1, -2)
            ds = p * (z * dp - D[:, :, iq].unsqueeze(2))
            p = p * z
        dv[:, :, r] = _gemm_keys(dv[:, :, r], p, Gd, path, terms)
        dk[:, :, r] = _gemm_keys(dk[:, :, r], ds, Q, path, terms)
    return dq[:, :, :N], dk[:, :, :N], dv[:, :, :N], D[:, :, :N]


# ------------------------------------------------------------------------------------------------------------------------------ decode step
def _rot(x):
    h = x.shape[-1] // 2
    return torch.cat([-x[..., h:], x[..., :h]], -1)


def draw_step(W: int, t: int, N: int, seed: int = 0):
    """one decode step, fp32 on the CPU: qkv [B, 3 inner] (q | k | v column blocks, the local heads behind G FAVOR+ heads), the rotary tables [N, 64],
    the caches [B, L, N, 64] with given rotated keys / values on [lo, t) and NaN everywhere else"""
    B = 2
    inner = (G + L) * DH
    gen = torch.Generator().manual_seed(seed + 17 * W + t)
    qkv = torch.randn(B, 3 * inner, generator=gen)
    fr = torch.einsum("i,j->ij", torch.arange(N, dtype=torch.float32), 1.0 / (10000 ** (torch.arange(0, DH, 2).float() / DH)))
    fr = torch.cat((fr, fr), -1)
    lo = max(0, (t // W - 1) * W)
    kc, vc = torch.full((B, L, N, DH), float("nan")), torch.full((B, L, N, DH), float("nan"))
    kc[:, :, lo:t], vc[:, :, lo:t] = torch.randn(B, L, t - lo, DH, generator=gen), torch.randn(B, L, t - lo, DH, generator=gen)
    return dict(qkv=qkv, cos=fr.cos().contiguous(), sin=fr.sin().contiguous(), kc=kc, vc=vc, lo=lo, W=W, t=t, N=N, B=B, inner=inner)


def step_heads(ops, dtype=torch.float64):
    """(q, k, v [B, L, 64]) of the local heads"""
    B, inner = ops["B"], ops["inner"]
    x = ops["qkv"].to(dtype)
    return tuple(x[:, n * inner + G * DH: n * inner + (G + L) * DH].reshape(B, L, DH) for n in range(3))


def step_ref(ops, lo=None, with_current: bool = True, rotate_key: bool = True, scale: float = SCALE):
    """fp64: dict(out [B, L, 64], kt (the rotated key), P, s, m, vals, keys, sq)"""
    t = ops["t"]
    lo = ops["lo"] if lo is None else lo
    q, k, v = step_heads(ops)
    cs, sn = ops["cos"][t].double(), ops["sin"][t].double()
    sq = (q * cs + _rot(q) * sn) * scale
    kt = k * cs + _rot(k) * sn
    keys = torch.cat([ops["kc"][:, :, lo:t].double(), (kt if rotate_key else k).unsqueeze(2)], 2)
    vals = torch.cat([ops["vc"][:, :, lo:t].double(), v.unsqueeze(2)], 2)
    if not with_current and t > lo:
        keys, vals = keys[:, :, :-1], vals[:, :, :-1]
    s = torch.einsum("bld,bljd->blj", sq, keys)
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    P = e / e.sum(-1, keepdim=True)
    return dict(out=torch.einsum("blj,bljd->bld", P, vals), kt=kt, v=v, P=P, s=s, m=m, keys=keys, vals=vals, sq=sq, q=q, k=k, cs=cs, sn=sn)


def step_bounds(ops, ref):
    """(bound of out, bound of kc[t])"""
    q, k, cs, sn, sq, keys, vals, P, s, m, out = (ref[n] for n in ("q", "k", "cs", "sn", "sq", "keys", "vals", "P", "s", "m", "out"))
    nk = keys.shape[2]
    dsq = SCALE * 2 * U * ((q * cs).abs() + (_rot(q) * sn).abs()) + 3 * U * sq.abs()
    dkt = 2 * U * ((k * cs).abs() + (_rot(k) * sn).abs())
    ds = 64 * U * torch.einsum("bld,bljd->blj", sq.abs(), keys.abs()) + torch.einsum("bld,bljd->blj", dsq, keys.abs())
    ds[..., -1] += (sq.abs() * dkt).sum(-1)
    ep = ds + EXP_E * U + EXP_ARG * U * (m - s)
    common = ((P * ep).unsqueeze(-1) * (vals - out.unsqueeze(2)).abs()).sum(2)
    chain_acc, chain_sum = -(-nk // 16) + 16, -(-nk // 1024) + 6 + 16 + 1
    bout = common + chain_acc * U * torch.einsum("blj,bljd->bld", P, vals.abs()) + out.abs() * chain_sum * U + 2 * nk * TINY * vals.abs().amax()
    return SECOND * bout + 1e-300, SECOND * dkt + 1e-300


def model_step(ops):
    """local_attn_step_kernel in fp32 torch arithmetic: (out [B, L, 64], kc[t], vc[t])"""
    t, lo = ops["t"], ops["lo"]
    q, k, v = step_heads(ops, torch.float32)
    cs, sn = ops["cos"][t], ops["sin"][t]
    sq = (q * cs + _rot(q) * sn) * torch.tensor(DH, dtype=torch.float32).rsqrt()
    kt = k * cs + _rot(k) * sn
    keys = torch.cat([ops["kc"][:, :, lo:t], kt.unsqueeze(2)], 2)
    vals = torch.cat([ops["vc"][:, :, lo:t], v.unsqueeze(2)], 2)
    B, nk = keys.shape[0], keys.shape[2]
    d = torch.zeros(B, L, nk)
    for e in range(16):
        for c in (3, 2, 1, 0):
            d = _fma(sq[..., 4 * e + c].unsqueeze(-1), keys[..., 4 * e + c], d)
    mx = d.amax(-1, keepdim=True)
    p = _exp32(d - mx)
    n2 = -(-nk // 1024) * 1024
    pp = _padded(p, n2, 2).reshape(B, L, n2 // 1024, 16, 64)         # thread = (wave, lane): its keys tid, tid + 1024
    th = torch.zeros(B, L, 16, 64)
    for trip in range(n2 // 1024):
        th = th + pp[:, :, trip]
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        th = th + th[..., lane ^ o]
    tot = torch.zeros(B, L)
    for w in range(16):
        tot = tot + th[:, :, w, 0]
    n3 = -(-nk // 16) * 16
    p16, v16 = _padded(p, n3, 2).reshape(B, L, n3 // 16, 16), _padded(vals, n3, 2).reshape(B, L, n3 // 16, 16, DH)
    acc = torch.zeros(B, L, 16, DH)                                   # wave wv adds its keys wv, wv + 16, ... in order
    for step in range(n3 // 16):
        acc = _fma(p16[:, :, step].unsqueeze(-1), v16[:, :, step], acc)
    o = torch.zeros(B, L, DH)
    for w in range(16):
        o = o + acc[:, :, w]
    return o / tot.unsqueeze(-1), kt, v


def verify_step(ops, got, ratios=None, asserted=None):
    """got = (out [B, L, 64], kc, vc [B, L, N, 64]) after one call on copies of ops' caches"""
    W, t, lo = ops["W"], ops["t"], ops["lo"]
    tag = f"[step W={W} t={t}]"
    out, kc, vc = (x.detach().cpu() for x in got)
    ref = step_ref(ops)
    bout, bk = step_bounds(ops, ref)
    wit = {"scale omitted": step_ref(ops, scale=1.0)["out"], "unrotated key": step_ref(ops, rotate_key=False)["out"]}
    if t > lo:
        wit["current key dropped"] = step_ref(ops, with_current=False)["out"]
    if t > lo + 1:
        wit["lower bound one key late"] = step_ref(ops, lo=lo + 1)["out"]
    within(f"{tag} out", out, ref["out"], bout, wit, ratios, asserted)
    within(f"{tag} kc", kc[:, :, t], ref["kt"], bk, {"unrotated key": ref["k"]}, ratios, asserted)
    assert torch.equal(vc[:, :, t], step_heads(ops, torch.float32)[2]), f"{tag}: vc[t] is not a copy of v"
    for name, after, before in (("kc", kc, ops["kc"]), ("vc", vc, ops["vc"])):
        rows = torch.arange(ops["N"]) != t
        assert torch.equal(after[:, :, rows].view(torch.int32), before[:, :, rows].view(torch.int32)), f"{tag}: {name} changed outside row t"


# ------------------------------------------------------------------------------------------------------------------------------ the docstring's table
def _table():
    rows = []
    for fam, outs in (("exact", ("o", "lse", "D", "dq", "dk", "dv")), ("split", ("o", "lse", "D", "dq", "dk", "dv")), ("step", ("out", "kc"))):
        for src, name in (("model", "model (CPU)"), ("mi355x", "MI355X kernels")):
            vals = MEASURED[src][fam]
            rows.append(f"    {fam:6s} {name:15s} " + "  ".join(f"{o_} {vals[o_]:.3g}" if o_ in vals else f"{o_} -" for o_ in outs))
    return "\n".join(rows)


__doc__ = __doc__ % dict(table=_table())
