"""Element-wise fp64 error bounds for the fused FAVOR+ kernels (csrc/favor_fused.hip: the projection tiles, the pre-pass, both forms of the chunk
states, the prefix, scan A, scan B with the feature-map backward and the projection adjoint, the paired launches, the key fix-up and dden), the
planted-defect witnesses an output must fail, and an fp32 / split-bf16 model of the kernels' arithmetic at MFMA granularity
(tests/test_favor_bounds_cpu.py holds the model to the same bounds; tests/test_favor_bounds_gpu.py holds the kernels to them).

Operation (oracle/performer_ref.py: softmax_kernel + causal_linear_attention), per batch b and head g, x a row of q or k, Ps [m, 64] the fp32 matrix the
kernel is given (data normaliser folded in; the reference sees it exactly):
    dd = Ps x,    h = c2half |x|^2,    phi_q = R exp(dd - h - max_f dd) + REPS,    phi_k = R exp(dd - h - gmax) + REPS       (gmax over ALL keys)
    A_ij = phi_q(i).phi_k(j) (j <= i),   den_i = sum_j A_ij + DEN_EPS sum_f phi_q(i)[f],   out_i = sum_j A_ij v_j / den_i,   inv_i = 1 / den_i
The constants are the kernel's own fp32 values taken as exact operands (fused_common / sa_favor_fused_prepass): R = 1 / sqrtf(m), REPS = R * 1e-4f,
c = powf(64, -0.25f), c2 = c * c, c2half = 0.5f * c * c, DEN_EPS = 1e-6f, EX_CONST = 1e-6f.  c is within one ulp (2 U relative) of 2^-1.5 whatever
powf the host has, so c2 and c2half are within C2_REL = 5 U (twice 2 U and the product's rounding) of 1/8 and 1/16; the reference uses the fp32
value numpy's powf gives and every term that carries c2 or c2half adds C2_REL of it, so a host powf that is one ulp off still passes.

The three stages are bounded in isolation: the pre-pass against fp64; the forward from the pre-pass outputs it is GIVEN (offq, offk, gmax are ABI
inputs of sa_favor_fused_fwd); the backward from fp32 attn and inv (the fp64 forward rounded once), the pre-pass outputs and amq.

Constants, from the code:
    U = 2^-24                 one fp32 rounding (conv_bounds.U32).
    SPLIT                     local_attn_bounds.SPLIT, per product of two split operands (split_pair on both sides).  On a bf16-representable
                              projection (flag word 0, PT_FLAG_OFF) P_lo = 0 and its residual is 0: of the three dropped terms only (ah) rb is left,
                              SPLIT / 3, and the chain has two products per term instead of three.  This holds for the two GEMMs that take the
                              projection tiles: dd (feat_slab / favor_prepass_kernel: products()) and dx (tile_cols_gemm(dxa, sPc, .., plo0)).
    chain(n) = 3 n U          n terms through mfma_f32_16x16x32_bf16 with three products per term, as local_attn_bounds counts them.
    bdd_f = (chain(64) + SPLIT) sum_d |Ps_fd| |x_d|          the six MFMAs of a dd accumulator (products(): ks = 0, 1 times hi*lo, lo*hi, hi*hi).
    EXP_E, EXP_ARG            local_attn_bounds: __expf = exp2 of a rounded product; EXP_ARG covers the rounding of the subtraction F - off too.
    DIV = 3                   1.f / part: at most 2.5 ulp if the build does not round it correctly.
    SECOND = 1.01             every bound is first order; the largest relative term (bdd in the hot regime) is 2e-3.

Pre-pass (favor_prepass_kernel).  ss = |x|^2 is an fma chain of sixteen per lane and two shuffles, times c2half: (18 + 1) U + C2_REL on h.
    offk:  |offk - h| <= (19 U + C2_REL) h
    offq:  |offq - h - max_f dd| <= (19 U + C2_REL) h + max_f bdd_f + U |offq|          (mx is the kernel's own dd at its pick; the sum rounds once)
    amq:   dd64[amq] >= max dd64 - (bdd[amq] + bdd[argmax64]); EQUAL to the fp64 argmax on every row where dd64[a] - dd64[f] > bdd[a] + bdd[f] for
           all f != a (the rows that fail this are `ambiguous`: at most 1 %% of a case's query rows, counted in the CPU test)
    gmax:  the decoded flat index (head row * LDF + feature) EQUALS the fp64 one (its margin over every other element exceeds the two bounds:
           asserted on the CPU), the value lies within bdd of it.

Forward (favor_fstate_kernel + favor_fprefix_kernel or favor_fstate_seq_kernel, then favor_fout_a_kernel).  A feature E + REPS, E = R exp(arg), has
    e = E (bdd + EXP_E U + EXP_ARG U |arg| + [keys] U |offk + gmax|) + U phi + R TINY            (load_x_operand adds offk + gmax; fmaf rounds once)
The same bit-identical features build numerator and denominator (feat_slab2 makes both maps in one walk), so with a_ij = e_q(i).phi_k(j) + phi_q(i).e_k(j)
    bout_id = sum_j a_ij |v_jd - o_id| / den_i + DEN_EPS sum_f e_q |o_id| / den_i + g_num(i) sum_j A_ij |v_jd| / den_i + (g_den(i) + (DIV + 1) U) |o_id|
    binv_i  = inv_i (sum_j a_ij / den_i + DEN_EPS sum_f e_q / den_i + g_den(i) + DIV U)
    g_num(i) = 2 SPLIT + chain(m) + chain(64 (c_i + 1))       c_i = i // 64 chunks in front of the row's own.  Inter-chunk: feat_to_tile x
               f_stage_values (SPLIT), the state's chain, tile_stage x acc_to_operand (SPLIT), chain(m) over the slabs; intra-chunk: the pair
               products (SPLIT, chain(m)), acc_to_operand x f_stage_values (SPLIT), chain(64) into the same accumulator.
    g_den(i) = SPLIT + chain(64 c_i) + chain(m) + (LDF / 4 + 19) U        z_prev (mfma3 with the exact weights 1), z + den_eps, the fmaf chain of a
               lane over its LDF / 4 features, sixteen pair products and two shuffles; the pair products carry SPLIT + chain(m).
The state chain is derived for the SEQUENTIAL form (the accumulator runs through all c_i chunks: chain(64 c_i)); the parallel form's chain(64) per
chunk plus c_i - 1 prefix additions lies below it, so one bound holds for both.  attn_lp must EQUAL the kernel's own attn rounded once.

Backward.  c_i = dattn_i inv_i, dden_i = -(dattn_i.attn_i) inv_i, W_ij = v_j.c_i + dden_i, Wabs_ij = sum_d |v_jd c_id| + |dden_i|:
    dphi_q(i) = sum_{j<=i} W_ij phi_k(j) + dden_i EX_CONST,    dphi_k(j) = sum_{i>=j} W_ij phi_q(i),    v = (phi - REPS) dphi,    t = sum_f v
    dq_i = sum_f v_f Ps[f] - t Ps[amq_i] - t c2 q_i,    dk_j = sum_f v_f Ps[f] - t c2 k_j  (- (sum of all t) Ps[f*] on the row of gmax),    dv_j = sum_{i>=j} A_ij c_i
    bdden_i = 9 U sum_d |dattn_id attn_id| inv_i                          (favor_fdden_v4_kernel: a product and three fmas, four shuffles, the product with inv)
    bdphi   = sum Wabs e_phi + g_B sum Wabs phi + sum bdden_i phi (+ bdden_i EX_CONST)
    g_B     = 2 SPLIT + chain(64 c) + 2 chain(64) + 6 U      the state (SPLIT, its chain), T_prev.c_i over d (SPLIT, chain(64)) or W (SPLIT, chain(64), the
              roundings of c and of + e) then phi.W over the chunk (SPLIT, chain(64)), zf * z and the two additions.  c counts the chunks in front in
              scan order: i // 64 for dq, (N - 1 - j) // 64 for the reversed scans.
    bv      = (e_phi + U E) |dphi| + E bdphi + U |v|,      bt = sum_f bv + (LDF / 4 + 2) U sum_f |v|              (tp: a lane's chain, two shuffles)
    bdx_d   = sum_f bv_f |Ps_fd| + (chain(m) + SPLIT + 2 U) sum_f |v_f Ps_fd| + bt (|Ps[am]_d| + c2 |x_d|) + 4 U |t Ps[am]_d| + (4 U + C2_REL) |t| c2 |x_d|
    fix-up  + bT |Ps[f*]_d| + 2 U |T Ps[f*]_d| + U |dk_d|,   bT = sum bt + (ceil(nblk / 64) + 12) U sum |t|      (wave_sum over sixteen live lanes and the
              four wave partials per block; favor_fkey_fix_kernel: ceil(nblk / 64) additions per lane, six shuffles)
    bdv_jd  = sum_i a_ij |c_id| + (2 SPLIT + chain(m) + chain(64 (c + 1)) + U) sum_i A_ij |c_id|
The three terms of dq / dk cancel (sum_f v_f (Ps[f] - Ps[am]) with most of the weight near the stabiliser row): the bound carries their absolute sum,
as the kernels' split products of the separate terms do.  What that leaves resolvable, from the fp64 references (the CPU test prints both figures per
case and output): the share of elements whose bound exceeds the tensor's own maximum is 0 except where SHARE_CAP says otherwise (dq and dk vanish at
N = 1; dq is lost in the offset and hot regimes, dk on 4.4 %% of the hot 150-row case), and the median bound / max |ref| of the flat cases is
1.5e-3 .. 1.1e-2 for dq, 4e-6 .. 4.5e-4 for dk, 7e-5 for dv, 1.4e-4 for out: a defect of a few per cent of dq's maximum on one element is seen, one
of 1e-3 in the others.
tsum_ws is an output of its own: each per-block partial against the sum of its rows' t.  On the row of the global maximum the plain dk bound has to
carry bT, every row's bound at once; Stage.verify_fixup therefore judges that row a second time from the partials the fix-up launch was GIVEN
(their fp64 sum times Ps[f*], the (ceil(nblk / 64) + 6) roundings of adding them), which resolves a partial that the sum misses.
dq_lp, dk_lp, dv_lp must EQUAL the fp32 outputs rounded once, the fix-up row included; columns outside the global heads stay bitwise untouched.

Witnesses (WITNESSES) are fp64 evaluations with one planted defect, asserted to fail wherever they leave the truth's bound and printed otherwise.
"rows >= N of the last chunk contributing" stands with the backward: in the forward those rows come after every valid row and the prefix is
exclusive, so no output can see them; in the reversed scans they come first, and reading them as copies of row 0 instead of zeros reaches every key.
den_eps omitted was expected below resolution; the early rows of every case resolve it (z is only (i + 1) REPS on the features the exponential leaves empty).

Worst max |err| / bound over every case (the threshold is the bound itself, ratio <= 1; MEASURED below):
%(table)s
The model sums each MFMA's 32 products exactly and rounds once; it takes the kernels' product order, the second splits, the slab loop, both
chunk-state forms, the prefix, the lane orders of den, tp, the block sums and the fix-up sum.  The kernels sit within a tenth of the model's figures
on every output and on the same digits for dq, dk, dv, tsum and offk.  The ratios are far below 1 because chain() charges one rounding per product
in the worst order where an MFMA rounds 32 products once, and because the bounds are sums of absolute values.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import conv_bounds as cb
import local_attn_bounds as lb
import norm_bounds as nb
from oracle import performer_ref as P

U = cb.U32
TINY = 2.0 ** -126
SPLIT, EXP_E, EXP_ARG = lb.SPLIT, lb.EXP_E, lb.EXP_ARG
SECOND = 1.01
DIV = 3.0
DH, CH = 64, 64
C32 = np.float32(64.0) ** np.float32(-0.25)
C2 = float(C32 * C32)
C2HALF = float(np.float32(0.5) * C32 * C32)
C2_REL = 5 * U
DEN_EPS = float(np.float32(1e-6))
EX_CONST = float(np.float32(1e-6))
AMBIGUOUS_CAP = 0.01
# the share of an output's elements whose bound may exceed the reference tensor's own maximum: 0 unless stated here (output -> "N1" or regime -> share).
# At N = 1 out = v_0 whatever q and k are: dq = dk = 0.  In the offset regime every key but one is left with its eps (out is a running mean of v, which
# does not depend on q) and in the hot regime one feature carries a query row, the one whose Ps[f] - Ps[amq] is zero: dq is what is left of three
# cancelling terms and the kernels' own split products of those terms are of its size.  Fixed from the fp64 references (tests/test_favor_bounds_cpu.py).
SHARE_CAP = dict(dq=dict(N1=1.0, offset=1.0, hot=1.0), dk=dict(N1=1.0, hot=0.05, offset=1e-3))


def ratio_consts(m: int):
    """(R, REPS) as fused_common computes them in fp32"""
    r = np.float32(1.0) / np.sqrt(np.float32(m))
    return float(r), float(r * np.float32(1e-4))


def ldf_of(m: int) -> int:
    return (m + 15) // 16 * 16


def chain(n):
    return 3 * n * U


# worst max |err| / bound per output: the model on the CPU, the kernels on the MI355X (tests/test_favor_bounds_gpu.py, every case and route)
MEASURED = dict(
    model=dict(offq=0.0611, offk=0.149, gmax=0.0312, out=0.0754, inv=0.0896, dden=0.16, dq=0.0139, dk=0.267, dv=0.148, tsum=0.0753, fixrow=0.0212),
    mi355x=dict(offq=0.0577, offk=0.149, gmax=0.0321, out=0.0817, inv=0.0871, dden=0.152, dq=0.0139, dk=0.267, dv=0.148, tsum=0.0753, fixrow=0.0217),
)

# (B, G, N, m): what each reaches
SHAPES = {
    (1, 1, 1, 16): "one position, one fragment",
    (2, 2, 63, 64): "one slab (no double buffering), one row short of the chunk",
    (2, 2, 64, 64): "one slab, exactly one chunk",
    (2, 2, 65, 64): "one slab, a one-row second chunk",
    (2, 2, 130, 10): "m < 16: six masked features inside the only fragment",
    (2, 2, 129, 256): "slab-exact LDF, a one-row last chunk",
    (2, 2, 129, 272): "five full-width slabs, the row block beside the flag word",
    (1, 2, 77, 120): "the existing shape: a half-filled second slab",
    (2, 2, 150, 266): "the existing shape: one fragment with ten live features in the last slab",
    (2, 1, 333, 266): "six chunks, a prefix loop of more than one step",
    (5, 8, 70, 266): "B G = 40: the dispatcher's own sequential route",
}
REGIME_SHAPES = [(2, 2, 150, 266), (2, 2, 65, 64)]
BF16_SHAPES = [(2, 2, 150, 266), (2, 2, 65, 64)]
# (B, G, N, m, regime, bf16-representable projection)
CASES = [(*s, "flat", False) for s in SHAPES] + [(*s, r, False) for s in REGIME_SHAPES for r in ("hot", "offset")] + [(*s, "flat", True) for s in BF16_SHAPES]
IDS = [f"{B}x{G}x{N}x{m}-{r}{'-bf16' if p else ''}" for (B, G, N, m, r, p) in CASES]
NEW_SHAPES = [c for c in CASES if c[2] == 1 or c[3] not in (266, 120)]        # feature counts and N that the existing tests never ran


def routes(B: int, G: int):
    """the chunk-state forms a case runs: (name, favor_seq_always or None for the dispatcher's own choice)"""
    return [("natural_seq", None)] if B * G >= 40 else [("parallel", False), ("seq", True)]


# ABI call -> route -> the distinct launch names it must produce, sorted (tests/test_favor_bounds_gpu.py asserts them through _ffi.kernel_log)
KERNELS = {
    "proj_tiles": {r: ["favor_proj_tiles_kernel"] for r in ("parallel", "seq", "natural_seq")},
    "prepass": {r: ["favor_prepass_kernel"] for r in ("parallel", "seq", "natural_seq")},
    "fwd": dict(parallel=["favor_fout_a_kernel", "favor_fprefix_kernel", "favor_fstate_kernel"], seq=["favor_fout_a_kernel", "favor_fstate_seq_kernel"]),
    "bwd_state_kept": dict(parallel=["favor_fdden_v4_kernel", "favor_fkey_fix_kernel", "favor_fpair_b_a_kernel", "favor_fpair_b_state_kernel", "favor_fprefix_kernel"],
                           seq=["favor_fdden_v4_kernel", "favor_fkey_fix_kernel", "favor_fpair_b_a_kernel", "favor_fpair_seq_b_kernel"]),
    "bwd_state_null": dict(parallel=["favor_fdden_v4_kernel", "favor_fkey_fix_kernel", "favor_fout_b_kernel", "favor_fpair_b_a_kernel", "favor_fprefix_kernel",
                                     "favor_fstate_kernel"],
                           seq=["favor_fdden_v4_kernel", "favor_fkey_fix_kernel", "favor_fout_b_kernel", "favor_fpair_b_a_kernel", "favor_fstate_seq_kernel"]),
}
for _e in ("fwd", "bwd_state_kept", "bwd_state_null"):
    KERNELS[_e]["natural_seq"] = KERNELS[_e]["seq"]
# rows held by reference, not by a run of this file
KERNELS_BY_REFERENCE = {
    **{k: "co-launch twin: tied bit for bit to the separate launches by tests/test_favor_fused_gpu.py::test_colaunched_local_heads_equal_separate_launches"
       for k in ("favor_fout_a_la_kernel", "favor_fpair_b_state_la_kernel", "favor_fseq_la_kernel", "favor_fpair_seq_b_la_kernel", "favor_fpair_b_a_la_kernel")},
    "favor_fdden_kernel": "not reachable from aligned buffers (the scalar fallback for a misaligned dattn / attn pointer; the chunk kernels' 16-byte loads "
                          "make no promise for one)",
}

WITNESSES = {
    "fwd": ("causal mask admits j = i + 1", "diagonal pair dropped", "chunk prefix inclusive", "one chunk's state missing from the prefix",
            "padded features unmasked", "feature-map eps omitted", "den_eps omitted", "key stabiliser per batch", "v of head g+1",
            "first key of the next batch visible", "ratio omitted from the query map", "truncated store"),
    "bwd": ("dden omitted", "-t Ps[amq] dropped", "-t c2 x dropped", "fix-up on row r*+1", "fix-up on head g+1", "fix-up omitted", "tsum missing the last block",
            "reversed scan missing the last chunk", "(phi - r eps) replaced by phi", "c_scale (inv) not applied", "running-sum term dropped",
            "rows >= N of the last chunk contributing", "truncated store"),
    "arith": ("plain-bf16 product in the dd GEMM",),
}

# ------------------------------------------------------------------------------------------------------------------------------ layout
def pack(t, stride: int, off: int, fill=float("nan"), dtype=torch.float32):
    """[B, G, N, 64] -> rows [B N, stride] with the head blocks at column `off`, `fill` elsewhere"""
    B, G, N, _ = t.shape
    out = torch.full((B * N, stride), fill, dtype=dtype)
    out[:, off: off + G * DH] = t.permute(0, 2, 1, 3).reshape(B * N, G * DH).to(dtype)
    return out


def unpack(rows, B: int, G: int, N: int, off: int = 0):
    return rows[:, off: off + G * DH].reshape(B, N, G, DH).permute(0, 2, 1, 3)


def outside(rows, G: int, off: int = 0):
    return torch.cat([rows[:, :off], rows[:, off + G * DH:]], 1)


def pack_rows(t):
    """[B, G, N] -> [B N G] (offq, offk, amq, inv, dden)"""
    return t.permute(0, 2, 1).reshape(-1).contiguous()


def unpack_rows(t, B: int, G: int, N: int):
    return t.reshape(B, N, G).permute(0, 2, 1)


# ------------------------------------------------------------------------------------------------------------------------------ fp64 references
def features(dd, off, R, REPS):
    return R * torch.exp(dd - off.unsqueeze(-1)) + REPS


def causal_weights(N: int, kind: str = "ok"):
    """Wt[i, j]: how often key j reaches query i"""
    i, j = torch.arange(N)[:, None], torch.arange(N)[None, :]
    w = (j <= i).double()
    if kind == "j<=i+1":
        w = (j <= i + 1).double()
    elif kind == "no diagonal":
        w = (j < i).double()
    elif kind == "inclusive prefix":
        w = torch.where(i // CH == j // CH, (j <= i).double() + 1.0, w)          # the whole own chunk once more, through the prefix
    elif kind == "chunk missing":
        w = torch.where(j // CH == i // CH - 1, torch.zeros_like(w), w)
    elif kind == "reversed chunk missing":           # queries of the last chunk in scan order 0 (i >= N - 64) never reach the keys of the later chunks
        w = torch.where(((N - 1 - i) // CH == 0) & ((N - 1 - j) // CH > 0), torch.zeros_like(w), w)
    return w


def forward_ref(c, pre, Wt=None, reps=None, den_eps=DEN_EPS, gmax=None, v=None, r_q=None, pad_features: bool = False, next_batch_key: bool = False):
    """fp64 forward from the pre-pass outputs it is given: dict(out, inv, A, den, phi_q, phi_k)"""
    R, REPS = c.R, (c.REPS if reps is None else reps)
    Wt = causal_weights(c.N) if Wt is None else Wt
    v = c.o64["v"] if v is None else v
    g = pre["gmax"] if gmax is None else gmax                     # a float or [B, 1, 1]
    offk = pre["offk"] + g
    phi_q = features(c.ddq, pre["offq"], R if r_q is None else r_q, REPS)
    phi_k = features(c.ddk, offk, R, REPS)
    if pad_features and c.LDF > c.m:                               # dd = 0 on the LDF - m padded rows of the projection tiles
        z = torch.zeros(*c.ddq.shape[:-1], c.LDF - c.m, dtype=torch.float64)
        phi_q, phi_k = torch.cat([phi_q, features(z, pre["offq"], R, REPS)], -1), torch.cat([phi_k, features(z, offk, R, REPS)], -1)
    A = torch.einsum("bgif,bgjf->bgij", phi_q, phi_k) * Wt
    num, den = A @ v, A.sum(-1) + den_eps * phi_q.sum(-1)
    if next_batch_key:                                             # rows of the last chunk also see key 0 of batch b + 1
        rows = (torch.arange(c.N) >= CH * ((c.N - 1) // CH)).double()
        ax = torch.einsum("bgif,bgf->bgi", phi_q, torch.roll(phi_k, -1, 0)[:, :, 0]) * rows
        num, den = num + ax.unsqueeze(-1) * torch.roll(v, -1, 0)[:, :, :1], den + ax
    return dict(out=num / den.unsqueeze(-1), inv=1.0 / den, A=A, den=den, phi_q=phi_q, phi_k=phi_k)


def feature_errors(dd, bdd, off, off_err, R, REPS):
    arg = dd - off.unsqueeze(-1)
    E = R * torch.exp(arg)
    e = E * (bdd + EXP_E * U + EXP_ARG * U * arg.abs() + off_err.unsqueeze(-1)) + U * (E + REPS) + R * TINY
    return E, e


def forward_bounds(c, pre, ref):
    """(bound of out [B, G, N, 64], bound of inv [B, G, N], a [B, G, N, N], e_q, e_k)"""
    N, m, v = c.N, c.m, c.o64["v"]
    offk = pre["offk"] + pre["gmax"]
    _, e_q = feature_errors(c.ddq, c.bddq, pre["offq"], torch.zeros_like(pre["offq"]), c.R, c.REPS)
    _, e_k = feature_errors(c.ddk, c.bddk, offk, U * offk.abs(), c.R, c.REPS)
    Wt = causal_weights(N)
    a = (torch.einsum("bgif,bgjf->bgij", e_q, ref["phi_k"]) + torch.einsum("bgif,bgjf->bgij", ref["phi_q"], e_k)) * Wt
    A, den, out = ref["A"], ref["den"], ref["out"]
    eps_e = DEN_EPS * e_q.sum(-1)
    ci = (torch.arange(N) // CH).double()
    g_num = (2 * SPLIT + chain(m) + chain(CH * (ci + 1))).view(1, 1, N, 1)
    g_den = SPLIT + chain(CH * ci) + chain(m) + (c.LDF / 4 + 19) * U
    common = torch.empty_like(out)
    for d in range(DH):
        common[..., d] = (a * (v[..., d].unsqueeze(2) - out[..., d: d + 1]).abs()).sum(-1)
    d1 = den.unsqueeze(-1)
    bo = (common + eps_e.unsqueeze(-1) * out.abs()) / d1 + g_num * (A @ v.abs()) / d1 + (g_den + (DIV + 1) * U).view(1, 1, N, 1) * out.abs()
    binv = ref["inv"] * ((a.sum(-1) + eps_e) / den + g_den + DIV * U)
    return SECOND * bo + 1e-300, SECOND * binv + 1e-300, a, e_q, e_k


def backward_ref(c, pre, attn, inv, fwd, *, no_dden=False, no_stab=False, no_c2=False, fix="ok", tsum_drop_last=False, rev_missing=False,
                 phi_not_E=False, no_inv=False, no_running=False, pad_row0=False, bounds=False, fb=None):
    """fp64 backward from the fp32 attn / inv it is given, the pre-pass outputs and amq.  fwd = forward_ref's dict (phi_q, phi_k, A).
    bounds=True also returns the bounds (fb = forward_bounds' (a, e_q, e_k))."""
    B, G, N, m = c.B, c.G, c.N, c.m
    q, k, v, da, Ps = c.o64["q"], c.o64["k"], c.o64["v"], c.o64["dattn"], c.Ps64
    phi_q, phi_k = fwd["phi_q"], fwd["phi_k"]
    E_q, E_k = (phi_q, phi_k) if phi_not_E else (phi_q - c.REPS, phi_k - c.REPS)
    cs = da * inv.unsqueeze(-1)
    dden = torch.zeros_like(inv) if no_dden else -(da * attn).sum(-1) * inv
    tri = causal_weights(N)
    S = (N + CH - 1) // CH
    # ---- dq
    cq = da if no_inv else cs
    Wq = (cq @ v.transpose(-1, -2) + dden.unsqueeze(-1)) * tri
    if no_running:                                                 # dden_i reaches only the keys of the query's own chunk
        same = (torch.arange(N)[:, None] // CH == torch.arange(N)[None, :] // CH).double()
        Wq = (cq @ v.transpose(-1, -2) + dden.unsqueeze(-1) * same) * tri
    dphi_q = Wq @ phi_k + (0.0 if no_running else 1.0) * dden.unsqueeze(-1) * EX_CONST
    vq = E_q * dphi_q
    tq = vq.sum(-1)
    Pam = Ps[pre["amq"]]                                            # [B, G, N, 64]
    dq = vq @ Ps - (0.0 if no_stab else 1.0) * tq.unsqueeze(-1) * Pam - (0.0 if no_c2 else 1.0) * tq.unsqueeze(-1) * C2 * q
    # ---- dk, dv
    trk = causal_weights(N, "reversed chunk missing") if rev_missing else tri
    W = (cs @ v.transpose(-1, -2) + dden.unsqueeze(-1)) * trk
    dphi_k = W.transpose(-1, -2) @ phi_q
    Ak = fwd["A"] if not rev_missing else fwd["A"] * trk
    dv = Ak.transpose(-1, -2) @ cs
    if pad_row0:                                                   # the S 64 - N rows in front of the reversed scan read as copies of row 0
        npad = S * CH - N
        w0 = cs[:, :, :1] @ v.transpose(-1, -2) + dden[:, :, :1].unsqueeze(-1)          # [B, G, 1, N]
        dphi_k = dphi_k + npad * w0.transpose(-1, -2) * phi_q[:, :, :1]
        dv = dv + npad * torch.einsum("bgf,bgjf->bgj", phi_q[:, :, 0], phi_k).unsqueeze(-1) * cs[:, :, :1]
    vk = E_k * dphi_k
    tk = vk.sum(-1)
    dk = vk @ Ps - (0.0 if no_c2 else 1.0) * tk.unsqueeze(-1) * C2 * k
    T = tk.sum()
    if tsum_drop_last:                                             # block B G S - 1: batch B - 1, head G - 1, the last chunk in scan order = rows 0 .. N - 1 - 64 (S - 1)
        T = T - tk[B - 1, G - 1, : N - CH * (S - 1)].sum()
    b_, n_, g_, f_ = c.gmax_where
    if fix == "row+1":
        n_ = (n_ + 1) % N
    elif fix == "head+1":
        g_ = (g_ + 1) % G
    dk_nofix = dk.clone()
    if fix != "none":
        dk[b_, g_, n_] = dk[b_, g_, n_] - T * Ps[f_]
    res = dict(dden=dden, dq=dq, dk=dk, dv=dv)
    if not bounds:
        return res
    # ------------------------------------------------------------------ bounds
    a, e_q, e_k = fb
    pl = 1.0 / 3.0 if c.bf16 else 1.0
    ch_m = (2 if c.bf16 else 3) * m * U
    bdden = 9 * U * (da * attn).abs().sum(-1) * inv.abs()
    Wabs = (cs.abs() @ v.abs().transpose(-1, -2) + dden.abs().unsqueeze(-1)) * tri
    ci = (torch.arange(N) // CH).double()
    cr = ((N - 1 - torch.arange(N)) // CH).double()
    g_B = lambda cc: (2 * SPLIT + chain(CH * cc) + 2 * chain(CH) + 6 * U).view(1, 1, N, 1)
    PsA = Ps.abs()

    def dx_bound(E, e_phi, dphi, bdphi, x, stab):
        vv = E * dphi
        bv = (e_phi + U * E.abs()) * dphi.abs() + E.abs() * bdphi + U * vv.abs()
        t = vv.sum(-1, keepdim=True)
        bt = bv.sum(-1, keepdim=True) + (c.LDF / 4 + 2) * U * vv.abs().sum(-1, keepdim=True)
        b = bv @ PsA + (ch_m + pl * SPLIT + 2 * U) * (vv.abs() @ PsA) + bt * (stab + C2 * x.abs()) + 4 * U * t.abs() * stab + (4 * U + C2_REL) * t.abs() * C2 * x.abs()
        return b, bt, t

    bdphi_q = Wabs @ e_k + g_B(ci) * (Wabs @ phi_k) + bdden.unsqueeze(-1) * (tri @ phi_k + EX_CONST)
    bdq, _, _ = dx_bound(E_q, e_q, dphi_q, bdphi_q, q, Pam.abs())
    WabsT = Wabs.transpose(-1, -2)
    bdphi_k = WabsT @ e_q + g_B(cr) * (WabsT @ phi_q) + (tri.transpose(-1, -2) * bdden.unsqueeze(-2)) @ phi_q
    bdk, btk, tkk = dx_bound(E_k, e_k, dphi_k, bdphi_k, k, torch.zeros_like(k))
    nblk = B * G * S
    bT = btk.sum() + (math.ceil(nblk / 64) + 12) * U * tkk.abs().sum()
    aux = dict(tk=tk, btk=btk.squeeze(-1), tabs=tkk.abs().squeeze(-1), row_nofix=dk_nofix[b_, g_, n_].clone(), brow_nofix=bdk[b_, g_, n_].clone())
    bdk[b_, g_, n_] = bdk[b_, g_, n_] + bT * PsA[f_] + 2 * U * (T * Ps[f_]).abs() + U * dk[b_, g_, n_].abs()
    g_nr = (2 * SPLIT + chain(m) + chain(CH * (cr + 1)) + U).view(1, 1, N, 1)
    bdv = a.transpose(-1, -2) @ cs.abs() + g_nr * (fwd["A"].transpose(-1, -2) @ cs.abs())
    res["aux"] = aux
    res["bounds"] = dict(dden=SECOND * bdden + 1e-300, dq=SECOND * bdq + 1e-300, dk=SECOND * bdk + 1e-300, dv=SECOND * bdv + 1e-300)
    return res


# ------------------------------------------------------------------------------------------------------------------------------ one case
class Case:
    """what does not depend on the output under test: operands, the fp64 dd of queries and keys, their bounds, the fp64 argmax and global maximum.
    Built once (case()) and shared, never written to."""

    def __init__(self, B, G, N, m, regime="flat", bf16=False):
        self.B, self.G, self.N, self.m, self.regime, self.bf16 = B, G, N, m, regime, bf16
        self.LDF, self.S = ldf_of(m), (N + CH - 1) // CH
        self.R, self.REPS = ratio_consts(m)
        gen = torch.Generator().manual_seed(N + m)
        q, k, v, dattn = (torch.randn(B, G, N, DH, generator=gen) for _ in range(4))
        proj = P.gaussian_orthogonal_random_matrix(m, DH, gen)
        Ps = (proj * DH ** -0.25).float()
        if bf16:
            Ps = Ps.to(torch.bfloat16).float()
        self.planted = None
        if regime == "hot":
            q, k = q * 2.0, k * 2.0
        elif regime == "offset":                                   # the global maximum on a known row: batch B - 1, head G - 1, row N - 1 (the last chunk; row 64 at N = 65)
            d0 = int(Ps.abs().amax(0).argmax())
            f0 = int(Ps[:, d0].abs().argmax())
            k[B - 1, G - 1, N - 1, d0] += 16.0 * float(torch.sign(Ps[f0, d0]))
            self.planted = (B - 1, N - 1, G - 1)
        self.ops = dict(q=q, k=k, v=v, dattn=dattn, Ps=Ps.contiguous())
        self.o64 = {n: t.double() for n, t in self.ops.items()}
        self.Ps64 = self.o64["Ps"]
        q64, k64 = self.o64["q"], self.o64["k"]
        self.ddq = q64 @ self.Ps64.T
        self.ddk = k64 @ self.Ps64.T
        cdd = ((2 if bf16 else 3) * DH * U + (SPLIT / 3 if bf16 else SPLIT)) * SECOND
        self.bddq = cdd * (q64.abs() @ self.Ps64.abs().T)
        self.bddk = cdd * (k64.abs() @ self.Ps64.abs().T)
        self.hq, self.hk = C2HALF * (q64 ** 2).sum(-1), C2HALF * (k64 ** 2).sum(-1)
        # queries: argmax and ambiguity
        self.maxq, self.argq = self.ddq.max(-1)
        ba = self.bddq.gather(-1, self.argq.unsqueeze(-1))
        margin = (self.maxq.unsqueeze(-1) - self.ddq) - (ba + self.bddq)
        margin.scatter_(-1, self.argq.unsqueeze(-1), float("inf"))
        self.ambiguous = margin.amin(-1) <= 0
        # keys: the global maximum, its flat index (head row * LDF + feature) and its margin over every other element
        flat = self.ddk.permute(0, 2, 1, 3).reshape(-1)             # [(b N + n) G + g, m]
        top = int(flat.argmax())
        r_, f_ = divmod(top, m)
        bn, g_ = divmod(r_, G)
        b_, n_ = divmod(bn, N)
        self.gmax64, self.gmax_where, self.gmax_index = float(flat[top]), (b_, n_, g_, f_), r_ * self.LDF + f_
        bflat = self.bddk.permute(0, 2, 1, 3).reshape(-1)
        self.bgmax = float(bflat[top])
        mg = (flat[top] - flat) - (bflat[top] + bflat)
        mg[top] = float("inf")
        self.gmax_margin = float(mg.min())

    @property
    def tag(self):
        return f"[{self.B}x{self.G}x{self.N}x{self.m} {self.regime}{' bf16' if self.bf16 else ''}]"


@functools.lru_cache(maxsize=3)
def case(B, G, N, m, regime="flat", bf16=False) -> Case:
    return Case(B, G, N, m, regime, bf16)


# ------------------------------------------------------------------------------------------------------------------------------ checks
def within(what, got, ref, bnd, witnesses, ratios=None, asserted=None):
    if asserted is not None:
        for name, wit in witnesses.items():
            if not float(((wit - ref).abs() / bnd).max()) <= 1.0:
                asserted.add(name)
    nb.assert_within(what, got, ref, bnd, witnesses, ratios)


def verify_prepass(c: Case, got, ratios=None):
    """got = (offq, offk [B, G, N] fp32, amq [B, G, N] int, gmax value, gmax flat index).  Returns the `pre` dict the later stages are given."""
    offq, offk, amq, gval, gidx = got
    offq, offk, amq = offq.detach().cpu(), offk.detach().cpu(), amq.detach().cpu().long()
    bh = (19 * U + C2_REL) * SECOND
    within(f"{c.tag} offk", offk, c.hk, bh * c.hk + 1e-300, {"c2half omitted": c.hk / C2HALF}, ratios)
    refq = c.hq + c.maxq
    within(f"{c.tag} offq", offq, refq, bh * c.hq + c.bddq.amax(-1) + SECOND * U * refq.abs() + 1e-300,
           {"row maximum omitted": c.hq, "global instead of row maximum": c.hq + c.ddq.amax()}, ratios)
    assert int(amq.min()) >= 0 and int(amq.max()) < c.m, f"{c.tag}: amq outside [0, m)"
    picked, bp = c.ddq.gather(-1, amq.unsqueeze(-1)).squeeze(-1), c.bddq.gather(-1, amq.unsqueeze(-1)).squeeze(-1)
    ba = c.bddq.gather(-1, c.argq.unsqueeze(-1)).squeeze(-1)
    assert bool((picked >= c.maxq - (bp + ba)).all()), f"{c.tag}: amq picks a feature below the row maximum by more than the two dd bounds"
    wrong = (amq != c.argq) & ~c.ambiguous
    n_amb = int(c.ambiguous.sum())
    print(f"  {c.tag} amq: {int((amq != c.argq).sum())} rows differ from the fp64 argmax, {n_amb} of {c.ambiguous.numel()} rows are ambiguous")
    assert not bool(wrong.any()), f"{c.tag}: amq differs from the fp64 argmax on {int(wrong.sum())} unambiguous rows"
    assert gidx == c.gmax_index, f"{c.tag}: gmax index {gidx} (row {gidx // c.LDF}, feature {gidx % c.LDF}) != {c.gmax_index}"
    gerr = abs(float(gval) - c.gmax64) / c.bgmax
    print(f"  {c.tag} gmax: |err| / bound = {gerr:.3g}")
    if ratios is not None:
        ratios["gmax"] = max(ratios.get("gmax", 0.0), gerr)
    assert gerr <= 1.0, f"{c.tag}: gmax value off by {gerr:.3g} x its bound"
    return dict(offq=offq.double(), offk=offk.double(), amq=amq, gmax=float(gval))


class Stage:
    """the fp64 truth, bounds and witnesses of the forward and the backward of one case, from one set of pre-pass outputs"""

    def __init__(self, c: Case, pre):
        self.c, self.pre = c, pre
        B, G, N = c.B, c.G, c.N
        f = self.fwd = forward_ref(c, pre)
        self.bout, self.binv, a, e_q, e_k = forward_bounds(c, pre, f)
        self.attn32, self.inv32 = f["out"].float(), f["inv"].float()
        fw = lambda **kw: forward_ref(c, pre, **kw)
        wf = {
            "causal mask admits j = i + 1": fw(Wt=causal_weights(N, "j<=i+1")),
            "diagonal pair dropped": fw(Wt=causal_weights(N, "no diagonal")),
            "feature-map eps omitted": fw(reps=0.0),
            "den_eps omitted": fw(den_eps=0.0),
            "ratio omitted from the query map": fw(r_q=1.0),
        }
        if c.S > 1:
            wf["chunk prefix inclusive"] = fw(Wt=causal_weights(N, "inclusive prefix"))
            wf["one chunk's state missing from the prefix"] = fw(Wt=causal_weights(N, "chunk missing"))
        if c.LDF > c.m:
            wf["padded features unmasked"] = fw(pad_features=True)
        if B > 1:
            gb = (c.ddk.amax((1, 2, 3)) + (pre["gmax"] - c.gmax64)).view(B, 1, 1)
            wf["key stabiliser per batch"] = fw(gmax=gb)
            wf["first key of the next batch visible"] = fw(next_batch_key=True)
        if G > 1:
            wf["v of head g+1"] = fw(v=torch.roll(c.o64["v"], -1, 1))
        self.wit_out = {n: r["out"] for n, r in wf.items()}
        self.wit_inv = {n: r["inv"] for n, r in wf.items() if n != "v of head g+1"}
        attn, inv = self.attn32.double(), self.inv32.double()
        bk = lambda **kw: backward_ref(c, pre, attn, inv, f, **kw)
        self.bwd = bk(bounds=True, fb=(a, e_q, e_k))
        self.bb, self.aux = self.bwd.pop("bounds"), self.bwd.pop("aux")
        wb = {
            "dden omitted": bk(no_dden=True), "-t Ps[amq] dropped": bk(no_stab=True), "-t c2 x dropped": bk(no_c2=True),
            "fix-up omitted": bk(fix="none"), "(phi - r eps) replaced by phi": bk(phi_not_E=True), "c_scale (inv) not applied": bk(no_inv=True),
            "tsum missing the last block": bk(tsum_drop_last=True),
        }
        if N > 1:
            wb["fix-up on row r*+1"] = bk(fix="row+1")
        if G > 1:
            wb["fix-up on head g+1"] = bk(fix="head+1")
        if c.S > 1:
            wb["reversed scan missing the last chunk"] = bk(rev_missing=True)
            wb["running-sum term dropped"] = bk(no_running=True)
        if c.S * CH > N:
            wb["rows >= N of the last chunk contributing"] = bk(pad_row0=True)
        reach = dict(dden=("dden omitted",),
                     dq=("dden omitted", "-t Ps[amq] dropped", "-t c2 x dropped", "(phi - r eps) replaced by phi", "c_scale (inv) not applied", "running-sum term dropped"),
                     dk=("dden omitted", "-t c2 x dropped", "fix-up omitted", "fix-up on row r*+1", "fix-up on head g+1", "tsum missing the last block",
                         "reversed scan missing the last chunk", "(phi - r eps) replaced by phi", "rows >= N of the last chunk contributing"),
                     dv=("reversed scan missing the last chunk", "rows >= N of the last chunk contributing"))
        self.wit_bwd = {o: {n: wb[n][o] for n in names if n in wb} for o, names in reach.items()}
        self.fwd = dict(out=f["out"], inv=f["inv"])

    def verify_forward(self, got, ratios=None, asserted=None):
        """got = (out [B, G, N, 64], inv [B, G, N], out_lp or None)"""
        out, inv, out_lp = got
        t = self.c.tag
        within(f"{t} out", out, self.fwd["out"], self.bout, self.wit_out, ratios, asserted)
        within(f"{t} inv", inv, self.fwd["inv"], self.binv, self.wit_inv, ratios, asserted)
        if out_lp is not None:
            lb.assert_rounded_once(f"{t} attn_lp", out, out_lp, asserted)

    def verify_backward(self, got, ratios=None, asserted=None):
        """got = (dden [B, G, N], dq, dk, dv [B, G, N, 64], (dq_lp, dk_lp, dv_lp) or None, tsum [B G S]) of a backward call that was given attn32 / inv32"""
        dden, dq, dk, dv, lps, tsum = got
        t = self.c.tag
        self.verify_fixup(dk, tsum, ratios, asserted)
        for name, x in (("dden", dden), ("dq", dq), ("dk", dk), ("dv", dv)):
            within(f"{t} {name}", x, self.bwd[name], self.bb[name], self.wit_bwd[name], ratios, asserted)
        if lps is not None:
            for name, x, lp in zip(("dq_lp", "dk_lp", "dv_lp"), (dq, dk, dv), lps):
                lb.assert_rounded_once(f"{t} {name}", x, lp, asserted)

    def verify_fixup(self, dk, tsum, ratios=None, asserted=None):
        """tsum_ws is an output in its own right: partial bid = (b G + g) S + chunk holds the sum of t over the key rows of that block (scan order:
        chunk = (N - 1 - n) // 64).  The row of the global maximum is then judged from the partials the fix-up launch was GIVEN: the sum over every
        row's bound that the plain dk bound has to carry there (bT) is replaced by the few roundings of adding the partials themselves."""
        c, x = self.c, self.aux
        B, G, N, S = c.B, c.G, c.N, c.S
        chunk = (N - 1 - torch.arange(N)) // CH
        onehot = (chunk[:, None] == torch.arange(S)[None, :]).double()                  # [N, S]
        ref = (x["tk"] @ onehot).reshape(-1)
        bnd = SECOND * ((x["btk"] @ onehot) + 8 * U * (x["tabs"] @ onehot)).reshape(-1) + 1e-300
        tsum = tsum.detach().cpu().double().reshape(-1)
        within(f"{c.tag} tsum", tsum, ref, bnd, {"partials in row order": ref.reshape(-1, S).flip(1).reshape(-1)}, ratios)
        b_, n_, g_, f_ = c.gmax_where
        Ps, nblk = c.Ps64, B * G * S
        row = lambda T: x["row_nofix"] - T * Ps[f_]
        T = tsum.sum()
        bnd = x["brow_nofix"] + SECOND * (((math.ceil(nblk / 64) + 6) * U * tsum.abs().sum()) * Ps[f_].abs() + 2 * U * (T * Ps[f_]).abs() + U * row(T).abs())
        wit = {"tsum missing the last block": row(T - tsum[-1]), "fix-up omitted": x["row_nofix"]}
        within(f"{c.tag} fixrow", dk.detach().cpu()[b_, g_, n_], row(T), bnd, wit, ratios, asserted)

    def shares(self):
        """per output: (share of elements whose bound exceeds the reference tensor's own maximum, median bound / max |ref|)"""
        res = {}
        for name, ref, b in (("out", self.fwd["out"], self.bout), ("inv", self.fwd["inv"], self.binv), *((n, self.bwd[n], self.bb[n]) for n in ("dden", "dq", "dk", "dv"))):
            top = float(ref.abs().max())
            res[name] = (float((b > top).double().mean()) if top > 0 else 0.0, float(b.median() / top) if top > 0 else 0.0)
        return res


# ------------------------------------------------------------------------------------------------------------------------------ model of the kernels' arithmetic
_fma, _exp32, _split = lb._fma, lb._exp32, lb._split


def _mm3(acc, A, Bm, nlo: bool = True):
    """acc [.., M, n] + A [.., M, K] Bm [.., K, n] as the tile GEMMs of split_bf16.h evaluate it: A the tile operand, Bm the register operand, both
    split; per 32 reduction steps the MFMAs A_hi B_lo, A_lo B_hi, A_hi B_hi, each summed exactly and added with one rounding (local_attn_bounds._gemm
    on the transposed product).  nlo=False: A_lo is known to be zero and its product is skipped."""
    terms = ("lh", "hl", "hh") if nlo else ("lh", "hh")
    return lb._gemm(acc.transpose(-1, -2), Bm.transpose(-1, -2), A.transpose(-1, -2), "split", terms).transpose(-1, -2)


def _dd(x, Ps_pad, terms=("lh", "hl", "hh")):
    """dd [.., rows, LDFp] in the product order of favor_prepass_kernel's products() = tile_rows_gemm = feat_slab2: P_hi x_lo, P_lo x_hi, P_hi x_hi"""
    return lb._gemm(torch.zeros(*x.shape[:-1], Ps_pad.shape[0]), x, Ps_pad.T.contiguous(), "split", terms)


def _pad_rows(Ps, m):
    LDFp = (ldf_of(m) + 63) // 64 * 64
    return torch.cat([Ps, torch.zeros(LDFp - m, DH)], 0)


def _butterfly(x, offsets):
    """__shfl_xor additions over the last axis"""
    idx = torch.arange(x.shape[-1])
    for o in offsets:
        x = x + x[..., idx ^ o]
    return x


def model_prepass(c: Case, terms=("lh", "hl", "hh")):
    """favor_prepass_kernel: (offq, offk, amq [B, G, N], gmax value, gmax flat index, ddq, ddk [B, G, N, m])"""
    Psp = _pad_rows(c.ops["Ps"], c.m)
    if c.bf16 and terms == ("lh", "hl", "hh"):
        terms = ("lh", "hh")
    out = {}
    for name in ("q", "k"):
        x = c.ops[name]
        dd = _dd(x, Psp, terms)[..., : c.m]
        xs = x.reshape(*x.shape[:-1], 2, 4, 8).permute(0, 1, 2, 4, 3, 5).reshape(*x.shape[:-1], 4, 16)     # lane g: (ks, e) in order
        ss = torch.zeros(*x.shape[:-1], 4)
        for e in range(16):
            ss = _fma(xs[..., e], xs[..., e], ss)
        ss = _butterfly(ss, (1, 2))[..., 0]
        out[name] = (dd, ss * torch.tensor(C2HALF, dtype=torch.float32))
    ddq, hq = out["q"]
    ddk, hk = out["k"]
    mx = ddq.amax(-1)
    idx = torch.arange(c.m).expand_as(ddq)
    amq = torch.where(ddq == mx.unsqueeze(-1), idx, torch.full_like(idx, 1 << 30)).amin(-1)
    flat = ddk.permute(0, 2, 1, 3).reshape(-1, c.m)
    gval = flat.max()
    r_, f_ = divmod(int((flat.reshape(-1) == gval).nonzero()[0]), c.m)
    return dict(offq=hq + mx, offk=hk, amq=amq, gmax=float(gval), gidx=r_ * c.LDF + f_, ddq=ddq, ddk=ddk)


def _scan(t, N: int, reverse: bool):
    """[B, G, N, ...] -> [B, G, S, 64, ...] in scan order (f_row), zeros where the row leaves [0, N)"""
    S = (N + CH - 1) // CH
    if reverse:
        t = t.flip(2)
    pad = torch.zeros(*t.shape[:2], S * CH - N, *t.shape[3:], dtype=t.dtype)
    return torch.cat([t, pad], 2).reshape(*t.shape[:2], S, CH, *t.shape[3:])


def _unscan(t, N: int, reverse: bool):
    t = t.reshape(*t.shape[:2], -1, *t.shape[4:])[:, :, :N]
    return t.flip(2) if reverse else t


def _feat(c: Case, dd, off, valid):
    """feat_slab: fmaf(ratio, __expf(dd - off), reps) on the live features of valid rows, 0 elsewhere; dd [.., S, 64, LDFp]"""
    F = _fma(torch.tensor(c.R, dtype=torch.float32), _exp32(dd - off.unsqueeze(-1)), torch.full_like(dd, c.REPS))
    live = (torch.arange(dd.shape[-1]) < c.m) & valid.unsqueeze(-1)
    return torch.where(live, F, torch.zeros_like(F))


def _states(Fa, b, w, seq: bool):
    """exclusive chunk prefixes (T [B, G, S, LDFp, 64], z [B, G, S, LDFp]) of U_c = Fa_c^T b_c, z_c = Fa_c^T w_c.  seq: favor_fstate_seq_body (one
    accumulator through the chunks); else favor_fstate_body per chunk and favor_fprefix_kernel's additions in chunk order."""
    S = Fa.shape[2]
    FaT = Fa.transpose(-1, -2)
    T, z = torch.zeros(*Fa.shape[:3], Fa.shape[-1], b.shape[-1]), torch.zeros(*Fa.shape[:3], Fa.shape[-1], 1)
    accT, accz = torch.zeros_like(T[:, :, 0]), torch.zeros_like(z[:, :, 0])
    if not seq:
        Uc, zc = _mm3(torch.zeros_like(T), FaT, b), _mm3(torch.zeros_like(z), FaT, w.unsqueeze(-1))
    for s in range(S):
        T[:, :, s], z[:, :, s] = accT, accz
        if seq:
            accT, accz = _mm3(accT, FaT[:, :, s], b[:, :, s]), _mm3(accz, FaT[:, :, s], w[:, :, s].unsqueeze(-1))
        else:
            accT, accz = accT + Uc[:, :, s], accz + zc[:, :, s]
    return T, z.squeeze(-1)


def _lane_feats(t):
    """[.., LDFp] -> [.., slab, f, g4, r]: feature slab * 64 + f * 16 + g4 * 4 + r"""
    return t.reshape(*t.shape[:-1], -1, 4, 4, 4)


def _scan_a(Fa, Fx, T, z, b, zmode: int):
    """favor_fout_a_body on every chunk: (y [.., S, 64 i, 64 d], inv [.., S, 64])"""
    shp = Fa.shape[:3]
    Pm, acc = torch.zeros(*shp, CH, CH), torch.zeros(*shp, DH, CH)
    den = torch.zeros(*shp, CH, 4)
    FxT = Fx.transpose(-1, -2)
    Fl, zl = _lane_feats(Fx), _lane_feats(z + torch.tensor(DEN_EPS, dtype=torch.float32))
    for sl in range(Fa.shape[-1] // 64):
        fs = slice(64 * sl, 64 * sl + 64)
        Pm = _mm3(Pm, Fa[..., fs], FxT[..., fs, :])
        acc = _mm3(acc, T[..., fs, :].transpose(-1, -2), FxT[..., fs, :])
        if zmode == 1:
            for f in range(4):
                for r in range(4):
                    den = _fma(Fl[..., sl, f, :, r], zl[..., sl, f, :, r].unsqueeze(-2), den)
    j, i = torch.arange(CH)[:, None], torch.arange(CH)[None, :]
    Pm = torch.where(j > i, torch.zeros_like(Pm), Pm)
    inv = torch.ones(*shp, CH)
    if zmode == 1:
        Pl = Pm.reshape(*shp, 4, 4, 4, CH)                        # [jf, g4, r, i]
        part = den
        for jf in range(4):
            part = part + ((Pl[..., jf, :, 0, :] + Pl[..., jf, :, 1, :]) + (Pl[..., jf, :, 2, :] + Pl[..., jf, :, 3, :])).transpose(-1, -2)
        inv = 1.0 / _butterfly(part, (1, 2))[..., 0]
    acc = _mm3(acc, b.transpose(-1, -2), Pm)
    return acc.transpose(-1, -2) * inv.unsqueeze(-1), inv


def _scan_b(c: Case, Fa, Fx, T, z, b, cop, ex_i, ex_j, zmode: int, valid, Psp):
    """favor_fout_b_body on every chunk: (dxa [.., S, 64 i, 64 d], t [.., S, 64]); cop = the c operand (times its scale), ex_i / ex_j = ex_scale at
    the row itself / at the summed rows"""
    shp = Fa.shape[:3]
    Pm = _mm3(torch.zeros(*shp, CH, CH), b, cop.transpose(-1, -2))
    e = ex_i.unsqueeze(-2) if zmode == 1 else ex_j.unsqueeze(-1)
    j, i = torch.arange(CH)[:, None], torch.arange(CH)[None, :]
    Pm = torch.where((j > i) | ~valid.unsqueeze(-1), torch.zeros_like(Pm), Pm + e)
    zf = ex_i if zmode == 1 else torch.ones_like(ex_i)
    cadd = ex_i * torch.tensor(EX_CONST, dtype=torch.float32) if zmode == 1 else torch.zeros_like(ex_i)
    dxa, tp = torch.zeros(*shp, DH, CH), torch.zeros(*shp, CH, 4)
    reps = torch.tensor(c.REPS, dtype=torch.float32)
    live = torch.arange(Fa.shape[-1]) < c.m
    for sl in range(Fa.shape[-1] // 64):
        fs = slice(64 * sl, 64 * sl + 64)
        acc = _mm3(torch.zeros(*shp, 64, CH), T[..., fs, :], cop.transpose(-1, -2))
        acc = _mm3(acc, Fa[..., fs].transpose(-1, -2), Pm)                       # [f, i]
        dphi = (acc + zf.unsqueeze(-2) * z[..., fs].unsqueeze(-1)) + cadd.unsqueeze(-2)
        ok = live[fs].view(-1, 1) & valid.unsqueeze(-2)
        vv = torch.where(ok, (Fx[..., fs].transpose(-1, -2) - reps) * dphi, torch.zeros_like(dphi))
        vl = vv.reshape(*shp, 4, 4, 4, CH)                                       # [f, g4, r, i]
        for f in range(4):
            for r in range(4):
                tp = tp + vl[..., f, :, r, :].transpose(-1, -2)
        dxa = _mm3(dxa, Psp[fs].T.contiguous().expand(*shp, DH, 64), vv, nlo=not c.bf16)
    return dxa.transpose(-1, -2), _butterfly(tp, (1, 2))[..., 0]


def _sides(c: Case, pre, reverse: bool):
    """the feature maps of keys and queries in scan order, from the model's own bit-identical dd"""
    N = c.N
    valid = _scan(torch.ones(c.B, c.G, N, dtype=torch.bool), N, reverse)
    Psp = _pad_rows(c.ops["Ps"], c.m)
    pad = Psp.shape[0] - c.m
    padf = lambda dd: torch.cat([dd, torch.zeros(*dd.shape[:-1], pad)], -1)
    offk = pre["offk"] + torch.tensor(pre["gmax"], dtype=torch.float32)
    Fk = _feat(c, _scan(padf(pre["ddk"]), N, reverse), _scan(offk, N, reverse), valid)
    Fq = _feat(c, _scan(padf(pre["ddq"]), N, reverse), _scan(pre["offq"], N, reverse), valid)
    return Fq, Fk, valid, Psp


def model_forward(c: Case, pre, seq: bool):
    """sa_favor_fused_fwd: (out [B, G, N, 64], inv [B, G, N], states)"""
    Fq, Fk, valid, _ = _sides(c, pre, False)
    vs = _scan(c.ops["v"], c.N, False)
    T, z = _states(Fk, vs, valid.float(), seq)
    y, inv = _scan_a(Fk, Fq, T, z, vs, 1)
    return _unscan(y, c.N, False), _unscan(inv, c.N, False), (T, z)


def model_backward(c: Case, pre, attn, inv, seq: bool):
    """sa_favor_fused_bwd given fp32 attn / inv: (dden [B, G, N], dq, dk, dv [B, G, N, 64], tsum [B G S])"""
    B, G, N = c.B, c.G, c.N
    o = c.ops
    # favor_fdden_v4_kernel: lane l16 holds d = 4 l16 .. + 3
    a4, b4 = o["dattn"].reshape(B, G, N, 16, 4), attn.reshape(B, G, N, 16, 4)
    sv = a4[..., 0] * b4[..., 0]
    for e in (1, 2, 3):
        sv = _fma(a4[..., e], b4[..., e], sv)
    dden = -_butterfly(sv, (8, 4, 2, 1))[..., 0] * inv
    cs = o["dattn"] * inv.unsqueeze(-1)
    Ps = c.ops["Ps"]
    c2 = torch.tensor(C2, dtype=torch.float32)
    # ---- dq: forward scan
    Fq, Fk, valid, Psp = _sides(c, pre, False)
    vs, css, dds = _scan(o["v"], N, False), _scan(cs, N, False), _scan(dden, N, False)
    T, z = _states(Fk, vs, valid.float(), seq)
    dxa, t = _scan_b(c, Fk, Fq, T, z, vs, css, dds, dds, 1, valid, Psp)
    dxa, t = _unscan(dxa, N, False), _unscan(t, N, False).unsqueeze(-1)
    dq = (dxa - t * Ps[pre["amq"]]) - (t * c2) * o["q"]
    # ---- dk, dv: reversed scans
    Fq, Fk, valid, Psp = _sides(c, pre, True)
    vs, css, dds = _scan(o["v"], N, True), _scan(cs, N, True), _scan(dden, N, True)
    T, z = _states(Fq, css, dds, seq)
    dxa, t = _scan_b(c, Fq, Fk, T, z, css, vs, dds, dds, 2, valid, Psp)
    dv, _ = _scan_a(Fq, Fk, T, z, css, 0)
    # per-block partial sums of t (wave_sum over the sixteen live lanes of a wave, the four waves), then favor_fkey_fix_kernel's fixed order
    tb = torch.where(valid, t, torch.zeros_like(t)).reshape(B, G, -1, 4, 16)
    tb = _butterfly(tb, (8, 4, 2, 1))[..., 0]
    part = ((tb[..., 0] + tb[..., 1]) + (tb[..., 2] + tb[..., 3])).reshape(-1)               # bid = (b G + g) S + chunk
    lanes = torch.zeros(64)
    for s0 in range(0, part.numel(), 64):
        seg = part[s0: s0 + 64]
        lanes[: seg.numel()] = lanes[: seg.numel()] + seg
    Tsum = _butterfly(lanes, (32, 16, 8, 4, 2, 1))[0]
    dxa, t = _unscan(dxa, N, True), _unscan(t, N, True).unsqueeze(-1)
    dk = dxa - (t * c2) * o["k"]                                                             # (ts = 0: dxa - 0 * Ps[0] is exact)
    r_, f_ = divmod(pre["gidx"], c.LDF)
    bn, g_ = divmod(r_, G)
    b_, n_ = divmod(bn, N)
    dk[b_, g_, n_] = dk[b_, g_, n_] - Tsum * Ps[f_]
    return dden, dq, dk, _unscan(dv, N, True), part


# ------------------------------------------------------------------------------------------------------------------------------ the docstring's table
OUTPUTS = ("offq", "offk", "gmax", "out", "inv", "dden", "dq", "dk", "dv", "tsum", "fixrow")


def _table():
    rows = []
    for src, name in (("model", "model (CPU)"), ("mi355x", "MI355X kernels")):
        rows.append(f"    {name:15s} " + "  ".join(f"{o} {MEASURED[src][o]:.3g}" for o in OUTPUTS))
    return "\n".join(rows)


__doc__ = __doc__ % dict(table=_table())
