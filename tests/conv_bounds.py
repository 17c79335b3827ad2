"""Element-wise fp64 error bounds for the implicit-GEMM convolution family, and the table of cases that pins every dispatchable kernel
variant to one (tests/test_conv_bounds_gpu.py runs it; tests/test_conv_coverage_cpu.py reads ``CASES`` as plain data).

The operands are drawn in fp32 and rounded to the kernel's operand type, so every product of two bf16 / f16 operands is exact in fp32 and
the only legitimate error of a correct kernel is the fp32 accumulation (and, where the output is 16-bit, its final rounding).  With ``ref``
the fp64 result on those exact values and ``A`` the same operation on the absolute values, an output element passes when

    |got - ref| <= lip * (GAMMA * A + 2 * 2^-24 * |ref| + extra) + half_ulp_out(|ref| + that slack)

``half_ulp_out`` is exact (0 for fp32 outputs), so an output truncated instead of rounded to nearest shows up as a whole-ulp error.  Each case
also checks a *witness*: the same reference with one planted defect (a dropped input channel, a dropped depth plane of the weight-gradient
reduction, a truncated output) that the kernel's output must FAIL -- proof that the bound discriminates at that shape.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

# fp32 accumulation of K exact products: the worst case grows like K * 2^-24 * A, a blocked / pairwise order like log2(K) * 2^-24 * A; the
# kernels here land at or below ~1e-6 * A.  2^-17 = 128 * 2^-24 leaves a margin of about ten over that and is still about a hundred times
# below the smallest defect the witnesses plant (a dropped channel / split / plane: 1e-4 .. 5e-3 of A).  One constant for every operand type.
GAMMA = 2.0 ** -17
U32 = 2.0 ** -24          # one fp32 rounding (bias / addend / final fp32 store)
GELU_LIP = 1.13           # max |gelu'(x)| (erf form): the bound of a GELU epilogue scales by it
SLOPE32 = float(torch.tensor(0.2, dtype=torch.float32))     # the LeakyReLU slope as the kernels get it (sa_epilogue.slope is a float)

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
_FMT = {"bf16": (7, -126), "f16": (10, -14)}     # (stored mantissa bits, minimum normal exponent)


def rounded(t: torch.Tensor, dt: str) -> torch.Tensor:
    """t rounded to the operand type `dt`, held as fp32 (the exact values the kernel sees)."""
    return t.to(DT[dt]).float()


def ulp(mag: torch.Tensor, dt: str) -> torch.Tensor:
    """one ulp of the 16-bit type `dt` at |value| = mag (float64; subnormals included)"""
    p, emin = _FMT[dt]
    mag = mag.abs()
    _, e = torch.frexp(mag)                      # mag = m * 2^e, m in [0.5, 1): exponent of the leading bit = e - 1
    e = torch.where(mag > 0, e - 1, torch.full_like(e, emin)).clamp(min=emin)
    return torch.ldexp(torch.ones_like(mag), e - p)


def half_ulp(mag: torch.Tensor, dt: str) -> torch.Tensor:
    if dt == "f32":
        return torch.zeros_like(mag)
    return 0.5 * ulp(mag, dt)


def truncated(ref: torch.Tensor, dt: str) -> torch.Tensor:
    """ref rounded toward zero to `dt` (the bf16-output witness: what a truncating store would write)"""
    u = ulp(ref.abs(), dt)
    return torch.sign(ref) * torch.floor(ref.abs() / u) * u


def bound(ref: torch.Tensor, A: torch.Tensor, out: str = "f32", lip: float = 1.0, extra=None) -> torch.Tensor:
    slack = lip * (GAMMA * A + 2 * U32 * ref.abs() + (0.0 if extra is None else extra))
    return slack + half_ulp(ref.abs() + slack, out) + 1e-300


def check(got: torch.Tensor, ref: torch.Tensor, A: torch.Tensor, out: str = "f32", lip: float = 1.0, extra=None):
    """(passes, max |got - ref| / A, index of the worst violation or None)"""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    b = bound(ref, A, out, lip, extra)
    bad = ~(err <= b)                           # (NaN fails)
    ratio = float((err / A.clamp_min(1e-30)).max())
    worst = None
    if bool(bad.any()):
        worst = tuple(int(i) for i in torch.nonzero(bad)[0])
    return not bool(bad.any()), ratio, worst


def assert_bounded(what: str, got, ref, A, witness_ref, out: str = "f32", lip: float = 1.0, extra=None, log=print):
    """got within the bound of ref, and NOT within the bound of witness_ref (the planted defect)."""
    ok, ratio, worst = check(got, ref, A, out, lip, extra)
    msg = f"{what}: max|err|/A = {ratio:.2e}"
    if worst is not None:
        g = float(got.detach().double().cpu()[worst])
        msg += f"; first violation at {worst}: got {g:.9g} ref {float(ref[worst]):.9g} A {float(A[worst]):.3g} bound {float(bound(ref[worst], A[worst], out, lip, None if extra is None else extra[worst])):.3g}"
    assert ok, msg
    wok, wratio, _ = check(got, witness_ref, A, out, lip, extra)
    log(f"  {msg} (witness: max|err|/A = {wratio:.2e}, {'PASSES -- bound does not discriminate' if wok else 'fails as it must'})")
    assert not wok, f"{what}: the planted defect is not detected at this shape (witness max|err|/A = {wratio:.2e})"


def assert_witness_fails(what: str, got, witness_ref, A, out: str = "f32", lip: float = 1.0, extra=None, log=print):
    """the witness half of assert_bounded alone: a further planted defect of an output that assert_bounded already held to its reference"""
    wok, wratio, _ = check(got, witness_ref, A, out, lip, extra)
    log(f"  {what}: witness max|err|/A = {wratio:.2e}, {'PASSES -- bound does not discriminate' if wok else 'fails as it must'}")
    assert not wok, f"{what}: the planted defect is not detected at this shape (witness max|err|/A = {wratio:.2e})"


# ------------------------------------------------------------------------------------------------------------------------------ references
def conv_ref(kind, x, w, b, s, p):
    if kind == "conv":
        return F.conv3d(x, w, b, stride=s, padding=p)
    return F.conv_transpose3d(x, w, b, stride=s, padding=p)


def dgrad_ref(kind, g, w, s, p, idims):
    if kind == "conv":
        od = g.shape[2:]
        opad = tuple(idims[d] - ((od[d] - 1) * s - 2 * p + w.shape[2 + d]) for d in range(3))
        return F.conv_transpose3d(g, w, stride=s, padding=p, output_padding=opad)
    return F.conv3d(g, w, stride=s, padding=p)


def wgrad_ref(kind, x, g, wshape, s, p):
    if kind == "conv":
        return torch.nn.grad.conv3d_weight(x, wshape, g, stride=s, padding=p)
    return torch.nn.grad.conv3d_weight(g, wshape, x, stride=s, padding=p)     # convT: x = conv3d(g, w) is its adjoint


def wgrad_last_plane(kind, x, g, wshape, s, p, k):
    """the contribution of the last depth plane of the last image of the reduction (rows = output voxels for conv, input voxels for convT)"""
    if kind == "conv":
        xp = F.pad(x[-1:], (p,) * 6)
        z0 = (g.shape[2] - 1) * s
        return torch.nn.grad.conv3d_weight(xp[:, :, z0:z0 + k], wshape, g[-1:, :, -1:], stride=s, padding=0)
    gp = F.pad(g[-1:], (p,) * 6)
    z0 = (x.shape[2] - 1) * s
    return torch.nn.grad.conv3d_weight(gp[:, :, z0:z0 + k], wshape, x[-1:, :, -1:], stride=s, padding=0)


# ------------------------------------------------------------------------------------------------------------------------------ case table
# One row per dispatchable variant: the smallest shape that selects it (N >= 2 and ragged extents wherever the path allows), the operand /
# output types, the epilogue, the debug.override switches, and the kernel-name prefixes that must appear in the kernel log (the reduce and
# column-sum kernels after a weight gradient leave no log entry: tests/test_conv_bounds_gpu.py restates which of them run from their rule).
#   op: fprop / dgrad / wgrad (ConvOp), bwd1x1 (engine.conv1x1_backward), resblock (_ResStage fused block), conv1 / convt1 (one-channel stages)
#   epi: none (no bias) | bias | relu | add_relu (addend before ReLU, 16-bit output) | mask (addend, then a sign mask of the given tensor) | gelu
#        | lrelu (forward: bias, then LeakyReLU 0.2) | mask_lrelu (data gradient: x 1 where the given tensor is > 0, x 0.2 elsewhere -- +0.0 and -0.0
#        planted in it; no addend).  Both also fail the same reference with slope 0 (ReLU / the sign mask), mask_lrelu the one that tests mask >= 0.
#   out_stride: channel stride of the forward output (the discriminator's last layer writes cout = 1 unpadded)
#   acc: weight gradients accumulate into non-zero dw / db
BF, H, F32 = "bf16", "f16", "f32"
DMA = "conv_fprop_dma_kernel"


def _c(id, op, kind, cin, cout, k, s, p, N, dims, dt, out, epi, kernels, flags=None, fwd=None, acc=False, out_stride=None):
    return dict(id=id, op=op, kind=kind, cin=cin, cout=cout, k=k, s=s, p=p, N=N, dims=dims, dt=dt, fwd=fwd or dt, out=out, epi=epi,
                kernels=list(kernels), flags=dict(flags or {}), acc=acc, out_stride=out_stride)


# 3x3x3 stride-1 grids the halo kernels take: (D, H, W) with N = 2
HALO = (64, 15, 31)         # 8 x 16 patches: 2 x 64 x 2 x 2 = 512 steps, 91 % efficient; cout 96 keeps halo256 out
HALO256 = (33, 32, 31)      # 16 x 16 patches, an odd plane count: the one-plane tiles (two-plane tiles would be more)
HALO256_P2 = (27, 40, 31)   # two-plane 2 x 8 x 16 tiles, odd plane count, ragged in H and W
WG9 = (65, 15, 31)          # halo weight gradients: 520 steps of 8 x 16, 260 per image -> the split grid crosses the image boundary
CELLS = (30, 64, 128)       # k4 s2 input: 15 x 32 x 64 cells -> 4 x 4 x 8 tiles of 4 x 8 x 8 cells per image, the last one half full in depth
CELLS_T = (15, 32, 64)      # the same cells as the input of a ConvTranspose3d k4 s2

CASES = [
    # ---- forward: im2col-order kernels
    _c("fprop_direct_f32", "fprop", "conv", 16, 24, 3, 1, 1, 2, (6, 7, 9), F32, F32, "relu", ["conv_fprop_kernel<float, 4, 1, 2, 2>"], dict(no_dma=True)),
    _c("fprop_direct_bf16", "fprop", "conv", 16, 24, 3, 1, 1, 2, (6, 7, 9), BF, BF, "add_relu", ["conv_fprop_kernel<unsigned short, 4, 1, 2, 2>"], dict(no_dma=True)),
    _c("fprop_direct_bf16_wide", "fprop", "conv", 16, 136, 3, 1, 1, 2, (5, 6, 7), BF, F32, "mask", ["conv_fprop_kernel<unsigned short, 2, 2, 4, 4>"], dict(no_dma=True)),
    _c("fprop_dma_32col_nonuniform", "fprop", "conv", 16, 24, 3, 1, 1, 2, (6, 7, 9), BF, F32, "mask", [f"{DMA}<unsigned short, 4, 1, 2, 2, false, false, 1>"]),
    _c("fprop_dma_64col_uniform", "fprop", "conv", 64, 40, 3, 1, 1, 2, (5, 6, 9), BF, BF, "add_relu", [f"{DMA}<unsigned short, 4, 1, 2, 4, true, false, 1>"]),
    _c("fprop_dma_16col_f32", "fprop", "conv", 16, 12, 4, 2, 1, 2, (8, 10, 12), F32, F32, "relu", [f"{DMA}<float, 4, 1, 2, 1, false, false, 1>"]),
    _c("fprop_dma_wide_f32", "fprop", "conv", 32, 136, 4, 2, 1, 2, (8, 10, 14), F32, F32, "bias", [f"{DMA}<float, 2, 2, 4, 4, true, false, 1>"]),
    _c("fprop_dma_wide_bf16_4w", "fprop", "conv", 32, 136, 4, 2, 1, 2, (8, 10, 14), BF, F32, "relu", [f"{DMA}<unsigned short, 2, 2, 4, 4, false, false, 1>"],
       dict(halo256_4w=True)),
    _c("fprop_dense_kg2", "fprop", "conv", 1024, 512, 1, 1, 0, 2, (1, 64, 64), BF, F32, "gelu", [f"{DMA}<unsigned short, 4, 2, 2, 4, true, false, 2>"]),
    _c("fprop_dense_kg1", "fprop", "conv", 1024, 512, 1, 1, 0, 2, (1, 64, 64), BF, BF, "bias", [f"{DMA}<unsigned short, 4, 2, 2, 4, true, false, 1>"],
       dict(no_kgroups=True)),
    _c("fprop_dense_narrow", "fprop", "conv", 256, 192, 1, 1, 0, 2, (8, 8, 15), BF, F32, "relu", [f"{DMA}<unsigned short, 4, 2, 2, 2, true, false, 1>"]),
    _c("fprop_dense_narrow_4w", "fprop", "conv", 256, 192, 1, 1, 0, 2, (8, 8, 15), BF, F32, "bias", [f"{DMA}<unsigned short, 4, 1, 2, 4, true, false, 1>"],
       dict(halo256_4w=True)),
    _c("fprop_dense_no_small_tiles", "fprop", "conv", 256, 192, 1, 1, 0, 2, (8, 8, 15), BF, F32, "relu", [f"{DMA}<unsigned short, 4, 2, 2, 4, true, false, 1>"],
       dict(no_small_tiles=True)),
    _c("fprop_dense_narrow_forced", "fprop", "conv", 1024, 512, 1, 1, 0, 2, (1, 64, 64), BF, F32, "bias", [f"{DMA}<unsigned short, 4, 2, 2, 2, true, false, 1>"],
       dict(dense_narrow=True)),
    _c("fpropT_classes", "fprop", "convT", 32, 40, 4, 2, 1, 2, (4, 5, 6), BF, F32, "relu", [f"{DMA}<unsigned short, 4, 1, 2, 4, false, false, 1>"]),
    _c("fpropT_classes_separate", "fprop", "convT", 32, 40, 4, 2, 1, 2, (4, 5, 6), BF, BF, "add_relu", [f"{DMA}<unsigned short, 4, 1, 2, 4, false, false, 1>"],
       dict(no_class_launch=True)),
    _c("fpropT_classes_im2col_128", "fprop", "convT", 64, 128, 4, 2, 1, 2, (3, 5, 6), BF, F32, "bias", [f"{DMA}<unsigned short, 4, 2, 2, 2, true, false, 1>"],
       dict(no_cells256=True)),
    _c("fprop_dma_f16", "fprop", "conv", 64, 40, 3, 1, 1, 2, (5, 6, 9), BF, H, "add_relu", [f"{DMA}<f16_t, 4, 1, 2, 4, true, false, 1>"], fwd=H),
    _c("fpropT_classes_f16", "fprop", "convT", 32, 40, 4, 2, 1, 2, (4, 5, 6), BF, F32, "relu", [f"{DMA}<f16_t, 4, 1, 2, 4, false, false, 1>"], fwd=H),
    # ---- forward: halo / cell mainloops
    _c("fprop_halo_bf16", "fprop", "conv", 64, 96, 3, 1, 1, 2, HALO, BF, BF, "add_relu", ["conv_fprop_halo_kernel<unsigned short, false>"]),
    _c("fprop_halo_f32", "fprop", "conv", 32, 96, 3, 1, 1, 2, HALO, F32, F32, "mask", ["conv_fprop_halo_kernel<float, false>"]),
    _c("fprop_halo_f16", "fprop", "conv", 64, 96, 3, 1, 1, 2, HALO, BF, H, "relu", ["conv_fprop_halo_kernel<f16_t, false>"], fwd=H),
    _c("fprop_halo256_bf16", "fprop", "conv", 64, 128, 3, 1, 1, 2, HALO256, BF, BF, "add_relu", ["conv_fprop_halo256_kernel<unsigned short, false, 8, false>"]),
    _c("fprop_halo256_p2_bf16", "fprop", "conv", 64, 128, 3, 1, 1, 2, HALO256_P2, BF, F32, "mask", ["conv_fprop_halo256_kernel<unsigned short, false, 8, true>"]),
    _c("fprop_halo256_f32", "fprop", "conv", 32, 128, 3, 1, 1, 2, HALO256, F32, F32, "relu", ["conv_fprop_halo256_kernel<float, false, 4, false>"]),
    _c("fprop_halo256_f16", "fprop", "conv", 64, 128, 3, 1, 1, 2, HALO256_P2, BF, H, "add_relu", ["conv_fprop_halo256_kernel<f16_t, false, 8, true>"], fwd=H),
    _c("fprop_cells256_conv", "fprop", "conv", 64, 128, 4, 2, 1, 2, CELLS, BF, BF, "relu", ["conv_fprop_cells256_kernel<unsigned short>"]),
    _c("fprop_cells256_convT", "fprop", "convT", 64, 128, 4, 2, 1, 2, CELLS_T, BF, F32, "bias", ["conv_fprop_cells256_kernel<unsigned short>"]),
    _c("fprop_cells256_convT_f16", "fprop", "convT", 64, 128, 4, 2, 1, 2, CELLS_T, BF, H, "relu", ["conv_fprop_cells256_kernel<f16_t>"], fwd=H),
    # ---- data gradient
    _c("dgrad_halo_taps_reversed", "dgrad", "conv", 96, 64, 3, 1, 1, 2, HALO, BF, BF, "mask", ["conv_fprop_halo_kernel<unsigned short, false>"]),
    _c("dgrad_halo256_taps_reversed", "dgrad", "conv", 128, 64, 3, 1, 1, 2, HALO256, BF, F32, "none", ["conv_fprop_halo256_kernel<unsigned short, false, 8, false>"]),
    _c("dgrad_stride2_classes", "dgrad", "conv", 32, 40, 4, 2, 1, 2, (8, 10, 12), BF, F32, "mask", [f"{DMA}<unsigned short, 4, 1, 2, 2, false, false, 1>"]),
    _c("dgrad_stride2_cells256", "dgrad", "conv", 128, 64, 4, 2, 1, 2, CELLS, BF, BF, "none", ["conv_fprop_cells256_kernel<unsigned short>"]),
    _c("dgrad_stride2_f32", "dgrad", "conv", 16, 24, 4, 2, 1, 2, (8, 10, 12), F32, F32, "none", [f"{DMA}<float, 4, 1, 2, 1, false, false, 1>"]),
    _c("dgradT", "dgrad", "convT", 32, 24, 4, 2, 1, 2, (4, 5, 6), BF, F32, "mask", [f"{DMA}<unsigned short, 4, 1, 2, 2, false, false, 1>"]),
    # ---- weight gradient (+ bias gradient)
    _c("wgrad_direct_f32", "wgrad", "conv", 16, 24, 3, 1, 1, 2, (6, 7, 9), F32, F32, "bias", ["conv_wgrad_kernel<float>", "wgrad_reduce_kernel", "colsum_kernel<float>"],
       dict(no_dma=True)),
    _c("wgrad_direct_bf16", "wgrad", "conv", 16, 24, 3, 1, 1, 2, (6, 7, 9), BF, F32, "bias",
       ["conv_wgrad_kernel<unsigned short>", "wgrad_reduce_kernel", "colsum_kernel<bf16_t>"], dict(no_dma=True), acc=True),
    _c("wgrad_dma_f32", "wgrad", "conv", 32, 40, 4, 2, 1, 2, (8, 10, 12), F32, F32, "bias", ["conv_wgrad_dma_kernel<float, false, 4>", "colsum_kernel<float>"]),
    _c("wgrad_dma_bf16_8w", "wgrad", "conv", 32, 136, 3, 1, 1, 2, (5, 6, 7), BF, F32, "bias", ["conv_wgrad_dma_kernel<unsigned short, false, 8>", "wgrad_reduce_kernel"],
       acc=True),
    _c("wgrad_dma_bf16_4w", "wgrad", "conv", 32, 136, 3, 1, 1, 2, (5, 6, 7), BF, F32, "bias", ["conv_wgrad_dma_kernel<unsigned short, false, 4>"], dict(halo256_4w=True)),
    _c("wgrad_dma_bf16_nofuseddb", "wgrad", "conv", 32, 136, 3, 1, 1, 2, (5, 6, 7), BF, F32, "bias", ["conv_wgrad_dma_kernel<unsigned short, false, 8>", "colsum_kernel<bf16_t>"],
       dict(no_fused_db=True), acc=True),
    _c("wgrad_deterministic", "wgrad", "conv", 32, 40, 4, 2, 1, 2, (8, 10, 12), BF, F32, "bias", ["conv_wgrad_dma_kernel<unsigned short, false, 8>", "colsum_det_stage1_kernel"],
       dict(deterministic=True), acc=True),
    _c("wgradT_f32_colsum_geom", "wgrad", "convT", 32, 24, 4, 2, 1, 2, (4, 5, 6), F32, F32, "bias", ["conv_wgrad_dma_kernel<float, false, 4>", "colsum_geom_kernel<float>"]),
    _c("wgradT_bf16_fused_db", "wgrad", "convT", 32, 24, 4, 2, 1, 2, (4, 5, 6), BF, F32, "bias", ["conv_wgrad_dma_kernel<unsigned short, false, 8>"], acc=True),
    _c("wgradT_bf16_colsum_geom", "wgrad", "convT", 32, 24, 4, 2, 1, 2, (4, 5, 6), BF, F32, "bias", ["colsum_geom_kernel<bf16_t>"], dict(no_fused_db=True)),
    _c("wgrad_dense_reduce_wide", "wgrad", "conv", 128, 128, 1, 1, 0, 2, (9, 40, 47), BF, F32, "bias", ["conv_wgrad_dma_kernel<unsigned short, false, 8>", "wgrad_reduce_wide_kernel"],
       dict(no_fused_db=True)),
    _c("wgrad_1x1_fused_dgrad", "bwd1x1", "conv", 128, 128, 1, 1, 0, 2, (9, 40, 47), BF, BF, "bias",
       ["conv_wgrad_dma_kernel<unsigned short, true, 4>", "wgrad_reduce_wide_kernel"], acc=True),
    _c("wgrad_halo9", "wgrad", "conv", 128, 128, 3, 1, 1, 2, WG9, BF, F32, "bias", ["conv_wgrad_halo9_kernel<8>", "wgrad_reduce_kernel"]),
    _c("wgrad_halo9_cout256_acc", "wgrad", "conv", 128, 256, 3, 1, 1, 2, WG9, BF, F32, "bias", ["conv_wgrad_halo9_kernel<8>", "wgrad_reduce_kernel"], acc=True),
    _c("wgrad_halo3", "wgrad", "conv", 128, 128, 3, 1, 1, 2, WG9, BF, F32, "bias", ["conv_wgrad_halo_kernel<4>", "wgrad_reduce_kernel"], dict(no_wgrad_halo9=True),
       acc=True),
    # ---- fused residual block (3x3x3 + ReLU + 1x1x1 + residual + ReLU in one launch)
    _c("resblock_halo256_bf16", "resblock", "conv", 128, 128, 3, 1, 1, 2, HALO256, BF, BF, "add_relu", ["conv_fprop_halo256_kernel<unsigned short, true, 8, false>"]),
    _c("resblock_halo256_p2_f16", "resblock", "conv", 128, 128, 3, 1, 1, 2, HALO256_P2, BF, H, "add_relu", ["conv_fprop_halo256_kernel<f16_t, true, 8, true>"], fwd=H),
    _c("resblock_halo_bf16", "resblock", "conv", 128, 128, 3, 1, 1, 2, HALO256, BF, BF, "add_relu", ["conv_fprop_halo_kernel<unsigned short, true>"],
       dict(no_halo256_fuse=True)),
    _c("resblock_halo_f16", "resblock", "conv", 128, 128, 3, 1, 1, 2, HALO256, BF, H, "add_relu", ["conv_fprop_halo_kernel<f16_t, true>"], dict(no_halo256_fuse=True), fwd=H),
    _c("resblock_dma_bf16", "resblock", "conv", 128, 128, 3, 1, 1, 2, (5, 9, 11), BF, BF, "add_relu", [f"{DMA}<unsigned short, 2, 2, 4, 4, true, true, 1>"]),
    _c("resblock_dma_f16", "resblock", "conv", 128, 128, 3, 1, 1, 2, (5, 9, 11), BF, H, "add_relu", [f"{DMA}<f16_t, 2, 2, 4, 4, true, true, 1>"], fwd=H),
    # ---- one-channel first layer Conv3d(1 -> C, k4 s2 p1) (+ReLU) and last layer ConvTranspose3d(128 -> 1, k4 s2 p1); forward + weight / bias gradient
    #      (+ data gradient of the last layer), through the stage objects the network uses
    _c("conv1_fused", "conv1", "conv", 1, 128, 4, 2, 1, 2, (20, 26, 34), BF, BF, "relu", ["conv1_fwd_kernel", "conv1_wgrad_kernel"]),
    _c("conv1_fused_f16", "conv1", "conv", 1, 128, 4, 2, 1, 2, (20, 26, 34), BF, H, "relu", ["conv1_fwd_f16_kernel", "conv1_wgrad_kernel"], fwd=H),
    _c("conv1_im2col_bf16", "conv1", "conv", 1, 64, 4, 2, 1, 2, (20, 26, 34), BF, BF, "relu", ["conv1_im2col_kernel", DMA, "conv_wgrad_dma_kernel"]),
    _c("conv1_im2col_f32", "conv1", "conv", 1, 64, 4, 2, 1, 2, (20, 26, 34), F32, F32, "relu", ["convt1_im2col_kernel<float>", DMA, "conv_wgrad_dma_kernel<float"]),
    _c("convt1_fused", "convt1", "convT", 128, 1, 4, 2, 1, 2, (7, 18, 17), BF, F32, "bias", ["convt1_fused_fwd_kernel", "conv1_fwd_kernel", "conv1_wgrad_kernel"]),
    _c("convt1_gather_im2col", "convt1", "convT", 128, 1, 4, 2, 1, 2, (7, 18, 17), BF, F32, "bias", ["convt1_gather_kernel", "conv1_im2col_kernel"],
       dict(no_convt1_fused_fwd=True, no_convt1_fused_bwd=True)),
    _c("convt1_im2col_direct", "convt1", "convT", 128, 1, 4, 2, 1, 2, (7, 18, 17), BF, F32, "bias", ["convt1_im2col_kernel<bf16_t>"],
       dict(no_convt1_fused_bwd=True, im2col_direct=True)),
    _c("convt1_gemm_f32", "convt1", "convT", 128, 1, 4, 2, 1, 2, (7, 18, 17), F32, F32, "bias", ["convt1_gather_kernel", "convt1_im2col_kernel<float>"]),
    _c("convt1_direct_bf16", "convt1", "convT", 128, 1, 4, 2, 1, 2, (3, 5, 7), BF, F32, "bias",
       ["convt1_fwd_kernel<bf16_t>", "convt1_dgrad_kernel<bf16_t>", "convt1_wgrad_kernel<bf16_t>"]),
    _c("convt1_direct_f32", "convt1", "convT", 128, 1, 4, 2, 1, 2, (3, 5, 7), F32, F32, "bias",
       ["convt1_fwd_kernel<float>", "convt1_dgrad_kernel<float>", "convt1_wgrad_kernel<float>"]),
    # ---- the PatchGAN discriminator's own paths (networks/discriminator/baseline.py): the LeakyReLU of the forward epilogue and of the data-gradient
    #      mask in each of the three epilogue bodies (csrc/conv_fprop_common.h: batched LDS body, row-at-a-time body, register body), and its
    #      stride-1 k4 layers -- the last one with cout = 1 (fp32 output at channel stride 1; its gradient arrives 8 wide with one valid channel)
    _c("disc_first_layer_lrelu", "fprop", "conv", 1, 64, 4, 2, 1, 2, (8, 10, 12), BF, BF, "lrelu", [f"{DMA}<unsigned short, 4, 1, 2, 4, false, false, 1>"]),
    _c("fprop_dma_16col_f32_lrelu", "fprop", "conv", 16, 12, 4, 2, 1, 2, (8, 10, 12), F32, F32, "lrelu", [f"{DMA}<float, 4, 1, 2, 1, false, false, 1>"]),
    _c("fprop_cells256_conv_lrelu", "fprop", "conv", 64, 128, 4, 2, 1, 2, CELLS, BF, BF, "lrelu", ["conv_fprop_cells256_kernel<unsigned short>"]),
    _c("dgrad_stride2_classes_mask_lrelu", "dgrad", "conv", 32, 40, 4, 2, 1, 2, (8, 10, 12), BF, F32, "mask_lrelu",
       [f"{DMA}<unsigned short, 4, 1, 2, 2, false, false, 1>"]),
    _c("dgrad_stride2_cells256_mask_lrelu", "dgrad", "conv", 128, 64, 4, 2, 1, 2, CELLS, BF, BF, "mask_lrelu", ["conv_fprop_cells256_kernel<unsigned short>"]),
    _c("disc_k4s1_fprop", "fprop", "conv", 32, 40, 4, 1, 1, 2, (6, 7, 9), BF, BF, "bias", [f"{DMA}<unsigned short, 4, 1, 2, 4, false, false, 1>"]),
    _c("disc_k4s1_dgrad", "dgrad", "conv", 32, 40, 4, 1, 1, 2, (6, 7, 9), BF, BF, "mask_lrelu", [f"{DMA}<unsigned short, 4, 1, 2, 2, false, false, 1>"]),
    _c("disc_k4s1_wgrad", "wgrad", "conv", 32, 40, 4, 1, 1, 2, (6, 7, 9), BF, F32, "bias", ["conv_wgrad_dma_kernel<unsigned short, false, 8>", "wgrad_reduce_kernel"], acc=True),
    _c("disc_last_layer_fprop", "fprop", "conv", 64, 1, 4, 1, 1, 2, (6, 7, 9), BF, F32, "bias", [f"{DMA}<unsigned short, 4, 1, 2, 1, true, false, 1>"], out_stride=1),
    _c("disc_last_layer_dgrad", "dgrad", "conv", 64, 1, 4, 1, 1, 2, (6, 7, 9), BF, BF, "mask_lrelu", [f"{DMA}<unsigned short, 4, 1, 2, 4, false, false, 1>"]),
    _c("disc_last_layer_wgrad", "wgrad", "conv", 64, 1, 4, 1, 1, 2, (6, 7, 9), BF, F32, "bias", ["conv_wgrad_dma_kernel<unsigned short, false, 8>", "wgrad_reduce_kernel"], acc=True),
]

# the split-count tunables (read once per process: csrc/elementwise.hip tunables_from_env): every setting runs the wgrad_halo9 case in a fresh child
SPLIT_ENVS = [
    ("halo_splits_1", {"SA_WGRAD_HALO_SPLITS": "1"}, "conv_wgrad_halo9_kernel<8>"),
    ("halo_splits_7", {"SA_WGRAD_HALO_SPLITS": "7"}, "conv_wgrad_halo9_kernel<8>"),        # 520 steps -> 7 splits of 75 (the last one 70)
    ("rows_64", {"SA_WGRAD_ROWS": "64", "SA_WGRAD_MIN_BLOCKS": "1"}, "conv_wgrad_halo9_kernel<8>"),
    ("halo9_16w", {"SA_PP_DBG": "16384"}, "conv_wgrad_halo9_kernel<16>"),
]
