"""GPU: ``sa_conv_fprop`` at the twelve distinct 2-D geometries the Fire modules of the LPIPS-squeeze stack add: the eight 1 x 1
squeeze launches 64 -> 16, 128 -> 16, 128 -> 32, 256 -> 32, 256 -> 48, 384 -> 48, 384 -> 64, 512 -> 64 and the four merged 3 x 3 expand launches 16 -> 128,
32 -> 256, 48 -> 384, 64 -> 512 (the 1 x 1 half on the centre tap, zeros around it: losses.lpips_squeeze.merged_expand) -- forward with bias + ReLU and the
data gradient with addend + SA_MASK_POS, in both compute dtypes, under the element-wise fp64 bound of tests/conv_bounds.py with its dropped-channel witness.
Modelled on tests/test_lpips_conv2d_gpu.py; the narrow sides (16, 32, 48 channels) are the first such widths any 2-D caller hands the dispatcher."""
import pytest
import torch
import torch.nn.functional as F

import conv_bounds as cb

pytestmark = pytest.mark.gpu

DEV = "cuda"
S, HW = 3, (7, 8)
LAYERS = {"sq_64_16": (64, 16, 1), "sq_128_16": (128, 16, 1), "sq_128_32": (128, 32, 1), "sq_256_32": (256, 32, 1), "sq_256_48": (256, 48, 1),
          "sq_384_48": (384, 48, 1), "sq_384_64": (384, 64, 1), "sq_512_64": (512, 64, 1),
          "ex_16_128": (16, 128, 3), "ex_32_256": (32, 256, 3), "ex_48_384": (48, 384, 3), "ex_64_512": (64, 512, 3)}


def _nchw(t):       # channels-last [N, h, w, C] -> [N, C, h, w], float64 on the CPU
    return t.detach().double().cpu().permute(0, 3, 1, 2)


def _operands(layer, dt):
    from synthanatomy_amd.losses.lpips_squeeze import merged_expand
    ci, co, k = LAYERS[layer]
    gen = torch.Generator().manual_seed(sum(map(ord, layer + dt)))
    if k == 1:
        w = torch.randn(co, ci, 1, 1, generator=gen) * ci ** -0.5
        b = torch.randn(co, generator=gen) * 0.1
    else:           # the merged expand: Cout / 2 rows of a 1 x 1 on the centre tap, Cout / 2 rows of a 3 x 3
        w, b = merged_expand(torch.randn(co // 2, ci, 1, 1, generator=gen) * ci ** -0.5, torch.randn(co // 2, generator=gen) * 0.1,
                             torch.randn(co // 2, ci, 3, 3, generator=gen) * (ci * 9) ** -0.5, torch.randn(co // 2, generator=gen) * 0.1)
    return ci, co, k, gen, cb.rounded(w, dt), b


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("layer", list(LAYERS))
def test_conv2d_forward_within_fp64_bound(layer, dt):
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.losses.lpips import Conv2dOp
    ci, co, k, gen, w, b = _operands(layer, dt)
    x = cb.rounded(torch.randn(S, *HW, ci, generator=gen), dt)
    op = Conv2dOp(w.to(DEV), b.to(DEV), cb.DT[dt])
    with _ffi.kernel_log() as names:
        y = op.fprop(x.to(DEV).to(cb.DT[dt]))
        torch.cuda.synchronize()
    print(f"[{layer} {dt} fprop] kernels: {', '.join(sorted(names))}")
    x64, w64, b64 = _nchw(x), w.double(), b.double()
    z = F.conv2d(x64, w64, b64, padding=k // 2)
    A = F.conv2d(x64.abs(), w64.abs(), b64.abs(), padding=k // 2)
    wit = torch.relu(z - F.conv2d(x64[:, -1:], w64[:, -1:], padding=k // 2))      # witness: the last input channel dropped
    cb.assert_bounded(f"[{layer} {dt}] y", _nchw(y), torch.relu(z), A, wit, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("layer", list(LAYERS))
def test_conv2d_data_gradient_with_mask_within_fp64_bound(layer, dt):
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.losses.lpips import Conv2dOp
    ci, co, k, gen, w, b = _operands(layer, dt)
    g = cb.rounded(torch.randn(S, *HW, co, generator=gen), dt)
    add = cb.rounded(torch.randn(S, *HW, ci, generator=gen), dt)
    mask = cb.rounded(torch.relu(torch.randn(S, *HW, ci, generator=gen)), dt)      # a forward output: zeros where the ReLU was off
    op = Conv2dOp(w.to(DEV), b.to(DEV), cb.DT[dt])
    with _ffi.kernel_log() as names:
        dx = op.dgrad(g.to(DEV).to(cb.DT[dt]), addend=add.to(DEV).to(cb.DT[dt]), mask=mask.to(DEV).to(cb.DT[dt]))
        torch.cuda.synchronize()
    print(f"[{layer} {dt} dgrad] kernels: {', '.join(sorted(names))}")
    g64, w64, m = _nchw(g), w.double(), (_nchw(mask) > 0).double()
    z = F.conv_transpose2d(g64, w64, padding=k // 2) + _nchw(add)
    A = F.conv_transpose2d(g64.abs(), w64.abs(), padding=k // 2) + _nchw(add).abs()
    wit = (z - F.conv_transpose2d(g64[:, -1:], w64[-1:], padding=k // 2)) * m       # witness: the last gradient channel dropped
    # (A is not masked: a masked-out element must be an exact zero, which err <= bound(0, A) cannot tell from a small value -- checked apart)
    cb.assert_bounded(f"[{layer} {dt}] dx", _nchw(dx), z * m, A, wit, dt)
    assert bool((_nchw(dx)[m == 0] == 0).all()), "masked-out elements of the data gradient must be exact zeros"
