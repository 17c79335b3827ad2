"""GPU: the strip tiles of the two-plane 3x3x3 halo kernel (conv_fprop_halo256_kernel<..., 8, true, true>: the last 1..8 columns of a plane on 16 (H) x 8 (W)
tiles).  On each shape the strip plan must be the one that runs (logged kernel name), every tensor a launch writes must EQUAL what the ordinary two-plane
tiles write (debug.override(no_strip_tiles=True)), bit for bit and with no voxel left unwritten, and the default-path result must lie under the fp64 bound
of tests/conv_bounds.py -- so that correctness does not rest on the older kernel alone.  Shapes that the other tests pin stay on the kernels they name."""
import contextlib

import pytest
import torch

import conv_bounds as cb
from test_conv_bounds_gpu import _RUN, _operand

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, H, F32 = cb.BF, cb.H, cb.F32
US = "unsigned short"

# N = 2, 128 output channels: the smallest grids that reach this kernel and take the strip plan.  halo256_eligible starts from halo_eligible, so a grid needs
# efficiency >= 0.8 on 8 x 16 patches and >= 512 of them besides >= 256 patches of 16 x 16 at >= 0.7: with rem <= 8 that rules out WA = 1 altogether (W <= 24 of 32
# columns), WA = 2 below W = 39, and 11 planes of 56 x 40 at N = 2 (462 patches) -- the shapes first proposed for this test, (33, 30, 24), (22, 32, 34) and
# (11, 56, 40), run on the im2col-order kernel.  These keep what each of them was to exercise.
# tiles per volume (one-plane | two-plane | strip plan): 156 | 147 | 126,  132 | 132 | 121,  156 | 147 | 126
SHAPES = [(13, 54, 40),    # WA = 2, rem = 8 (a full strip), odd plane count, ragged in H for both tile kinds (54 = 6 x 8 + 6 = 3 x 16 + 6)
          (22, 16, 82),    # WA = 5, rem = 2: a strip that is mostly empty; one band of 16 rows
          (13, 56, 40)]    # the production plane: 7 bands + 3.5 strip bands, odd plane count
SENTINEL = -24576.0        # exact in bf16, f16 and fp32; no output of these launches comes near it


def _name(t, fuse, strip):
    return f"conv_fprop_halo256_kernel<{t}, {'true' if fuse else 'false'}, 8, true{', true' if strip else ''}>"


def _tag(dims):
    return "x".join(map(str, dims))


def _cases(dims, strip=True):
    t = _tag(dims)
    return [
        cb._c(f"strip_fprop_add_relu_{t}", "fprop", "conv", 64, 128, 3, 1, 1, 2, dims, BF, BF, "add_relu", [_name(US, False, strip)]),
        cb._c(f"strip_fprop_mask_{t}", "fprop", "conv", 64, 128, 3, 1, 1, 2, dims, BF, F32, "mask", [_name(US, False, strip)]),
        cb._c(f"strip_dgrad_{t}", "dgrad", "conv", 128, 64, 3, 1, 1, 2, dims, BF, F32, "none", [_name(US, False, strip)]),
        cb._c(f"strip_resblock_bf16_{t}", "resblock", "conv", 128, 128, 3, 1, 1, 2, dims, BF, BF, "add_relu", [_name(US, True, strip)]),
        cb._c(f"strip_resblock_f16_{t}", "resblock", "conv", 128, 128, 3, 1, 1, 2, dims, BF, H, "add_relu", [_name("f16_t", True, strip)], fwd=H),
    ]


CASES = [c for dims in SHAPES for c in _cases(dims)]


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_strip_plan_within_fp64_bound(case):
    """the default path: the strip instantiation is what runs, and its result is under the fp64 bound (with the planted-defect witnesses of the helpers)"""
    gen = torch.Generator().manual_seed(sum(map(ord, case["id"])))
    _RUN[case["op"]](case, gen)


# ---------------------------------------------------------------------------------------------------------------------------- equality with ordinary tiles
@contextlib.contextmanager
def _sentinel_outputs():
    """every floating-point tensor the library wrappers allocate starts as SENTINEL, so that a voxel no tile writes shows in the result"""
    empty, empty_like = torch.empty, torch.empty_like

    def fill(t):
        return t.fill_(SENTINEL) if t.is_floating_point() else t

    torch.empty = lambda *a, **k: fill(empty(*a, **k))
    torch.empty_like = lambda *a, **k: fill(empty_like(*a, **k))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = empty, empty_like


def _fprop_runner(case, gen):
    from synthanatomy_amd import _ffi, engine
    N, dims, fdt = case["N"], case["dims"], case["fwd"]
    w = _operand((case["cout"], case["cin"], 3, 3, 3), fdt, gen, (case["cin"] * 27) ** -0.5)
    b = torch.randn(case["cout"], generator=gen) * 0.1
    x = _operand((N, *dims, case["cin"]), fdt, gen, relu=case["epi"] == "mask").to(DEV).to(cb.DT[fdt])
    add = _operand((N, *dims, case["cout"]), fdt, gen).to(DEV).to(cb.DT[fdt])
    mask = _operand((N, *dims, case["cout"]), case["dt"], gen).to(DEV).to(cb.DT[case["dt"]]) if case["epi"] == "mask" else None
    op = engine.ConvOp("conv", case["cin"], case["cout"], 3, 1, 1, w.to(DEV), b.to(DEV), cb.DT[case["dt"]], fwd_dtype=cb.DT[fdt])

    def run():
        y = op.fprop(x, act=_ffi.ACT_RELU if case["epi"] == "add_relu" else _ffi.ACT_NONE, addend=add, add_before_act=case["epi"] == "add_relu", mask=mask,
                     mask_mode=_ffi.MASK_POS if mask is not None else _ffi.MASK_NONE, out_dtype=cb.DT[case["out"]], use_bias=True)
        return dict(y=y)
    return run


def _dgrad_runner(case, gen):
    from synthanatomy_amd import engine
    N, dims, dt = case["N"], case["dims"], case["dt"]
    w = _operand((case["cout"], case["cin"], 3, 3, 3), dt, gen, (case["cin"] * 27) ** -0.5)
    b = torch.zeros(case["cout"])
    g = _operand((N, *dims, case["cout"]), dt, gen).to(DEV).to(cb.DT[dt])
    op = engine.ConvOp("conv", case["cin"], case["cout"], 3, 1, 1, w.to(DEV), b.to(DEV), cb.DT[dt])
    return lambda: dict(dx=op.dgrad(g, dims, out_dtype=cb.DT[case["out"]]))


def _resblock_runner(case, gen):
    from synthanatomy_amd.networks.vqvae.baseline import ResidualLayer, _Act, _ResStage
    fdt, N, dims = case["fwd"], case["N"], case["dims"]
    mod = ResidualLayer(128, 128, 0.0)
    with torch.no_grad():
        mod[0].weight.copy_(_operand((128, 128, 3, 3, 3), fdt, gen, (128 * 27) ** -0.5)), mod[0].bias.copy_(torch.randn(128, generator=gen) * 0.1)
        mod[3].weight.copy_(_operand((128, 128, 1, 1, 1), fdt, gen, 128 ** -0.5)), mod[3].bias.copy_(torch.randn(128, generator=gen) * 0.1)
    st = _ResStage(mod.to(DEV).eval(), in_act=True, dtype=torch.bfloat16, fwd_dtype=cb.DT[fdt] if fdt != "bf16" else None)
    x = _operand((N, *dims, 128), fdt, gen, relu=True).to(DEV).to(cb.DT[fdt])

    def run():
        tape = []
        y = st.fwd(x, tape)
        out = dict(h_out=tape[0][1])
        if isinstance(y, _Act):
            assert fdt == "f16" and y.s is not None
            out.update(y=y.f, y_bf16_copy=y.s)
        else:
            out.update(y=y)
        return out
    return run


_RUNNER = dict(fprop=_fprop_runner, dgrad=_dgrad_runner, resblock=_resblock_runner)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_strip_tiles_equal_ordinary_tiles(case):
    """the same launch on strip tiles and, under no_strip_tiles, on ordinary two-plane tiles: every written tensor equal, nothing left at the sentinel"""
    from synthanatomy_amd import _ffi, debug
    run = _RUNNER[case["op"]](case, torch.Generator().manual_seed(sum(map(ord, case["id"]))))
    res = {}
    for strip in (True, False):
        with debug.override(no_strip_tiles=not strip), _ffi.kernel_log() as names, _sentinel_outputs():
            res[strip] = run()
            torch.cuda.synchronize()
        fuse = case["op"] == "resblock"
        want = _name("f16_t" if case["fwd"] == "f16" else US, fuse, strip)
        got = sorted(names)
        print(f"[{case['id']}] no_strip_tiles={not strip}: {', '.join(got)}")
        assert want in got, f"{case['id']}: expected a launch of {want!r}, the log holds {got}"
    assert sorted(res[True]) == sorted(res[False])
    for k, a in res[True].items():
        b = res[False][k]
        assert a.shape == b.shape and a.dtype == b.dtype
        for which, t in (("strip", a), ("ordinary", b)):
            left = int((t == SENTINEL).sum())
            assert left == 0, f"{case['id']} {k}: {left} elements of the {which}-tile run were never written"
        assert torch.equal(a, b), f"{case['id']} {k}: {int((a != b).sum())} of {a.numel()} elements differ, max |diff| {float((a.float() - b.float()).abs().max()):.3e}"


# ---------------------------------------------------------------------------------------------------------------------------- shapes other tests pin
@pytest.mark.parametrize("dims,strip_free_name", [((27, 40, 31), _name(US, False, False)),      # tests/conv_bounds.py HALO256_P2: rem = 15
                                                  ((35, 40, 44), _name(US, False, False))],     # tests/test_vqvae_gpu.py: rem = 12
                         ids=["27x40x31", "35x40x44"])
def test_pinned_shapes_keep_their_kernel(dims, strip_free_name):
    from synthanatomy_amd import _ffi
    case = cb._c("pinned_" + _tag(dims), "fprop", "conv", 64, 128, 3, 1, 1, 2, dims, BF, BF, "add_relu", [strip_free_name])
    run = _fprop_runner(case, torch.Generator().manual_seed(11))
    with _ffi.kernel_log() as names:
        run()
        torch.cuda.synchronize()
    assert _ffi.lib().sa_last_conv_kernel().decode() == strip_free_name, sorted(names)
    assert not any(n.endswith("true, true>") for n in names), sorted(names)
