"""GPU: the compile-time recipes of the register epilogue (csrc/conv_fprop_common.h: EpiRecipe, epi_recipe_id) in the eight-wave 3x3x3 halo kernels and the
stride-2 cell kernel.  For every recipe the same launch runs on the default path and under debug.override(generic_epilogue=True), which sends it through the
generic code; every tensor the launch writes (output, bf16 copy, hidden activation) must be EQUAL bit for bit with no voxel left at the sentinel, the library
must name the expected recipe for the launch's epilogue (sa_epilogue_recipe evaluates the kernels' own rule) and none under the flag, and the default-path
result must lie under the fp64 bound of tests/conv_bounds.py, so that correctness does not rest on the generic code alone.  One case per fall-through family
(LeakyReLU, fp32 output, alpha) checks that it still takes the generic code.

Shapes: the smallest that reach each tile kind with rows outside the volume (lanes whose row is not stored).  The halo kernels need 512 patches of 8 x 16
(halo_eligible), which (13, 54, 40) -- strip plus ordinary tiles, ragged in H, odd plane count -- and (27, 40, 31) -- the ordinary two-plane plan -- reach from
N = 2 (273 and 270 patches per volume: N = 1 runs on the im2col-order kernel); the cell kernel needs 256 tiles, which the ragged shapes of
tests/test_kernels_gpu.py::test_stride2_layers_on_the_cell_mainloop (70 tiles per volume) reach at its N = 4.  The reduction is 64 channels wide where the
layer allows (the fused block is 128 -> 128 -> 128): the epilogue does not depend on it and the fp64 reference, computed ONCE per family and shared by its
cases, stays a few seconds.  The cell references cover the last image only (every ragged tile row of a volume is in it); equality covers everything."""
import contextlib
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_bounds as cb
from test_conv_bounds_gpu import _RUN, _ncdhw
from test_strip_tiles_gpu import SENTINEL, _resblock_runner, _sentinel_outputs

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, H, F32 = cb.BF, cb.H, cb.F32
US = "unsigned short"
HALO_DIMS = [(13, 54, 40), (27, 40, 31)]
CELL_LAYERS = [("conv", (14, 112, 80)), ("convT", (8, 52, 38))]
ALPHA = 0.75


def _tag(dims):
    return "x".join(map(str, dims))


def _exact16(t):
    """values exact in bf16 AND f16, so that the bf16 and the f16 kernels of a family share operands and reference"""
    t = torch.where(t.abs() < 2.0 ** -10, torch.zeros_like(t), t)
    return cb.rounded(t, BF)


# ---------------------------------------------------------------------------------------------------------------------------- operands and references
_FAMILY = {}


def _family(kind, k, s, p, N, dims, op, ref_images):
    """operands and fp64 references of one (layer, direction), built once: op = "fprop" (64 -> 128 channels, bias) or "dgrad" (the gradient is 64 wide,
    dx 128).  References: z, A (the same on absolute values), dz (the witness: the last reduction channel alone) on the last `ref_images` images."""
    key = (kind, k, dims, op)
    if key in _FAMILY:
        return _FAMILY[key]
    from synthanatomy_amd import engine
    gen = torch.Generator().manual_seed(sum(map(ord, repr(key))))
    cin, cout = (64, 128) if op == "fprop" else (128, 64)
    wshape = (cout, cin, k, k, k) if kind == "conv" else (cin, cout, k, k, k)
    red = 64 * k ** 3
    w = _exact16(torch.randn(wshape, generator=gen) * red ** -0.5)
    b = torch.randn(cout, generator=gen) * 0.1
    probe = engine.ConvOp(kind, cin, cout, k, s, p, w, b, torch.bfloat16)
    od = probe.out_dims(dims)
    src_dims, dst_dims, dst_c = (dims, od, cout) if op == "fprop" else (od, dims, cin)
    src = _exact16(torch.randn((N, *src_dims, 64), generator=gen))
    # addend / mask at the destination; mixed signs, and the mask with exact zeros of both signs (MASK_POS keeps a value only where mask > 0)
    add = _exact16(torch.randn((N, *dst_dims, dst_c), generator=gen))
    mask = _exact16(torch.randn((N, *dst_dims, dst_c), generator=gen))
    mask.view(-1)[0::97] = 0.0
    mask.view(-1)[1::97] = -0.0
    s64, w64 = _ncdhw(src[-ref_images:]), w.double()
    if op == "fprop":
        z = cb.conv_ref(kind, s64, w64, b.double(), s, p)
        A = cb.conv_ref(kind, s64.abs(), w64.abs(), b.double().abs(), s, p)
        dz = F.conv3d(s64[:, -1:], w64[:, -1:], stride=s, padding=p) if kind == "conv" else F.conv_transpose3d(s64[:, -1:], w64[-1:], stride=s, padding=p)
    else:
        z = cb.dgrad_ref(kind, s64, w64, s, p, dims)
        A = cb.dgrad_ref(kind, s64.abs(), w64.abs(), s, p, dims)
        dz = cb.dgrad_ref(kind, s64[:, -1:], w64[-1:], s, p, dims) if kind == "conv" else cb.dgrad_ref(kind, s64[:, -1:], w64[:, -1:], s, p, dims)
    fam = dict(kind=kind, k=k, s=s, p=p, N=N, dims=dims, op=op, cin=cin, cout=cout, w=w, b=b, src=src, add=add, mask=mask, z=z, A=A, dz=dz, n_ref=ref_images,
               ops={})
    _FAMILY[key] = fam
    return fam


def _conv_op(fam, fwd):
    """the family's ConvOp for forward operands of type `fwd` (packed operands are cached on it)"""
    from synthanatomy_amd import engine
    if fwd not in fam["ops"]:
        fam["ops"][fwd] = engine.ConvOp(fam["kind"], fam["cin"], fam["cout"], fam["k"], fam["s"], fam["p"], fam["w"].to(DEV), fam["b"].to(DEV), torch.bfloat16,
                                        fwd_dtype=cb.DT[fwd])
    return fam["ops"][fwd]


# epilogue of a case: act (none / relu / lrelu), add ("first" / "last" / None), mask, alpha, output type, bf16 copy
def _epi(act="none", add=None, mask=False, alpha=False, out=BF, lp=False):
    return dict(act=act, add=add, mask=mask, alpha=alpha, out=out, lp=lp)


def _reference(fam, epi, z):
    """the generic epilogue's definition on the fp64 pre-activation: addend first, activation, alpha, addend last, mask"""
    n = fam["n_ref"]
    add64 = _ncdhw(fam["add"][-n:]) if epi["add"] else None
    x = z + add64 if epi["add"] == "first" else z
    if epi["act"] == "relu":
        x = torch.relu(x)
    elif epi["act"] == "lrelu":
        x = torch.where(x > 0, x, cb.SLOPE32 * x)
    if epi["alpha"]:
        x = x * ALPHA
    if epi["add"] == "last":
        x = x + add64
    if epi["mask"]:
        x = x * (_ncdhw(fam["mask"][-n:]) > 0)
    return x


def _launch(fam, epi, fwd):
    """-> run(): the launch through the engine, {name: tensor it wrote}"""
    from synthanatomy_amd import _ffi
    op = _conv_op(fam, fwd)
    sdt = cb.DT[fwd] if fam["op"] == "fprop" else torch.bfloat16
    src = fam["src"].to(DEV).to(sdt)
    add = fam["add"].to(DEV).to(sdt) if epi["add"] else None
    mask = fam["mask"].to(DEV).to(torch.bfloat16) if epi["mask"] else None
    alpha = torch.tensor([ALPHA], device=DEV) if epi["alpha"] else None
    act = dict(none=_ffi.ACT_NONE, relu=_ffi.ACT_RELU, lrelu=_ffi.ACT_LRELU)[epi["act"]]
    mode = _ffi.MASK_POS if epi["mask"] else _ffi.MASK_NONE

    def run():
        if fam["op"] == "dgrad":
            assert act == _ffi.ACT_NONE and epi["add"] != "first" and alpha is None
            return dict(dx=op.dgrad(src, fam["dims"], addend=add, mask=mask, mask_mode=mode, out_dtype=cb.DT[epi["out"]]))
        res = op.fprop(src, act=act, addend=add, add_before_act=epi["add"] == "first", mask=mask, mask_mode=mode, alpha=alpha, out_dtype=cb.DT[epi["out"]],
                       slope=cb.SLOPE32, want_lp=epi["lp"])
        return dict(y=res[0], y_bf16_copy=res[2]) if epi["lp"] else dict(y=res)
    return run


@contextlib.contextmanager
def _epilogues_seen(seen):
    """records every sa_epilogue the engine builds"""
    from synthanatomy_amd import engine
    make = engine.ConvOp._epilogue

    def wrapped(*a, **k):
        ep = make(*a, **k)
        seen.append(ep)
        return ep
    engine.ConvOp._epilogue = staticmethod(wrapped)
    try:
        yield
    finally:
        engine.ConvOp._epilogue = staticmethod(make)


def _both_paths(cid, run, kernel, recipe, dtype_id):
    """the launch on the default path and under generic_epilogue: kernel and recipe as expected, every written tensor equal, nothing left at the sentinel"""
    from synthanatomy_amd import _ffi, debug
    res = {}
    for generic in (False, True):
        seen = []
        with debug.override(generic_epilogue=generic), _ffi.kernel_log() as names, _sentinel_outputs(), _epilogues_seen(seen):
            res[generic] = run()
            torch.cuda.synchronize()
            got = [_ffi.lib().sa_epilogue_recipe(ctypes.byref(ep), dtype_id) for ep in seen]
        print(f"[{cid}] generic_epilogue={generic}: {', '.join(sorted(names))}; recipe {got}")
        assert kernel in names, f"{cid}: expected a launch of {kernel!r}, the log holds {sorted(names)}"
        assert got == [0 if generic else recipe], f"{cid}: the library names recipes {got} for this launch, expected {[0 if generic else recipe]}"
    assert sorted(res[False]) == sorted(res[True])
    for k, a in res[False].items():
        b = res[True][k]
        assert a.shape == b.shape and a.dtype == b.dtype
        for which, t in (("default", a), ("generic", b)):
            left = int((t == SENTINEL).sum())
            assert left == 0, f"{cid} {k}: {left} elements of the {which} run were never written"
        assert torch.equal(a, b), f"{cid} {k}: {int((a != b).sum())} of {a.numel()} elements differ, max |diff| {float((a.float() - b.float()).abs().max()):.3e}"
    return res[False]


def _bounded(cid, fam, epi, res):
    n = fam["n_ref"]
    ref, wit = _reference(fam, epi, fam["z"]), _reference(fam, epi, fam["z"] - fam["dz"])
    A = fam["A"] + (_ncdhw(fam["add"][-n:]).abs() if epi["add"] else 0.0)
    for name, t in res.items():
        copy = name == "y_bf16_copy"      # rounded from the f16 value: half an f16 ulp more (tests/test_conv_bounds_gpu.py::_resblock)
        cb.assert_bounded(f"[{cid}] {name}", _ncdhw(t[-n:]), ref, A, wit, BF if copy else epi["out"], 1.0, cb.half_ulp(ref, H) if copy else None)


# ---------------------------------------------------------------------------------------------------------------------------- the cases
def _halo_name(t, fuse, dims):
    strip = dims == (13, 54, 40)
    return f"conv_fprop_halo256_kernel<{t}, {'true' if fuse else 'false'}, 8, true{', true' if strip else ''}>"


# (id, family op, epilogue, forward operand type, recipe)
PLAIN = [("dgrad_add_mask", "dgrad", _epi(add="last", mask=True), BF, 1),
         ("dgrad_add", "dgrad", _epi(add="last"), BF, 2),
         ("dgrad_mask", "dgrad", _epi(mask=True), BF, 3),
         ("add_relu_bf16", "fprop", _epi("relu", add="first"), BF, 4),
         ("add_relu_f16_copy", "fprop", _epi("relu", add="first", out=H, lp=True), H, 5),     # (compiled into the FUSED f16 kernels only: pins the fall-through here)
         ("relu_bf16", "fprop", _epi("relu"), BF, 6),
         ("relu_f16_copy", "fprop", _epi("relu", out=H, lp=True), H, 7)]
FALL_THROUGH = [("lrelu", "fprop", _epi("lrelu"), BF, 0), ("relu_f32_out", "fprop", _epi("relu", out=F32), BF, 0),
                ("relu_alpha", "fprop", _epi("relu", alpha=True), BF, 0)]
HALO_CASES = [(f"halo256_{cid}_{_tag(d)}", d, op, epi, fwd, r) for d in HALO_DIMS for cid, op, epi, fwd, r in PLAIN] + \
             [(f"halo256_{cid}_{_tag(HALO_DIMS[0])}", HALO_DIMS[0], op, epi, fwd, r) for cid, op, epi, fwd, r in FALL_THROUGH]
# the stride-2 family on cells256: forward ReLU (bf16; f16 with the bf16 copy) and the masked data gradient, strided and transposed
CELL_CASES = [(f"cells256_{kind}_{cid}_{_tag(d)}", kind, d, op, epi, fwd, r) for kind, d in CELL_LAYERS
              for cid, op, epi, fwd, r in PLAIN if r in (3, 6, 7)]
FUSED_CASES = [cb._c(f"recipe_resblock_{'f16' if f == H else 'bf16'}_{_tag(d)}", "resblock", "conv", 128, 128, 3, 1, 1, 2, d, BF, f, "add_relu",
                     [_halo_name("f16_t" if f == H else US, True, d)], fwd=f) for d in HALO_DIMS for f in (BF, H)]


@pytest.mark.parametrize("cid,dims,op,epi,fwd,recipe", HALO_CASES, ids=[c[0] for c in HALO_CASES])
def test_halo256_recipe_equals_generic_epilogue(cid, dims, op, epi, fwd, recipe):
    from synthanatomy_amd import _ffi
    fam = _family("conv", 3, 1, 1, 2, dims, op, ref_images=2)
    res = _both_paths(cid, _launch(fam, epi, fwd), _halo_name("f16_t" if fwd == H else US, False, dims), recipe,
                      _ffi.dtype_id(cb.DT[fwd] if op == "fprop" else torch.bfloat16))
    _bounded(cid, fam, epi, res)


@pytest.mark.parametrize("cid,kind,dims,op,epi,fwd,recipe", CELL_CASES, ids=[c[0] for c in CELL_CASES])
def test_cells256_recipe_equals_generic_epilogue(cid, kind, dims, op, epi, fwd, recipe):
    from synthanatomy_amd import _ffi
    fam = _family(kind, 4, 2, 1, 4, dims, op, ref_images=1)
    res = _both_paths(cid, _launch(fam, epi, fwd), f"conv_fprop_cells256_kernel<{'f16_t' if fwd == H else US}>", recipe,
                      _ffi.dtype_id(cb.DT[fwd] if op == "fprop" else torch.bfloat16))
    _bounded(cid, fam, epi, res)


@pytest.mark.parametrize("case", FUSED_CASES, ids=[c["id"] for c in FUSED_CASES])
def test_fused_block_recipe_equals_generic_epilogue(case):
    """the fused residual block (training: hidden activation stored; f16: the bf16 copy of the output): recipes 4 (bf16) and 5 (f16).  (The strip-tile
    instance of the fused kernel is compiled without recipes -- it would spill -- so at 13 x 54 x 40 both runs execute the generic code and the case pins
    that the flag changes nothing there; the two-plane instance at 27 x 40 x 31 carries the recipe.)"""
    from synthanatomy_amd import _ffi
    f16 = case["fwd"] == H
    run = _resblock_runner(case, torch.Generator().manual_seed(sum(map(ord, case["id"]))))
    res = _both_paths(case["id"], run, case["kernels"][0], 5 if f16 else 4, _ffi.dtype_id(cb.DT[case["fwd"]]))
    assert sorted(res) == (["h_out", "y", "y_bf16_copy"] if f16 else ["h_out", "y"])
    _RUN["resblock"](case, torch.Generator().manual_seed(sum(map(ord, case["id"]))))       # the default path under the fp64 bound, with its witnesses
