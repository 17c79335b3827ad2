"""GPU: ``sa_volume_egress`` (csrc/egress.hip) against ``egress_ref`` / ``autoscale_ref`` of tests/nifti_out_ref.py, and tied to
``sa_volume_ingest`` by a round trip through the writer and the reader of utils/nifti.py.

Every comparison is equality of bytes: float32 is a copy, and an integer code is two rounded fp64 operations, a round-half-even and a clamp on both
sides.  The one tolerance of this file is the integer round trip's (see that test).  Shapes are the ingest tests': (5, 7, 11) and (1, 1, 1) sit inside one
64 x 64 tile, (33, 65, 31) and (64, 1, 33) give every axis a value from {1, 31, 33, 64, 65}: a full tile, partial tiles and a second tile along every axis
that can be tiled, and groups of 4 / 8 / 16 output voxels that are whole, cut by the row's end, and misaligned for a 16-byte store."""
import ctypes

import numpy as np
import pytest
import torch

from nifti_out_ref import SIGNED_PERMS, autoscale_ref, egress_ref, finite_min_max, ulp32
from nifti_ref import signed_perm_affine

pytestmark = pytest.mark.gpu

ORIENTATIONS = [((1, 2, 0), (1, -1, 1)), ((0, 1, 2), (1, 1, 1)), ((2, 1, 0), (-1, -1, -1))]      # perm[2] == 0; perm[2] != 0; every axis reversed
DEV = "cuda:0"
CODE = {"float32": 16, "int16": 4, "uint8": 2}


def _x(file_dims, perm, seed=0, scale=100.0):
    """A canonical fp32 volume whose file has ``file_dims`` under ``perm``."""
    ext = [file_dims[perm[a]] for a in range(3)]
    return (np.random.default_rng(seed).standard_normal(ext) * scale).astype(np.float32)


def _egress(x, perm, sign, dtype="float32", x_dtype=torch.float32, **kw):
    from synthanatomy_amd.utils.vqvae import hip_egress
    out = hip_egress(torch.from_numpy(x).to(DEV).to(x_dtype), perm, sign, dtype, **kw)
    torch.cuda.synchronize()
    return out


def _words(ws):
    w = ws.cpu().numpy()
    mn, mx = np.array([w[2] & 0xFFFFFFFF, (w[2] >> 32) & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
    return w, mn, mx


def test_all_48_signed_permutations_float32():
    x = _x((5, 7, 11), (0, 1, 2))
    for perm, sign in SIGNED_PERMS:
        raw = _egress(x, perm, sign)
        assert raw.dtype == torch.uint8 and raw.numel() == x.size * 4
        assert raw.cpu().numpy().tobytes() == egress_ref(x, perm, sign)[0], (perm, sign)


@pytest.mark.parametrize("dims", [(33, 65, 31), (64, 1, 33), (1, 1, 1)])
@pytest.mark.parametrize("dtype", ["float32", "int16", "uint8"])
@pytest.mark.parametrize("x_dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_tile_edges(dims, dtype, x_dtype):
    for perm, sign in ORIENTATIONS:
        x = _x(dims, perm, seed=3)
        x = torch.from_numpy(x).to(x_dtype).float().numpy()      # what a bf16 input holds, widened exactly
        if dtype == "float32":
            raw = _egress(x, perm, sign, dtype, x_dtype)
            want = egress_ref(x, perm, sign)[0]
        else:
            slope, inter = (0.01, 5.0) if dtype == "int16" else (2.5, -300.0)
            raw, pair = _egress(x, perm, sign, dtype, x_dtype, autoscale=False, slope=slope, inter=inter)
            assert pair.tolist() == [slope, inter]
            want = egress_ref(x, perm, sign, dtype, slope, inter)[0]
        assert raw.cpu().numpy().tobytes() == want, (dims, dtype, perm, sign)


def test_integer_conversion_rounds_half_to_even_and_clamps():
    slope, inter = 0.5, -3.25
    for dtype, (lo, hi) in (("int16", (-32768, 32767)), ("uint8", (0, 255))):
        codes = np.concatenate([np.arange(lo, lo + 40), np.arange(hi - 40, hi + 1), np.arange(-20, 60)]).astype(np.float64)
        ties = (np.concatenate([codes + 0.5, codes - 0.5, codes]) * slope + inter).astype(np.float32)      # exact in fp32: multiples of 1 / 4 below 2^15
        beyond = np.array([lo * slope + inter - 1000, hi * slope + inter + 1000, -1e30, 1e30, lo * slope + inter - 0.25, hi * slope + inter + 0.25], dtype=np.float32)
        v = np.concatenate([ties, beyond])
        x = np.resize(v, (5, 7, 17)).astype(np.float32)
        assert x.size >= v.size
        for perm, sign in ORIENTATIONS:
            raw, _ = _egress(x, perm, sign, dtype, autoscale=False, slope=slope, inter=inter)
            want = egress_ref(x, perm, sign, dtype, slope, inter)[0]
            assert raw.cpu().numpy().tobytes() == want, (dtype, perm, sign)
        got = np.frombuffer(egress_ref(x, (0, 1, 2), (1, 1, 1), dtype, slope, inter)[0], dtype=np.dtype(dtype))
        assert got.min() == lo and got.max() == hi      # (the reference itself reaches both clamps)


@pytest.mark.parametrize("dtype", ["int16", "uint8"])
def test_autoscale_pair_and_codes(dtype):
    for (perm, sign), dims in zip(ORIENTATIONS, [(33, 65, 31), (64, 1, 33), (5, 7, 11)]):
        x = _x(dims, perm, seed=5, scale=37.0) + np.float32(11.5)
        raw, pair, ws = _egress(x, perm, sign, dtype, return_workspace=True)
        w, mn, mx = _words(ws)
        assert (mn, mx) == finite_min_max(x) and w[3] == 0
        slope, inter = autoscale_ref(mn, mx, dtype)
        assert pair.tolist() == [slope, inter]
        assert np.float32(slope) == slope and np.float32(inter) == inter      # what a header can hold
        assert raw.cpu().numpy().tobytes() == egress_ref(x, perm, sign, dtype, slope, inter)[0]
        codes = np.frombuffer(raw.cpu().numpy().tobytes(), dtype=np.dtype(dtype))
        info = np.iinfo(np.dtype(dtype))
        assert codes.min() == info.min and codes.max() >= info.max - 1      # the full code range is used
    x = np.full((5, 7, 11), 3.75, dtype=np.float32)                         # a constant volume: slope 1, inter = the value, every code 0
    raw, pair = _egress(x, (2, 0, 1), (1, -1, 1), dtype)
    assert pair.tolist() == [1.0, 3.75] == list(autoscale_ref(3.75, 3.75, dtype)) and not raw.any()


def _round_trip(x, perm, sign, dtype, tmp_path, ext):
    from synthanatomy_amd.utils.nifti import header_orientation, output_header, read_nifti, write_nifti
    from synthanatomy_amd.utils.vqvae import hip_egress, hip_ingest
    out = hip_egress(torch.from_numpy(x).to(DEV), perm, sign, dtype)
    raw, pair = (out, None) if dtype == "float32" else out
    slope, inter = (1.0, 0.0) if pair is None else pair.tolist()
    dims = [0, 0, 0]
    for a in range(3):
        dims[perm[a]] = x.shape[a]
    path = str(tmp_path / f"rt_{dtype}{ext}")
    write_nifti(path, output_header(dims, CODE[dtype], signed_perm_affine(perm, sign), slope, inter), raw.cpu().numpy())
    header, block = read_nifti(path)
    assert header.dims == tuple(dims) and header.datatype == CODE[dtype] and header_orientation(header, True) == (list(perm), list(sign))
    back = hip_ingest(header, block, None, normalize=False, canonical=True, device=DEV)
    assert back.shape == (1, *x.shape)
    return back[0].cpu().numpy(), slope, inter


def test_round_trip_through_the_file_and_the_ingest_kernel_is_exact_for_float32(tmp_path):
    for perm, sign in SIGNED_PERMS:
        xp = _x((5, 7, 11), perm, seed=6)
        for ext in (".nii", ".nii.gz"):
            back, _, _ = _round_trip(xp, perm, sign, "float32", tmp_path, ext)
            assert back.tobytes() == xp.tobytes(), (perm, sign, ext)
    for ext in (".nii", ".nii.gz"):      # and both containers on a tiled shape
        xp = _x((33, 65, 31), (1, 2, 0), seed=7)
        assert _round_trip(xp, (1, 2, 0), (1, -1, 1), "float32", tmp_path, ext)[0].tobytes() == xp.tobytes()


@pytest.mark.parametrize("dtype", ["int16", "uint8"])
def test_round_trip_of_integer_dtypes_is_within_half_a_step(dtype, tmp_path):
    """|ingest(egress(x)) - x| <= 0.5 * slope + ulp32(|inter|) + ulp32(max |x|): the quantisation half-step (auto-scaling covers [min, max], so no
    voxel is clamped by more than the intercept's rounding), plus the float32 rounding of the stored intercept (at most half an ulp of inter, bounded by
    one), plus the reader's final rounding of code * slope + inter to fp32 (at most half an ulp of a value next to max |x|, bounded by one ulp of it)."""
    for k, (perm, sign) in enumerate(SIGNED_PERMS):
        x = _x((5, 7, 11), perm, seed=8, scale=37.0) + np.float32(11.5)
        back, slope, inter = _round_trip(x, perm, sign, dtype, tmp_path, ".nii.gz" if k % 2 else ".nii")
        bound = 0.5 * slope + ulp32(inter) + ulp32(np.abs(x).max())
        err = float(np.abs(back.astype(np.float64) - x.astype(np.float64)).max())
        if k == 0:
            print(f"{dtype} round trip: max error {err:.6g}, bound {bound:.6g}, slope {slope:.6g}")
        assert err <= bound, (perm, sign, err, bound)


@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_non_finite_inputs_are_stored_as_zero_and_counted(dtype):
    for perm, sign in ORIENTATIONS:
        x = _x((33, 65, 31), perm, seed=9)
        x[0, 0, 0], x[-1, -1, -1], x[3, 17, 9], x[2, 2, 2] = np.nan, np.inf, -np.inf, np.nan
        if dtype == "float32":
            raw, ws = _egress(x, perm, sign, dtype, return_workspace=True)
            pair = (1.0, 0.0)
        else:
            raw, pair, ws = _egress(x, perm, sign, dtype, return_workspace=True)
            pair = tuple(pair.tolist())
        w, mn, mx = _words(ws)
        assert w[3] == 4 and (mn, mx) == finite_min_max(x) and np.isfinite(mn) and np.isfinite(mx)
        if dtype != "float32":
            assert pair == autoscale_ref(mn, mx, dtype)
        want, bad = egress_ref(x, perm, sign, dtype, *pair)
        assert bad == 4 and raw.cpu().numpy().tobytes() == want
    x = np.full((5, 7, 11), np.nan, dtype=np.float32)      # no finite voxel at all: min = max = 0, slope 1, inter 0, zeros
    raw, pair, ws = _egress(x, (0, 1, 2), (1, 1, 1), "int16", return_workspace=True)
    assert not raw.any() and pair.tolist() == [1.0, 0.0] and ws.cpu().tolist()[2:4] == [0, 385]


def test_workspace_is_left_ready_for_the_next_call():
    from synthanatomy_amd.utils import vqvae as uv
    a = (_x((33, 65, 31), (1, 2, 0), seed=10), (1, 2, 0), (1, -1, 1), "int16")
    b = (_x((64, 1, 33), (2, 1, 0), seed=11) + np.float32(1000), (2, 1, 0), (-1, -1, -1), "uint8")
    c = (_x((5, 7, 11), (0, 1, 2), seed=12), (0, 1, 2), (1, 1, 1), "float32")
    fresh = []
    for x, perm, sign, dtype in (a, b, c):
        uv._EGRESS_WS.clear()      # a fresh, zeroed workspace
        out = _egress(x, perm, sign, dtype, return_workspace=True)
        fresh.append([t.cpu().numpy().copy() for t in out])
    uv._EGRESS_WS.clear()
    for k in (0, 1, 2, 0):      # back to back on one workspace, nothing cleared in between
        x, perm, sign, dtype = (a, b, c)[k]
        out = _egress(x, perm, sign, dtype, return_workspace=True)
        for got, want in zip(out, fresh[k]):
            assert np.array_equal(got.cpu().numpy(), want)
        words = out[-1].cpu().tolist()
        assert words[0] == words[1] == words[4] == words[5] == 0


def test_hip_egress_refuses_what_it_does_not_take():
    from synthanatomy_amd.utils.vqvae import hip_egress
    x = torch.zeros(5, 7, 11, device=DEV)
    for bad in (x[None, None], x[:, :, ::2], x.double(), x.half(), torch.zeros(2, 5, 7, 11, device=DEV), x.cpu()):
        with pytest.raises(ValueError, match="hip_egress"):
            hip_egress(bad, (0, 1, 2), (1, 1, 1))
    for kw in (dict(perm=(0, 1, 1)), dict(sign=(1, 0, 1)), dict(dtype="int32")):
        with pytest.raises(ValueError, match="hip_egress"):
            hip_egress(x, **{"perm": (0, 1, 2), "sign": (1, 1, 1), **kw})
    assert hip_egress(x[None], (0, 1, 2), (1, 1, 1)).numel() == 1540 and hip_egress(x.bfloat16(), (0, 1, 2), (1, 1, 1), "uint8")[0].numel() == 385


def test_argument_checks_return_their_code_and_launch_nothing():
    from synthanatomy_amd import _ffi
    lib = _ffi.lib()
    x = torch.zeros(5 * 7 * 11, device=DEV)
    raw = torch.full((5 * 7 * 11 * 4 + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(8, dtype=torch.int64, device=DEV)
    assert lib.sa_volume_egress_workspace_bytes() == 64

    def call(x_ptr=None, raw_ptr=None, nbytes=1540, ws_ptr=None, null_params=False, **fields):
        P = _ffi.EgressParams(x_dtype=0, dtype=16, flags=0, slope=1.0, inter=0.0)
        P.ext[:], P.perm[:], P.sign[:] = (5, 7, 11), (0, 1, 2), (1, 1, 1)
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(P, k)[:] = v
            else:
                setattr(P, k, v)
        return lib.sa_volume_egress(ctypes.c_void_p(x.data_ptr() if x_ptr is None else x_ptr), ctypes.c_void_p(raw.data_ptr() if raw_ptr is None else raw_ptr),
                                    nbytes, None if null_params else ctypes.byref(P), ctypes.c_void_p(ws.data_ptr() if ws_ptr is None else ws_ptr), _ffi.stream())

    E, U = _ffi.SA_EINVAL, _ffi.SA_EUNSUPPORTED
    assert call(x_ptr=0) == E and call(raw_ptr=0) == E and call(ws_ptr=0) == E and call(null_params=True) == E      # null operands
    assert call(raw_ptr=raw.data_ptr() + 4) == E                                                                     # raw not 16-byte aligned
    assert call(ext=(5, 0, 11)) == E and call(ext=(5, 7, -1)) == E                                                   # an extent < 1
    assert call(perm=(0, 1, 1)) == E and call(perm=(0, 1, 3)) == E and call(perm=(-1, 1, 2)) == E                    # no permutation
    assert call(nbytes=1539) == E and call(dtype=4, nbytes=769) == E                                                 # raw_bytes smaller than the dims need
    for pair in (dict(slope=0.0), dict(slope=float("nan")), dict(slope=float("inf")), dict(inter=float("nan")), dict(inter=float("-inf"))):
        assert call(dtype=4, **pair) == E and call(dtype=2, **pair) == E                                           # a zero or non-finite given pair
        assert call(dtype=4, flags=1, **pair) == 0                                                                   # (ignored with AUTOSCALE; zeros in, zeros out)
    torch.cuda.synchronize()
    assert not raw[:770].any() and bool((raw[770:] == 0xA5).all())
    raw.fill_(0xA5)
    ws.zero_()
    for code in (0, 1, 8, 32, 64, 256, 512, 768, 3):
        assert call(dtype=code) == U                                                                                 # another dtype
    assert call(x_dtype=2) == U and call(x_dtype=-1) == U                                                            # another x_dtype
    assert call(ext=(2048, 2048, 512), nbytes=1 << 40) == U                                                          # 2^31 voxels
    assert call(ext=(1 << 30, 2, 1), nbytes=1 << 40) == U and call(ext=(46341, 46341, 1), nbytes=1 << 40) == U
    torch.cuda.synchronize()
    assert bool((raw == 0xA5).all()) and not ws.any()                                                                # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert not raw[:1540].any() and bool((raw[1540:] == 0xA5).all())                                                 # zeros in, zeros out, nothing behind the block
