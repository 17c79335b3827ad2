"""GPU: ``sa_volume_ingest`` (csrc/ingest.hip) against ``ingest_ref`` of tests/nifti_ref.py.

Without normalisation the bound is equality: an integer voxel converts exactly or with one correctly rounded conversion on both sides, and the scaling is
two rounded fp64 operations and one rounding to fp32 on both sides.  With normalisation both sides run the same three IEEE fp32 operations (a subtraction,
an addition and a correctly rounded division; the build has no fast-math), so the expected difference is 0; the test allows 1 ulp of the expected value
and prints the measured maximum (measured on MI355X: 0 ulp, 0.0 absolute, in every case).  Shapes: (5, 7, 11) and (1, 1, 1) sit inside
one 64 x 64 tile, (33, 65, 31) and (64, 1, 33) give every axis a value from {1, 31, 33, 64, 65}: a full tile, partial tiles and a second tile along
every axis that can be tiled."""
import ctypes

import numpy as np
import pytest
import torch

from nifti_ref import CODES, SIGNED_PERMS, header_bytes, ingest_ref, signed_perm_affine

pytestmark = pytest.mark.gpu

ORIENTATIONS = [((0, 1, 2), (1, 1, 1)), ((2, 1, 0), (-1, -1, -1)), ((1, 2, 0), (1, -1, 1))]
DEV = "cuda:0"


def _data(dtype, dims, seed=0):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (rng.standard_normal(dims) * 100).astype(dt)
    info = np.iinfo(dt)
    v = rng.integers(info.min, info.max, size=dims, endpoint=True, dtype=dt)
    v.flat[0], v.flat[-1] = info.min, info.max
    return v


def _case(data, perm=(0, 1, 2), sign=(1, 1, 1), big_endian=False, slope=0.0, inter=0.0):
    """(header, voxel block) of ``data`` [n0, n1, n2] stored with the orientation (perm, sign)."""
    from synthanatomy_amd.utils.nifti import parse_header
    header = parse_header(header_bytes(data.shape, CODES[data.dtype.name], big_endian=big_endian, slope=slope, inter=inter,
                                       sform=signed_perm_affine(perm, sign)))
    raw = np.asfortranarray(data).astype(data.dtype.newbyteorder(">" if big_endian else "<")).tobytes(order="F")
    return header, raw


def _check_equal(header, raw, window=None, canonical=True):
    from synthanatomy_amd.utils.vqvae import hip_ingest
    got = hip_ingest(header, raw, window, normalize=False, canonical=canonical, device=DEV)
    want, _ = ingest_ref(header, raw, window, normalize=False, canonical=canonical)
    assert got.shape == (1, *want.shape) and got.dtype == torch.float32
    assert torch.equal(got[0].cpu(), torch.from_numpy(want)), (header.dims, header.datatype, window)
    return got


def test_all_48_signed_permutations_int16():
    from synthanatomy_amd.utils.nifti import header_orientation
    data = _data("int16", (5, 7, 11))
    for perm, sign in SIGNED_PERMS:
        header, raw = _case(data, perm, sign)
        assert header_orientation(header, True) == (list(perm), list(sign))
        got = _check_equal(header, raw)
        assert tuple(got.shape[1:]) == tuple(data.shape[k] for k in perm)
    _check_equal(*_case(data, (2, 0, 1), (-1, 1, -1)), canonical=False)      # the stored order


@pytest.mark.parametrize("dtype", sorted(CODES))
def test_every_dtype_on_three_orientations(dtype):
    data = _data(dtype, (5, 7, 11), seed=1)
    for perm, sign in ORIENTATIONS:
        _check_equal(*_case(data, perm, sign))


@pytest.mark.parametrize("dtype", ["int16", "float32", "float64"])
def test_byte_swapped(dtype):
    data = _data(dtype, (5, 7, 11), seed=2)
    for perm, sign in ORIENTATIONS:
        header, raw = _case(data, perm, sign, big_endian=True)
        assert header.byteswap
        _check_equal(header, raw)


@pytest.mark.parametrize("dims", [(33, 65, 31), (64, 1, 33), (1, 1, 1)])
@pytest.mark.parametrize("dtype", ["uint8", "int16", "float32", "float64"])      # 16, 8, 4 and 2 elements per 16-byte chunk
def test_tile_edges(dims, dtype):
    data = _data(dtype, dims, seed=3)
    for perm, sign in ORIENTATIONS + [((0, 2, 1), (1, 1, -1)), ((1, 0, 2), (-1, 1, 1)), ((2, 0, 1), (1, 1, 1))]:
        _check_equal(*_case(data, perm, sign))


def test_windows_at_every_corner_and_one_voxel():
    data = _data("int16", (33, 65, 31), seed=4)
    for perm, sign in ORIENTATIONS:
        header, raw = _case(data, perm, sign)
        n = [data.shape[k] for k in perm]
        size = [7, 9, 5]
        for corner in np.ndindex(2, 2, 2):
            _check_equal(header, raw, ([c * (m - s) for c, m, s in zip(corner, n, size)], size))
        for start in ([0, 0, 0], [m - 1 for m in n], [m // 2 for m in n]):
            _check_equal(header, raw, (start, [1, 1, 1]))


def test_scaling_is_two_rounded_double_operations():
    _check_equal(*_case(_data("int16", (5, 7, 11), seed=5), (1, 2, 0), (1, -1, 1), slope=0.5, inter=-3.25))
    big = _data("uint32", (5, 7, 11), seed=6)
    big.flat[1:4] = (2 ** 24 + 1, 2 ** 31 + 12345, 2 ** 32 - 1)
    assert (big > 2 ** 24).sum() > 300
    for perm, sign in ORIENTATIONS:
        _check_equal(*_case(big, perm, sign, slope=1e-3, inter=7.0))
        _check_equal(*_case(big, perm, sign))      # and unscaled: one correctly rounded conversion
    _check_equal(*_case(_data("float64", (5, 7, 11), seed=7), (2, 1, 0), (-1, -1, -1), slope=-2.5, inter=0.1))


def _check_normalized(header, raw, window, label):
    from synthanatomy_amd.utils.vqvae import hip_ingest
    got = hip_ingest(header, raw, window, normalize=True, device=DEV)[0].cpu().numpy()
    want, _ = ingest_ref(header, raw, window, normalize=True)
    assert got.shape == want.shape and np.isfinite(got).all()
    ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(want), np.float32(2.0 ** -126)))
    print(f"normalisation {label}: max difference {ulps.max():.3f} ulp, {np.abs(got - want).max():.3e} absolute")
    assert ulps.max() <= 1.0, label
    return got


def test_normalisation_matches_the_host_expression():
    for dtype, dims in (("int16", (33, 65, 31)), ("float32", (33, 65, 31)), ("uint8", (64, 1, 33)), ("float64", (5, 7, 11))):
        for perm, sign in ORIENTATIONS:
            header, raw = _case(_data(dtype, dims, seed=8), perm, sign)
            got = _check_normalized(header, raw, None, f"{dtype} {dims} {perm} {sign}")
            assert got.min() == 0.0 and 0.999999 < got.max() <= 1.0
    header, raw = _case(_data("int16", (33, 65, 31), seed=9), (1, 2, 0), (1, -1, 1), slope=0.5, inter=-3.25)
    _check_normalized(header, raw, ([3, 4, 5], [20, 17, 9]), "scaled int16, windowed")


def test_extremes_outside_the_window_and_constant_volume():
    data = np.full((33, 65, 31), 100, dtype=np.int16)
    data[4:30, 4:60, 4:28] = _data("int16", (26, 56, 24), seed=10) // 64 + 100      # inside [-412, 611]
    data.flat[0], data.flat[-1] = -30000, 30000                                     # min at voxel 0, max at the last voxel
    header, raw = _case(data)
    window = ([8, 16, 8], [16, 32, 16])
    got = _check_normalized(header, raw, window, "extremes outside the window")
    inner = data[8:24, 16:48, 8:24].astype(np.float64)
    assert np.allclose(got, (inner + 30000) / 60000, atol=1e-6) and got.min() > 0.49 and got.max() < 0.52
    for dtype in ("int16", "float32"):
        header, raw = _case(np.full((33, 65, 31), 7, dtype=dtype), (2, 1, 0), (-1, -1, -1))
        got = _check_normalized(header, raw, None, f"constant {dtype}")
        assert not got.any()


def test_non_finite_voxels_become_zero_and_are_counted():
    from synthanatomy_amd.utils.vqvae import hip_ingest
    data = _data("float32", (33, 65, 31), seed=11)
    data[0, 0, 0], data[32, 64, 30], data[17, 3, 9] = np.nan, np.nan, np.inf
    finite = data[np.isfinite(data)]
    for perm, sign in ORIENTATIONS:
        header, raw = _case(data, perm, sign)
        got, ws = hip_ingest(header, raw, None, normalize=False, device=DEV, return_workspace=True)
        want, bad = ingest_ref(header, raw, None, normalize=False)
        assert bad == 3 and torch.equal(got[0].cpu(), torch.from_numpy(want)) and int((got == 0).sum()) >= 3
        words = ws.cpu().numpy()
        assert words[3] == 3
        mn, mx = np.array([words[2] & 0xFFFFFFFF, (words[2] >> 32) & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
        assert mn == finite.min() and mx == finite.max()
        _check_normalized(header, raw, None, "with non-finite voxels")
    header, raw = _case(np.full((5, 7, 11), np.nan, dtype=np.float32))      # no finite voxel at all: zeros, min = max = 0
    got, ws = hip_ingest(header, raw, None, normalize=True, device=DEV, return_workspace=True)
    assert not got.any() and ws.cpu().tolist()[2:4] == [0, 385]


def test_workspace_is_left_ready_for_the_next_call():
    from synthanatomy_amd.utils.vqvae import hip_ingest
    a = _case(_data("int16", (33, 65, 31), seed=12), (1, 2, 0), (1, -1, 1))
    b = _case(_data("float32", (64, 1, 33), seed=13) + 1000, (2, 1, 0), (-1, -1, -1))
    for header, raw in (a, b, a):      # back to back on one workspace, nothing cleared in between
        got, ws = hip_ingest(header, raw, None, normalize=True, device=DEV, return_workspace=True)
        want, _ = ingest_ref(header, raw, None, normalize=True)
        assert np.abs(got[0].cpu().numpy() - want).max() <= np.spacing(np.float32(1.0))
        words = ws.cpu().tolist()
        assert words[0] == words[1] == words[4] == words[5] == 0 and words[3] == 0


def test_argument_checks_return_their_code_and_launch_nothing():
    from synthanatomy_amd import _ffi
    lib = _ffi.lib()
    raw = torch.zeros(5 * 7 * 11 * 2 + 16, dtype=torch.uint8, device=DEV)
    y = torch.full((5 * 7 * 11,), -1.0, device=DEV)
    ws = torch.zeros(8, dtype=torch.int64, device=DEV)
    assert lib.sa_volume_ingest_workspace_bytes() <= 64

    def call(raw_ptr=None, nbytes=770, y_ptr=None, ws_ptr=None, null_params=False, **fields):
        P = _ffi.IngestParams(dtype=4, byteswap=0, flags=1, slope=1.0, inter=0.0)
        P.n[:], P.perm[:], P.sign[:], P.off[:], P.ext[:] = (5, 7, 11), (0, 1, 2), (1, 1, 1), (0, 0, 0), (5, 7, 11)
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(P, k)[:] = v
            else:
                setattr(P, k, v)
        return lib.sa_volume_ingest(ctypes.c_void_p(raw.data_ptr() if raw_ptr is None else raw_ptr), nbytes, ctypes.c_void_p(y.data_ptr() if y_ptr is None else y_ptr),
                                    None if null_params else ctypes.byref(P), ctypes.c_void_p(ws.data_ptr() if ws_ptr is None else ws_ptr), _ffi.stream())

    E, U = _ffi.SA_EINVAL, _ffi.SA_EUNSUPPORTED
    assert call(raw_ptr=0) == E and call(y_ptr=0) == E and call(ws_ptr=0) == E and call(null_params=True) == E      # null operands
    assert call(raw_ptr=raw.data_ptr() + 2) == E                                                                       # raw not 16-byte aligned
    assert call(ext=(5, 0, 11)) == E and call(ext=(5, 7, -1)) == E and call(n=(5, 0, 11)) == E                         # an extent / a dim < 1
    assert call(off=(1, 0, 0)) == E and call(off=(0, 0, -1)) == E and call(off=(0, 0, 1), ext=(5, 7, 11)) == E         # a window outside the canonical dims
    assert call(perm=(2, 1, 0)) == E                                                                                   # (5, 7, 11) no longer fits (11, 7, 5)
    assert call(perm=(0, 1, 1)) == E and call(perm=(0, 1, 3)) == E and call(perm=(-1, 1, 2)) == E                      # no permutation
    assert call(nbytes=769) == E and call(dtype=8) == E                                                                # raw_bytes smaller than the dims need
    for code in (0, 1, 32, 128, 1024, 1280, 1536, 3):
        assert call(dtype=code) == U                                                                                   # an unknown dtype
    assert call(n=(2048, 2048, 512), ext=(1, 1, 1), nbytes=1 << 40) == U                                               # 2^31 voxels
    assert call(n=(1 << 30, 2, 1), ext=(1, 1, 1), nbytes=1 << 40) == U and call(n=(46341, 46341, 1), ext=(1, 1, 1), nbytes=1 << 40) == U
    torch.cuda.synchronize()
    assert bool((y == -1.0).all()) and not ws.any()                                                                    # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert not (y == -1.0).any() and not y.any()                                                                       # (a constant volume normalises to 0)
