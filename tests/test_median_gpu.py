"""GPU: ``median_filter_map`` (sa_anomaly_median) against the numpy reference of tests/median_ref.py.  The median is an order statistic
under a total order of the fp32 bits, so ``out`` is compared by exact bit equality; the integer summaries exactly, the fp64 sum within the rounding of
n additions in any order.  Shapes: below the window, one line, one past a tile side on every axis, exactly one tile, 2 x 2 x 2 tiles minus one voxel
per axis (derived from the ``TILE`` the module exports)."""
import ctypes
import functools

import numpy as np
import pytest

import median_ref as ref
from synthanatomy_amd.metrics import median as M

pytestmark = pytest.mark.gpu

T = M.TILE
ONE_TILE = tuple(T)
EIGHT_TILES = tuple(2 * t - 1 for t in T)
SHAPES = [(5, 5, 5), (2, 3, 5), (1, 1, 70), (70, 1, 1), (9, 17, 33), ONE_TILE, EIGHT_TILES]
CONTENTS = ["normal", "sparse", "levels", "zeros", "special", "constant", "ramp_d", "ramp_h", "ramp_w"]
MASKS = ["random", "ball", "all", "none"]
SIZES = (1, 3, 5)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


@functools.lru_cache(maxsize=None)
def _volume(shape, content, seed=0):
    rng = np.random.default_rng(seed + 1000 * CONTENTS.index(content) + sum(shape))
    n = int(np.prod(shape))
    if content == "normal":
        a = rng.standard_normal(shape)
    elif content == "sparse":      # 95 % exact zeros: the early-outs
        a = rng.standard_normal(shape) * (rng.random(shape) < 0.05)
        a = np.where(a == 0, 0.0, a)
    elif content == "levels":      # ties everywhere
        a = rng.choice(np.array([-1.5, 0.25, 2.0]), size=shape)
    elif content == "zeros":       # -0 and +0 are different elements of the order
        a = rng.choice(np.array([-0.0, 0.0]), size=shape)
    elif content == "special":
        a = rng.standard_normal(shape).astype(np.float32)
        pick = rng.random(shape)
        a[pick < 0.08] = np.float32(np.nan)
        a[(pick >= 0.08) & (pick < 0.16)] = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]      # a negative NaN
        a[(pick >= 0.16) & (pick < 0.22)] = np.float32(np.inf)
        a[(pick >= 0.22) & (pick < 0.28)] = np.float32(-np.inf)
    elif content == "constant":
        a = np.full(shape, 0.75)
    else:
        axis = "dhw".index(content[-1])
        a = np.arange(n).reshape(shape) * 0.0 + np.arange(shape[axis]).reshape([-1 if i == axis else 1 for i in range(3)]) * 0.37 - 1.0
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _mask(shape, kind):
    if kind == "random":       # 90 % foreground
        m = np.random.default_rng(7 + sum(shape)).random(shape) < 0.9
    elif kind == "ball":       # touches the volume's border on every axis
        g = np.meshgrid(*[(np.arange(s) - (s - 1) / 2) / max(s / 2, 1) for s in shape], indexing="ij")
        m = g[0] ** 2 + g[1] ** 2 + g[2] ** 2 <= 1.0
    elif kind == "all":
        m = np.ones(shape, dtype=bool)
    else:
        m = np.zeros(shape, dtype=bool)
    m = (m * 3).astype(np.uint8)      # any non-zero byte is foreground
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _want(shape, content, k, mask_kind=None, e=0, seed=0):
    """the reference's output for one volume: computed once, shared, read-only"""
    out = ref.median(_volume(shape, content, seed), k, None if mask_kind is None else _mask(shape, mask_kind), e)
    out.setflags(write=False)
    return out


def _run(a, k, mask=None, e=0, labels=None, threshold=None, hist_max=1.0):
    """``a`` [B, D, H, W] numpy -> (out numpy, summaries of numpy arrays)"""
    import torch
    dev = lambda v: None if v is None else torch.from_numpy(np.array(v)).cuda()
    out, s = M.median_filter_map(dev(a), size=k, mask=dev(mask), erosion=e, labels=dev(labels), threshold=threshold, hist_max=hist_max)
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(a.shape)
    return out.cpu().numpy(), {key: (v.cpu().numpy() if hasattr(v, "cpu") else v) for key, v in s.items()}


def _same_bits(got, want, what):
    gb, wb = _bits(got), _bits(want)
    assert gb.shape == wb.shape and gb.tobytes() == wb.tobytes(), (what, int((gb != wb).sum()), np.argwhere(gb != wb)[:4].tolist())


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_content_on_every_shape_equals_the_reference_bit_for_bit(shape, content):
    a = _volume(shape, content)
    for k in SIZES:
        out, _ = _run(a[None], k)
        _same_bits(out[0], _want(shape, content, k), (shape, content, k))
    _same_bits(_want(shape, content, 1), a, "size 1 without a mask is the identity")


@pytest.mark.parametrize("e", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("shape", [(2, 3, 5), (70, 1, 1), (9, 17, 33), EIGHT_TILES])
def test_masks_and_every_erosion_count(shape, kind, e):
    m = _mask(shape, kind)
    for k, content in ((1, "special"), (3, "normal"), (5, "special")):
        out, _ = _run(_volume(shape, content)[None], k, m[None], e)
        _same_bits(out[0], _want(shape, content, k, kind, e), (shape, kind, e, k))
        if kind == "none":
            assert not _bits(out).any()      # all background: +0.0 everywhere
    if kind == "all" and e > 0:
        assert not ref.erode(m != 0, e)[0].any()      # the volume's outside is background: the border erodes


def test_the_ball_erodes_to_something_and_the_mask_matters():
    shape = EIGHT_TILES
    kept = [int(ref.erode(_mask(shape, "ball") != 0, e).sum()) for e in range(5)]
    assert all(a > b > 0 for a, b in zip(kept, kept[1:]))
    assert _bits(_want(shape, "normal", 5, "ball", 2)).tobytes() != _bits(_want(shape, "normal", 5)).tobytes()


@pytest.mark.parametrize("k", SIZES)
def test_a_volume_has_the_same_bits_alone_and_in_a_batch(k):
    """a halo that reads the neighbouring volume instead of zeros shows here: the three volumes differ and are contiguous"""
    shape = (9, 17, 33)
    vols = [("normal", 0), ("special", 1), ("sparse", 2)]
    a = np.stack([_volume(shape, c, s) for c, s in vols])
    m = np.stack([_mask(shape, "random"), _mask(shape, "ball"), _mask(shape, "all")])
    y = (np.random.default_rng(3).random(a.shape) < 0.3).astype(np.uint8)
    out, s = _run(a, k, m, 1, y, 0.1)
    for b, (c, seed) in enumerate(vols):
        _same_bits(out[b], ref.median(a[b], k, m[b], 1), (k, b))
        one, s1 = _run(a[b:b + 1], k, m[b:b + 1], 1, y[b:b + 1], 0.1)
        _same_bits(one[0], out[b], (k, b, "alone"))
        for key in ("sum", "max", "tp", "fp", "fn", "hist"):
            assert s1[key][0].tobytes() == s[key][b].tobytes(), (k, b, key)
    # without a mask the window of the first and last planes would reach into the neighbours
    out, _ = _run(a, k)
    for b in range(3):
        _same_bits(out[b], ref.median(a[b], k), (k, b, "no mask"))


def test_two_calls_on_one_workspace_give_the_same_bits():
    import torch
    from synthanatomy_amd import _ffi
    shape = EIGHT_TILES
    a = torch.from_numpy(np.stack([_volume(shape, "normal"), _volume(shape, "sparse")])).cuda()
    m = torch.from_numpy(np.stack([_mask(shape, "ball"), _mask(shape, "random")])).cuda()
    y = (torch.rand(a.shape, device="cuda") < 0.2).to(torch.uint8)
    P = _ffi.MedianParams(B=2, D=shape[0], H=shape[1], W=shape[2], size=5, erosion=3, has_mask=1, has_labels=1, has_threshold=1, inv_bin=256.0,
                          threshold=0.25)
    lib = _ffi.lib()
    nbytes = lib.sa_anomaly_median_workspace_bytes(ctypes.byref(P))
    assert nbytes > 0
    ws = torch.full(((nbytes + 7) // 8,), float("nan"), dtype=torch.float64, device="cuda")
    got = []
    for _ in range(2):
        out = torch.full_like(a, -7.0)
        res = torch.full((2, _ffi.ANOMALY_RESULT_WORDS), -1, dtype=torch.int64, device="cuda")
        _ffi.check(lib.sa_anomaly_median(_ffi.ptr(a), _ffi.ptr(m), _ffi.ptr(y), _ffi.ptr(out), ctypes.byref(P), _ffi.ptr(res), _ffi.ptr(ws), _ffi.stream()))
        got.append((out.cpu().numpy(), res.cpu().numpy()))
    assert _bits(got[0][0]).tobytes() == _bits(got[1][0]).tobytes() and got[0][1].tobytes() == got[1][1].tobytes()
    for b, (c, kind) in enumerate((("normal", "ball"), ("sparse", "random"))):
        _same_bits(got[0][0][b], _want(shape, c, 5, kind, 3), b)
    assert not got[0][1][:, 5:8].any()      # words 5..7 of the record stay 0


@pytest.mark.parametrize("labelled, threshold", [(True, 0.25), (True, None), (False, 0.25), (False, None)])
@pytest.mark.parametrize("k", SIZES)
def test_the_summaries_are_those_of_the_kernels_own_output(k, labelled, threshold):
    shape = (9, 17, 33)
    rng = np.random.default_rng(k)
    a = np.abs(np.stack([_volume(shape, "normal"), _volume(shape, "sparse", 1)])) * np.float32(0.8)      # finite, non-negative, many above hist_max
    m = np.stack([_mask(shape, "random"), _mask(shape, "ball")])
    y = (rng.random(a.shape) < 0.25).astype(np.uint8) if labelled else None
    hist_max = 0.25
    out, s = _run(a, k, m, 1, y, threshold, hist_max)
    assert s["inv_bin"] == np.float32(256 / hist_max) and s["taps"] is None
    wants = [ref.summaries(out[b], s["inv_bin"], None if y is None else y[b], threshold) for b in range(2)]
    # the inputs exercise the clamp to bin 255, the middle bins and, with a threshold, both predictions
    assert sum(w["hist"][:, 255].sum() for w in wants) > 0 and sum(w["hist"][:, 1:255].sum() for w in wants) > 0
    if threshold is not None:
        assert labelled == (sum(w["tp"] + w["fn"] for w in wants) > 0) and sum(w["tp"] + w["fp"] for w in wants) > 0
    for b, want in enumerate(wants):
        assert np.array_equal(s["hist"][b], want["hist"]) and s["hist"][b].sum() == out[b].size
        assert s["max"][b] == want["max"] and s["max"].dtype == np.float32
        if threshold is None:
            assert s["tp"] is None and s["fp"] is None and s["fn"] is None and s["threshold"] is None
        else:
            assert (int(s["tp"][b]), int(s["fp"][b]), int(s["fn"][b])) == (want["tp"], want["fp"], want["fn"])
        bound = out[b].size * 2.0 ** -53 * float(np.abs(out[b].astype(np.float64)).sum())
        print(f"k={k} b={b}: sum {s['sum'][b]!r} against {want['sum']!r}, bound {bound:.3e}")
        assert abs(float(s["sum"][b]) - want["sum"]) <= bound


def test_size_one_without_a_mask_returns_the_maps_bits():
    a = np.stack([_volume(EIGHT_TILES, "special"), _volume(EIGHT_TILES, "zeros")])
    out, _ = _run(a, 1)
    _same_bits(out, a, "identity")
