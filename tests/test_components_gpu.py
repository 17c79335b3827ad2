"""GPU: ``connected_components`` (sa_components) against the numpy reference of tests/components_ref.py.  Everything is an integer, so every
comparison is exact equality.  Batches of two different volumes with different labels; shapes that are ragged against the tile, below a tile, one line,
and one built from ``TILE`` on which the largest component provably crosses tiles along every axis."""
import functools

import numpy as np
import pytest

import components_ref as ref
from synthanatomy_amd.metrics import components as C

pytestmark = pytest.mark.gpu

T = C.TILE
P = {6: 0.30, 18: 0.13, 26: 0.09}      # near each lattice's site-percolation threshold: components sprawl
TILE_SHAPE = (2 * T[0] + 3, 2 * T[1] + 1, 2 * T[2] + 5)
SHAPES = [(19, 21, 67), (24, 40, 16), (18, 14, 22), (33, 2, 5), (1, 1, 300), TILE_SHAPE]
WRONG = {26: 18, 18: 6}


@functools.lru_cache(maxsize=None)
def _fields(shape, c):
    """(a [2, D, H, W] fp32, t, labels [2, D, H, W] uint8): two volumes and, at half the density, two label volumes"""
    rng = np.random.default_rng(c)
    a = rng.random((2,) + shape, dtype=np.float32)
    y = (rng.random((2,) + shape, dtype=np.float32) >= np.float32(1.0 - P[c] / 2)).astype(np.uint8)
    a.setflags(write=False)
    y.setflags(write=False)
    return a, np.float32(1.0 - P[c]), y


@functools.lru_cache(maxsize=None)
def _full(shape, c, c_ref=None):
    """the unfiltered canonical ids of the two volumes under connectivity c_ref (default c): computed once, shared, read-only"""
    a, t, _ = _fields(shape, c)
    out = np.stack([ref.label_mask(ref.foreground(a[b], t), c_ref or c) for b in range(2)])
    out.setflags(write=False)
    return out


def _want(shape, c, n, labels=True):
    a, t, y = _fields(shape, c)
    full = _full(shape, c)
    return [ref.filter_ids(full[b], c, n, y[b] if labels else None) for b in range(2)]


def _run(a, t, c, n, y=None):
    import torch
    ids, s = C.connected_components(torch.from_numpy(np.array(a)).cuda(), threshold=t, connectivity=c, min_size=n,
                                    labels=None if y is None else torch.from_numpy(np.array(y)).cuda())
    assert ids.dtype == torch.int32 and tuple(ids.shape) == tuple(a.shape)
    return ids.cpu().numpy(), {k: (None if v is None else v.cpu().numpy()) for k, v in s.items()}


def _check(ids, s, want):
    for b, (wi, ws) in enumerate(want):
        got = {k: (None if v is None else int(v[b])) for k, v in s.items()}
        assert got == ws, (b, got, ws)
        assert ids[b].tobytes() == wi.tobytes(), (b, int((ids[b] != wi).sum()))


def _largest(shape, c, b=0):
    sizes = np.bincount(_full(shape, c)[b].ravel())
    sizes[0] = 0
    return int(sizes.argmax()), int(sizes.max())


def test_the_references_figures_on_the_first_shape():
    got = [ref.filter_ids(_full(SHAPES[0], c)[0], c, 1)[1] for c in (6, 18, 26)]
    assert [g["components"] for g in got] == [1713, 669, 496] and [g["largest_component"] for g in got] == [602, 305, 266]


@pytest.mark.parametrize("c", [6, 18, 26])
def test_on_the_tile_derived_shape_the_largest_component_crosses_tiles_along_every_axis_and_the_filter_bites(c):
    for b in range(2):
        big, _ = _largest(TILE_SHAPE, c, b)
        for (lo, hi), t in zip(ref.extents(_full(TILE_SHAPE, c)[b], big), T):
            assert lo // t < hi // t, (b, lo, hi, t)
        for n in (2, 8):
            s = ref.filter_ids(_full(TILE_SHAPE, c)[b], c, n)[1]
            assert 0 < s["components_kept"] < s["components"]


@pytest.mark.parametrize("c", [6, 18, 26])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_fields_near_percolation(shape, c):
    a, t, y = _fields(shape, c)
    top = max(_largest(shape, c, b)[1] for b in range(2))
    for n in (1, 2, 8, top + 1):
        ids, s = _run(a, t, c, n, y)
        _check(ids, s, _want(shape, c, n))
        if n == top + 1:
            assert not ids.any() and not s["components_kept"].any() and not s["voxels_kept"].any() and not s["lesions_detected"].any()
    ids, s = _run(a[:, None], t, c, 2)      # [B, 1, D, H, W], no labels: the label summaries are None
    assert ids.shape == (2, 1) + shape
    _check(ids[:, 0], s, _want(shape, c, 2, labels=False))
    # the witness: a reference with a smaller neighbourhood differs, so a dropped class of offsets would show.  (On the one-line shape the three
    # neighbourhoods are the same two voxels, so there the references must coincide instead: no field can tell them apart.)
    if c in WRONG:
        wrong = _full(shape, c, WRONG[c])
        ids, _ = _run(a, t, c, 1)
        for b in range(2):
            if sum(n > 1 for n in shape) >= 2:
                assert not np.array_equal(ids[b], wrong[b])
            else:
                assert np.array_equal(_full(shape, c)[b], wrong[b])


def _offsets26():
    return [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]


@pytest.mark.parametrize("c", [6, 18, 26])
def test_every_contact_across_a_tile_boundary(c):
    shape = (3 * T[0], 3 * T[1], 3 * T[2])
    offs = _offsets26()
    a = np.zeros((len(offs),) + shape, dtype=np.float32)
    pairs = []
    for i, o in enumerate(offs):
        # a corner voxel of the centre tile from which o leaves the tile along every axis it moves on
        p = tuple(T[k] if o[k] < 0 else 2 * T[k] - 1 for k in range(3))
        q = tuple(p[k] + o[k] for k in range(3))
        assert all((q[k] // T[k] != 1) == (o[k] != 0) for k in range(3))
        a[i][p] = a[i][q] = 1.0
        pairs.append((np.ravel_multi_index(p, shape), np.ravel_multi_index(q, shape)))
    ids, s = _run(a, 0.5, c, 1)
    for i, (o, (lp, lq)) in enumerate(zip(offs, pairs)):
        joined = sum(abs(v) for v in o) <= ref.NORM[c]
        got = (int(ids[i].ravel()[lp]), int(ids[i].ravel()[lq]))
        assert got == ((min(lp, lq) + 1,) * 2 if joined else (lp + 1, lq + 1)), (o, got)
        assert int(s["components"][i]) == (1 if joined else 2) and int(s["voxels_foreground"][i]) == 2 == int((ids[i] > 0).sum())
        assert int(s["largest_component"][i]) == (2 if joined else 1)


def _snake(shape):
    D, H, W = shape
    m = np.zeros(shape, dtype=bool)
    for d in range(0, D, 2):
        m[d, 0::2, :] = True                                   # full rows at even h ...
        for k, h in enumerate(range(1, H, 2)):
            m[d, h, W - 1 if k % 2 == 0 else 0] = True        # ... joined at alternating ends
    for k, d in enumerate(range(1, D, 2)):
        m[d, H - 1 if k % 2 == 0 else 0, 0] = True            # the planes at even d, joined by one voxel at odd d
    return m


def test_structures():
    shape = SHAPES[0]
    D, H, W = shape
    d, h, w = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    board = ((d + h + w) % 2 == 0).astype(np.float32)
    snake = _snake(shape)
    assert ref.offsets(6) and np.unique(ref.label_mask(snake, 6)).tolist() == [0, 1] and snake.sum() > 7000      # ONE component, id 1
    a = np.stack([board, snake.astype(np.float32), np.ones(shape, np.float32), np.zeros(shape, np.float32)])
    n_board = -(-D * H * W // 2)
    for c in (6, 18, 26):
        ids, s = _run(a, 0.5, c, 1)
        assert s["components"].tolist() == [n_board if c == 6 else 1, 1, 1, 0]
        assert s["largest_component"].tolist() == [1 if c == 6 else n_board, int(snake.sum()), D * H * W, 0]
        assert s["voxels_foreground"].tolist() == [n_board, int(snake.sum()), D * H * W, 0]
        want0 = np.where(board > 0, np.arange(1, D * H * W + 1).reshape(shape), 0) if c == 6 else (board > 0).astype(np.int64)
        assert np.array_equal(ids[0], want0)
        assert np.array_equal(ids[1], snake.astype(np.int32)) and np.array_equal(ids[2], np.ones(shape, np.int32)) and not ids[3].any()
        for b in range(4):
            wi, ws = ref.components(a[b], 0.5, c, 1)
            assert ids[b].tobytes() == wi.tobytes() and all(int(s[k][b]) == ws[k] for k in ref.NAMES)
    ids, s = _run(a, 0.5, 6, 2)      # the checkerboard's single voxels go, the rest stays
    assert s["components_kept"].tolist() == [0, 1, 1, 0] and not ids[0].any() and np.array_equal(ids[1], snake.astype(np.int32))


def test_nans_are_background_and_voxels_equal_to_the_threshold_are_foreground():
    shape = SHAPES[2]
    a, t, y = _fields(shape, 18)
    a = a.copy()
    rng = np.random.default_rng(5)
    a[0][rng.random(shape) < 0.2] = np.nan
    a[1][rng.random(shape) < 0.2] = t
    below = np.nextafter(t, np.float32(0), dtype=np.float32)
    a[1][rng.random(shape) < 0.2] = below
    ids, s = _run(a, t, 18, 3, y)
    want = [ref.components(a[b], t, 18, 3, y[b]) for b in range(2)]
    _check(ids, s, want)
    assert not ids[0][np.isnan(a[0])].any()
    assert int(s["voxels_foreground"][1]) == int((a[1] >= t).sum()) > int((a[1] > t).sum())


@pytest.mark.parametrize("c", [6, 26])
def test_a_volume_alone_and_inside_a_batch_of_three_and_two_calls_on_one_workspace_give_the_same_bits(c):
    import ctypes
    import torch
    from synthanatomy_amd import _ffi
    shape = TILE_SHAPE
    a, t, y = _fields(shape, c)
    a3, y3 = np.concatenate([a, a[:1, ::-1]]), np.concatenate([y, y[:1, :, ::-1]])
    ids3, s3 = _run(a3, t, c, 4, y3)
    for b in range(3):
        ids1, s1 = _run(a3[b:b + 1], t, c, 4, y3[b:b + 1])
        assert ids1[0].tobytes() == ids3[b].tobytes()
        assert all(int(s1[k][0]) == int(s3[k][b]) for k in s3)
    # one workspace, two calls (the second over whatever the first left), then a call with other arguments in between
    av, yv = torch.from_numpy(np.ascontiguousarray(a3)).cuda(), torch.from_numpy(np.ascontiguousarray(y3)).cuda()
    lib = _ffi.lib()

    def call(P, ws, lab):
        res = torch.full((3, 16), -7, dtype=torch.int64, device="cuda")
        ids = torch.full(av.shape, -7, dtype=torch.int32, device="cuda")
        _ffi.check(lib.sa_components(_ffi.ptr(av), _ffi.ptr(lab), _ffi.ptr(ids), ctypes.byref(P), _ffi.ptr(res), _ffi.ptr(ws), _ffi.stream()), "sa_components")
        return ids.cpu().numpy(), res.cpu().numpy()
    P = _ffi.ComponentsParams(B=3, D=shape[0], H=shape[1], W=shape[2], connectivity=c, min_size=4, has_labels=1, threshold=float(t))
    ws = torch.full(((lib.sa_components_workspace_bytes(ctypes.byref(P)) + 7) // 8,), float("nan"), dtype=torch.float64, device="cuda")
    first = call(P, ws, yv)
    second = call(P, ws, yv)
    Q = _ffi.ComponentsParams.from_buffer_copy(P)
    Q.connectivity, Q.min_size, Q.has_labels = 6 if c == 26 else 26, 1, 0
    call(Q, ws, None)
    third = call(P, ws, yv)
    assert first[0].tobytes() == second[0].tobytes() == third[0].tobytes() == ids3.tobytes()
    assert first[1].tobytes() == second[1].tobytes() == third[1].tobytes()
    assert not first[1][:, 11:].any() and [int(v) for v in first[1][:, 0]] == [int(v) for v in s3["components"]]


@pytest.mark.parametrize("c", [6, 18, 26])
def test_the_ids_label_themselves_and_the_summaries_follow_from_the_kernels_own_ids(c):
    shape = SHAPES[0]
    a, t, y = _fields(shape, c)
    ids, s = _run(a, t, c, 1, y)
    again, s2 = _run(ids.astype(np.float32), 0.5, c, 1, y)
    assert again.tobytes() == ids.tobytes() and all(np.array_equal(s[k], s2[k]) for k in s)
    n = 5
    ids, s = _run(a, t, c, n, y)
    full, _ = _run(a, t, c, 1)
    for b in range(2):
        sizes = np.bincount(full[b].ravel())
        sizes[0] = 0
        kept = ids[b] > 0
        yy = y[b] != 0
        assert np.array_equal(kept, (sizes >= n)[full[b]]) and np.array_equal(ids[b][kept], full[b][kept])
        assert int(s["components"][b]) == np.count_nonzero(sizes) and int(s["components_kept"][b]) == np.unique(ids[b][kept]).size
        assert int(s["voxels_foreground"][b]) == sizes.sum() and int(s["voxels_kept"][b]) == kept.sum() and int(s["largest_component"][b]) == sizes.max()
        assert (int(s["tp"][b]), int(s["fp"][b]), int(s["fn"][b])) == ((kept & yy).sum(), (kept & ~yy).sum(), (~kept & yy).sum())
        lesion, _ = _run(y[b:b + 1].astype(np.float32), 0.5, c, 1)      # the label volume through the kernel itself
        assert int(s["lesions"][b]) == np.unique(lesion[0][yy]).size
        assert int(s["lesions_detected"][b]) == np.unique(lesion[0][yy & kept]).size
        assert int(s["kept_true"][b]) == np.unique(ids[b][kept & yy]).size
