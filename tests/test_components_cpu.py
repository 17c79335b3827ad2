"""CPU: the connected-component rule of DESIGN §7.17 -- the numpy reference against a flood fill and against scipy, every refusal of
``metrics/components.py`` and of the ``--anomaly_min_component`` / ``--anomaly_connectivity`` flags with no device, ``lesion_scores``, and the ABI."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import components_ref as ref
import run_vqvae as RV
from synthanatomy_amd.engines import anomaly as AS
from synthanatomy_amd.metrics import components as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flood(mask, connectivity):
    """ids by a flood fill in linear-index order: the first voxel met of a component is its smallest"""
    D, H, W = mask.shape
    ids = np.zeros(mask.shape, dtype=np.int64)
    offs = ref.offsets(connectivity)
    for start in range(D * H * W):
        p = np.unravel_index(start, mask.shape)
        if not mask[p] or ids[p]:
            continue
        ids[p] = start + 1
        stack = [p]
        while stack:
            d, h, w = stack.pop()
            for a, b, c in offs:
                q = (d + a, h + b, w + c)
                if 0 <= q[0] < D and 0 <= q[1] < H and 0 <= q[2] < W and mask[q] and not ids[q]:
                    ids[q] = start + 1
                    stack.append(q)
    return ids


def test_the_three_neighbourhoods_have_6_18_and_26_offsets():
    assert [len(ref.offsets(c)) for c in (6, 18, 26)] == [6, 18, 26]
    assert (1, 1, 0) in ref.offsets(18) and (1, 1, 1) not in ref.offsets(18) and (1, 1, 0) not in ref.offsets(6)


@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("shape, p", [((5, 5, 8), 0.5), ((3, 8, 8), 0.3), ((1, 1, 40), 0.6), ((7, 4, 7), 0.15), ((2, 2, 2), 0.5)])
def test_the_reference_equals_a_flood_fill(connectivity, shape, p):
    assert np.prod(shape) <= 200
    mask = np.random.default_rng(connectivity + shape[0]).random(shape) < p
    assert mask.any() and not mask.all()
    got = ref.label_mask(mask, connectivity)
    assert got.dtype == np.int64 and np.array_equal(got, _flood(mask, connectivity))
    assert np.array_equal(got > 0, mask)


def test_the_three_connectivities_differ_on_a_diagonal_pair():
    m = np.zeros((3, 3, 3), dtype=bool)
    m[0, 0, 0] = m[1, 1, 1] = m[2, 2, 1] = True
    assert [np.unique(ref.label_mask(m, c)).size - 1 for c in (6, 18, 26)] == [3, 2, 1]


def test_the_filter_and_the_summaries_on_a_hand_made_volume():
    a = np.zeros((2, 3, 6), dtype=np.float32)
    a[0, 0, 0:3] = 1.0          # three voxels, id 1
    a[1, 2, 5] = 0.5            # one voxel equal to the threshold, id 36
    a[0, 2, 4] = np.nan         # background
    y = np.zeros(a.shape, dtype=np.uint8)
    y[0, 0, 2:5] = 1            # one lesion of three voxels, one of them inside component 1
    y[1, 0, 0] = 7              # one lesion that nothing hits
    ids, s = ref.components(a, 0.5, 6, 1, y)
    assert ids.dtype == np.int32 and ids[0, 0, 1] == 1 and ids[1, 2, 5] == 36 and ids[0, 2, 4] == 0 and (ids > 0).sum() == 4
    assert s == {"components": 2, "components_kept": 2, "voxels_foreground": 4, "voxels_kept": 4, "largest_component": 3, "tp": 1, "fp": 3, "fn": 3,
                 "lesions": 2, "lesions_detected": 1, "kept_true": 1}
    ids, s = ref.components(a, 0.5, 6, 2, y)
    assert ids[1, 2, 5] == 0 and s["components"] == 2 and s["components_kept"] == 1 and s["voxels_kept"] == 3 and s["fp"] == 2
    ids, s = ref.components(a, 0.5, 6, 4, y)
    assert not ids.any() and (s["components_kept"], s["voxels_kept"], s["tp"], s["fn"], s["lesions_detected"], s["kept_true"]) == (0, 0, 0, 4, 0, 0)
    assert ref.components(a, 0.5, 6, 1)[1]["lesions"] is None


@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_the_reference_equals_scipy_relabelled_to_minimum_indices(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = ndi.generate_binary_structure(3, ref.NORM[connectivity])
    for shape in ((19, 21, 67), (24, 40, 16), (33, 2, 5), (1, 1, 300)):
        mask = np.random.default_rng(connectivity).random(shape, dtype=np.float32) >= np.float32(0.8)
        lab, n = ndi.label(mask, structure=structure)
        first = np.full(n + 1, mask.size, dtype=np.int64)
        np.minimum.at(first, lab.ravel(), np.arange(mask.size))
        want = np.where(mask, first[lab] + 1, 0)
        assert np.array_equal(ref.label_mask(mask, connectivity), want)


# ---- refusals, no device ----

def test_check_arguments_accepts_and_returns_what_the_kernel_gets():
    assert C.check_arguments((2, 1, 3, 4, 5), 0.1, 26, 1) == ((2, 3, 4, 5), np.float32(0.1), 26, 1)
    assert C.check_arguments((2, 3, 4, 5), 1, 6, np.int64(7), (2, 3, 4, 5)) == ((2, 3, 4, 5), np.float32(1.0), 6, 7)
    assert C.CONNECTIVITIES == (6, 18, 26)


@pytest.mark.parametrize("args, match", [
    (((2, 3, 4), 0.1, 26, 1), "volumes"),
    (((2, 2, 3, 4, 5), 0.1, 26, 1), "volumes"),
    (((2, 0, 4, 5), 0.1, 26, 1), "every side"),
    (((1, 1 << 11, 1 << 10, 1 << 10), 0.1, 26, 1), r"2\^31 - 1"),
    (((1, 2 ** 31 - 1, 1, 1), 0.1, 26, 1), r"2\^31 - 1"),
    (((2, 3, 4, 5), float("nan"), 26, 1), "threshold"),
    (((2, 3, 4, 5), float("inf"), 26, 1), "threshold"),
    (((2, 3, 4, 5), 1e39, 26, 1), "threshold"),
    (((2, 3, 4, 5), "high", 26, 1), "threshold"),
    (((2, 3, 4, 5), None, 26, 1), "threshold"),
    (((2, 3, 4, 5), 0.1, 8, 1), "connectivity"),
    (((2, 3, 4, 5), 0.1, True, 1), "connectivity"),
    (((2, 3, 4, 5), 0.1, "26", 1), "connectivity"),
    (((2, 3, 4, 5), 0.1, 26, 0), "min_size"),
    (((2, 3, 4, 5), 0.1, 26, -3), "min_size"),
    (((2, 3, 4, 5), 0.1, 26, 2.0), "min_size"),
    (((2, 3, 4, 5), 0.1, 26, True), "min_size"),
    (((2, 3, 4, 5), 0.1, 26, 2 ** 31), "min_size"),
    (((2, 3, 4, 5), 0.1, 26, 1, (2, 3, 4, 6)), "labels"),
])
def test_check_arguments_refuses_by_name(args, match):
    with pytest.raises(ValueError, match=match):
        C.check_arguments(*args)


def test_a_volume_just_below_the_limit_passes_check_arguments():
    assert C.check_arguments((1, 2 ** 31 - 2, 1, 1), 0.0, 6, 1)[0] == (1, 2 ** 31 - 2, 1, 1)


def test_connected_components_refuses_before_any_launch_and_has_no_cpu_path(monkeypatch):
    from synthanatomy_amd import _ffi

    def touched():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(_ffi, "require_gpu", touched)
    a = torch.zeros(2, 1, 3, 4, 5)
    for kw, match in ((dict(threshold=float("nan")), "threshold"), (dict(threshold=0.1, connectivity=7), "connectivity"),
                      (dict(threshold=0.1, min_size=0), "min_size"), (dict(threshold=0.1, labels=torch.zeros(2, 1, 3, 4, 4)), "labels")):
        with pytest.raises(ValueError, match=match):
            C.connected_components(a, **kw)
    with pytest.raises(ValueError, match="volumes"):
        C.connected_components(torch.zeros(3, 4, 5), threshold=0.1)
    with pytest.raises(AssertionError, match="the device was asked for"):      # valid arguments go on to the device: there is nothing else to run
        C.connected_components(a, threshold=0.1)


def test_lesion_scores_on_hand_made_counts():
    assert C.lesion_scores(4, 3, 6, 3) == (0.75, 0.5, 2 * 0.5 * 0.75 / 1.25)
    assert C.lesion_scores(2, 2, 2, 2) == (1.0, 1.0, 1.0)
    assert C.lesion_scores(5, 0, 3, 0) == (0.0, 0.0, 0.0)          # P + R = 0
    assert C.lesion_scores(5, 0, 0, 0) == (0.0, 0.0, 0.0)          # nothing kept: precision 0
    r, p, f = C.lesion_scores(0, 0, 3, 0)                           # no lesion: recall undefined
    assert math.isnan(r) and (p, f) == (0.0, 0.0)
    r, p, f = C.lesion_scores(np.int64(0), np.int64(0), np.int64(0), np.int64(0))
    assert math.isnan(r) and (p, f) == (0.0, 0.0)
    assert all(isinstance(v, float) for v in C.lesion_scores(np.int64(3), np.int64(1), np.int64(2), np.int64(1)))


# ---- the flags ----

class _DeviceTouched(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    from synthanatomy_amd.runtime import ddp

    def touched():
        raise _DeviceTouched()
    monkeypatch.setattr(ddp, "init_distributed", touched)
    monkeypatch.setattr(torch.cuda, "is_available", touched)


def _argv(tmp_path, *extra, mode="anomaly"):
    return ["run", "--training_subjects=synthetic:2", "--validation_subjects=synthetic:2", f"--project_directory={tmp_path}/", "--experiment_name=e",
            f"--mode={mode}", *extra]


def test_the_flags_their_defaults_and_a_full_command_line(tmp_path, no_device):
    from synthanatomy_amd.utils.general import parse_flags
    D = RV.DEFAULTS
    assert (D["anomaly_min_component"], D["anomaly_connectivity"]) == (None, 26)
    cfg = parse_flags(_argv(tmp_path, "--anomaly_threshold=0.125", "--anomaly_min_component=20", "--anomaly_connectivity=18"), D)
    assert (cfg["anomaly_min_component"], cfg["anomaly_connectivity"]) == (20, 18)
    AS._check_anomaly_flags(cfg)
    for extra in (("--anomaly_threshold=0.1", "--anomaly_min_component=1"), ("--anomaly_threshold=0.1", "--anomaly_connectivity=6"),
                  ("--anomaly_threshold=0.1", "--anomaly_min_component=4", "--anomaly_connectivity=26", "--anomaly_labels=/l")):
        with pytest.raises(_DeviceTouched):
            RV.run(_argv(tmp_path, *extra))
    assert "--anomaly_min_component" in RV.__doc__ and "--anomaly_connectivity" in RV.__doc__


@pytest.mark.parametrize("extra, match", [
    (("--anomaly_min_component=4",), r"--anomaly_min_component=4.*--anomaly_threshold"),
    (("--anomaly_connectivity=6",), r"--anomaly_connectivity=6.*--anomaly_threshold"),
    (("--anomaly_threshold=0.1", "--anomaly_min_component=0"), "--anomaly_min_component=0"),
    (("--anomaly_threshold=0.1", "--anomaly_min_component=-2"), "--anomaly_min_component=-2"),
    (("--anomaly_threshold=0.1", "--anomaly_min_component=2.5"), "--anomaly_min_component=2.5"),
    (("--anomaly_threshold=0.1", "--anomaly_min_component=True"), "--anomaly_min_component=True"),
    (("--anomaly_threshold=0.1", "--anomaly_min_component=many"), "--anomaly_min_component=many"),
    (("--anomaly_threshold=0.1", "--anomaly_connectivity=8"), "--anomaly_connectivity=8"),
    (("--anomaly_threshold=0.1", "--anomaly_min_component=4", "--anomaly_connectivity=27"), "--anomaly_connectivity=27"),
    (("--anomaly_threshold=0.1", "--anomaly_connectivity=None"), "--anomaly_connectivity=None"),
    (("--anomaly_threshold=0.1", "--anomaly_connectivity=full"), "--anomaly_connectivity=full"),
])
def test_a_bad_flag_is_refused_by_name_before_the_device(tmp_path, no_device, extra, match):
    with pytest.raises(ValueError, match=match):
        RV.run(_argv(tmp_path, *extra))
    assert not os.path.exists(tmp_path / "e")


@pytest.mark.parametrize("mode", ["training", "extracting", "decoding"])
@pytest.mark.parametrize("flag", ["--anomaly_min_component=4", "--anomaly_connectivity=6"])
def test_the_flags_belong_to_the_anomaly_mode(tmp_path, no_device, mode, flag):
    with pytest.raises(ValueError, match=flag + r".*--mode=anomaly, not --mode=" + mode):
        RV.run(_argv(tmp_path, "--anomaly_threshold=0.1", flag, mode=mode))
    assert not os.path.exists(tmp_path / "e")


# ---- the ABI ----

def _header():
    with open(os.path.join(ROOT, "include", "synthanatomy_hip.h")) as f:
        return f.read()


def test_the_header_and_the_bindings_name_the_two_symbols_and_the_abi_version_stays():
    from synthanatomy_amd import _ffi
    text = _header()
    assert re.search(r"\bint sa_components\(const float \*a, const unsigned char \*label, int32_t \*ids_out, const sa_components_params \*params", text)
    assert re.search(r"\bint64_t sa_components_workspace_bytes\(const sa_components_params \*params\);", text)
    assert {"sa_components", "sa_components_workspace_bytes"} <= set(_ffi.declared_symbols())
    assert _ffi.ABI_VERSION == 5 and re.search(r"#define SA_ABI_VERSION 5\b", text)
    assert "no reference counterpart" in text[text.index("Connected components of a thresholded map"):text.index("sa_components_params {")]


def test_tile_equals_the_headers_constants_and_the_record_has_16_words():
    from synthanatomy_amd import _ffi
    text = _header()
    tile = tuple(int(re.search(rf"SA_COMPONENTS_TILE_{ax} = (\d+)", text).group(1)) for ax in "DHW")
    assert C.TILE == tile == _ffi.COMPONENTS_TILE and all(t >= 1 for t in tile)
    assert int(re.search(r"SA_COMPONENTS_RESULT_WORDS = (\d+)", text).group(1)) == 16 == _ffi.COMPONENTS_RESULT_WORDS
    assert len(C.NAMES) == 5 and len(C.LABEL_NAMES) == 6
    assert C.NAMES == ref.NAMES and C.LABEL_NAMES == ref.LABEL_NAMES


def test_the_params_struct_the_library_and_its_host_side_refusals():
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.build import build
    P = _ffi.ComponentsParams
    assert ctypes.sizeof(P) == 32 and [f[0] for f in P._fields_] == ["B", "D", "H", "W", "connectivity", "min_size", "has_labels", "threshold"]
    assert P.threshold.offset == 28 and P.connectivity.offset == 16
    lib = ctypes.CDLL(build(verbose=False))
    q = lib.sa_components_workspace_bytes
    q.restype, q.argtypes = ctypes.c_int64, [ctypes.POINTER(P)]
    ok = P(B=2, D=19, H=21, W=67, connectivity=26, min_size=1, has_labels=0, threshold=0.5)
    vol = 19 * 21 * 67
    blocks = -(-vol // 2048)      # the flat launches take 2048 voxels per block and leave twelve 64-bit words each

    def aligned(n):
        return (n + 15) // 16 * 16
    assert q(ctypes.byref(ok)) == 2 * aligned(2 * vol * 4) + 2 * blocks * 12 * 8
    ok.has_labels = 1
    assert q(ctypes.byref(ok)) == 2 * aligned(2 * 2 * vol * 4) + 2 * blocks * 12 * 8
    for field, bad in (("connectivity", 8), ("connectivity", 0), ("min_size", 0), ("min_size", -1), ("threshold", float("nan")),
                       ("threshold", float("inf")), ("B", 0), ("W", 0), ("D", -1)):
        Q = P.from_buffer_copy(ok)
        setattr(Q, field, bad)
        assert q(ctypes.byref(Q)) == _ffi.SA_EINVAL, (field, bad)
    big = P(B=1, D=2 ** 31 - 1, H=1, W=1, connectivity=6, min_size=1, has_labels=0, threshold=0.0)
    assert q(ctypes.byref(big)) == _ffi.SA_EINVAL
    big.D = 1 << 11
    big.H = big.W = 1 << 10
    assert q(ctypes.byref(big)) == _ffi.SA_EINVAL
    big.D, big.H, big.W = 2 ** 31 - 2, 1, 1
    assert q(ctypes.byref(big)) > 0
    # the entry point refuses the same, and null operands, before it touches a device
    run = lib.sa_components
    run.restype = ctypes.c_int
    run.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(P), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    bad = P(B=1, D=4, H=4, W=4, connectivity=7, min_size=1, has_labels=0, threshold=0.0)
    assert run(256, None, 256, ctypes.byref(bad), 256, 256, None) == _ffi.SA_EINVAL
    bad.connectivity = 6
    assert run(None, None, 256, ctypes.byref(bad), 256, 256, None) == _ffi.SA_EINVAL
    assert run(256, 256, 256, ctypes.byref(bad), 256, 256, None) == _ffi.SA_EINVAL      # labels the params do not announce
    bad.has_labels = 1
    assert run(256, None, 256, ctypes.byref(bad), 256, 256, None) == _ffi.SA_EINVAL
