"""GPU: sa_anomaly_map_ensemble (csrc/anomaly.hip) on the five shapes of tests/test_anomaly_gpu.py (tests/anomaly_ensemble_ref.CASES), the
smallest at which the tiling, ragged tiles, a window wider than the axis, unequal factors and the path without a grid can go wrong:

  wide    24 x 40 x 16, latent 3 x 5 x 2, sigma 4      ragged  18 x 14 x 22, latent 9 x 7 x 11, sigma 1.5      beyond  8 x 12 x 20, latent 2 x 3 x 5, sigma 8
  mixed   16 x 8 x 24, latent 2 x 4 x 3, sigma 2       plain   18 x 14 x 22, no weight grid, sigma 0

every case at B = 2 with seeded inputs, a label volume and a threshold.  The rule carries no tolerance: the ensemble map is held bit for bit to
``compose_fp32`` of the maps ``anomaly_map`` returns for the members; against the fp64 mean it is held to the derived bound of
tests/anomaly_ensemble_ref.py, which two witnesses must fail.  Integer outputs, sum and maximum are held to the kernel's OWN map."""
import functools
import math

import numpy as np
import pytest

import anomaly_ensemble_ref as ER
import anomaly_ref

pytestmark = pytest.mark.gpu

CASES, MODES = ER.CASES, ER.MODES
THRESHOLD, HIST_MAX = 0.05, 0.5
KEYS = ("map", "sum", "max", "tp", "fp", "fn", "hist")


def _dev():
    import torch
    return torch.device("cuda", 0)


def _out(amap, s):
    out = {k: s[k].cpu().numpy() for k in ("sum", "max", "tp", "fp", "fn", "hist")}
    out.update(map=amap.cpu().numpy(), inv_bin=s["inv_bin"], threshold=s["threshold"])
    return out


@functools.lru_cache(maxsize=None)
def _single(case, mode, k):
    """what ``anomaly_map`` gives for member k alone"""
    import torch
    from synthanatomy_amd.metrics.anomaly import anomaly_map
    x, r, m, labels = ER.inputs(case)
    t = lambda v: torch.from_numpy(np.array(v)).to(_dev())      # noqa: E731  (a writable copy: the shared inputs are read-only)
    return _out(*anomaly_map(t(x), t(r[k]), None if m is None else t(m[k]), sigma=CASES[case][2], residual=mode, labels=t(labels), threshold=THRESHOLD,
                             hist_max=HIST_MAX))


def _launch(case, mode, members, pick=slice(None)):
    """the ensemble over the given member indices, in that order"""
    import torch
    from synthanatomy_amd.metrics.anomaly import anomaly_map_ensemble
    x, r, m, labels = ER.inputs(case)
    idx = list(members)
    t = lambda v: torch.from_numpy(np.array(v)).to(_dev())      # noqa: E731  (a writable copy: the shared inputs are read-only)
    amap, s = anomaly_map_ensemble(t(x[pick]), t(r[idx][:, pick]), None if m is None else t(m[idx][:, pick]), sigma=CASES[case][2], residual=mode,
                                   labels=t(labels[pick]), threshold=THRESHOLD, hist_max=HIST_MAX)
    assert s["members"] == len(idx) and s["inv_members"] == np.float32(1.0 / len(idx)) and s["inv_members"].dtype == np.float32
    return _out(amap, s)


@functools.lru_cache(maxsize=None)
def _run(case, mode, K):
    return _launch(case, mode, range(K))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_one_member_is_anomaly_map_bit_for_bit(case, mode):
    got, want = _run(case, mode, 1), _single(case, mode, 0)
    assert got["map"].shape == (2, *CASES[case][0]) and got["map"].dtype == np.float32
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    assert got["inv_bin"] == want["inv_bin"] and got["threshold"] == want["threshold"]


@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_map_is_the_fp32_composition_of_the_members_maps_bit_for_bit(case, K):
    for mode in MODES:
        want = ER.compose_fp32([_single(case, mode, k)["map"] for k in range(K)])
        assert _run(case, mode, K)["map"].tobytes() == want.tobytes(), mode


@pytest.mark.parametrize("case", sorted(CASES))
def test_two_members_swapped_give_the_same_bits(case):
    swapped = _launch(case, "abs", (1, 0))
    for k in KEYS:
        assert swapped[k].tobytes() == _run(case, "abs", 2)[k].tobytes(), k


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_three_members_stay_inside_the_derived_bound_and_the_witnesses_do_not(case, mode):
    good, unscaled, rotated = ER.worst_ratios(_run(case, mode, 3)["map"], case, 3, mode)
    print(f"{case} {mode} K = 3: worst |err| / bound = {good:.4f}; witness without inv_K {unscaled:.4g}; witness with rotated weights {rotated:.4g}")
    assert good <= 1.0
    if CASES[case][1] is not None:      # (without grids every weight is 1: nothing to rotate)
        assert unscaled > 1.0 and rotated > 1.0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_integer_outputs_sum_and_max_against_the_kernels_own_map(case, mode):
    _, _, _, labels = ER.inputs(case)
    got = _run(case, mode, 3)
    assert got["inv_bin"] == np.float32(256.0 / HIST_MAX) and got["threshold"] == np.float32(THRESHOLD)
    for b in range(2):
        a = got["map"][b]
        assert np.array_equal(got["hist"][b], anomaly_ref.histograms(a, labels[b], got["inv_bin"]))
        assert (int(got["tp"][b]), int(got["fp"][b]), int(got["fn"][b])) == anomaly_ref.counts(a, labels[b], got["threshold"])
        exact = math.fsum(a.astype(np.float64).ravel().tolist())
        assert abs(float(got["sum"][b]) - exact) <= 1e-12 * exact
        assert got["max"][b] == a.max() and got["max"].dtype == np.float32
    assert got["hist"][:, 1].sum() == labels.sum() and got["hist"].sum() == labels.size


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_volume_alone_equals_itself_in_the_batch_and_launches_repeat(case):
    both = _run(case, "abs", 3)
    alone = _launch(case, "abs", range(3), pick=slice(1, 2))
    again = _launch(case, "abs", range(3))
    for k in KEYS:
        assert alone[k].tobytes() == both[k][1:2].tobytes(), k
        assert again[k].tobytes() == both[k].tobytes(), k


def test_the_limits():
    import torch
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.metrics.anomaly import anomaly_map_ensemble
    case = "beyond"
    x, r, m, labels = (torch.from_numpy(np.array(v)).to(_dev()) for v in ER.inputs(case))
    sigma = CASES[case][2]
    # sixteen members run and equal the composition
    want = ER.compose_fp32([_single(case, "abs", k)["map"] for k in range(16)])
    assert _run(case, "abs", 16)["map"].tobytes() == want.tobytes()
    # seventeen are refused with no launch
    with _ffi.kernel_log() as launched:
        with pytest.raises(ValueError, match="recons holds 17 members"):
            anomaly_map_ensemble(x, torch.cat([r, r[:1]]), torch.cat([m, m[:1]]), sigma=sigma)
        with pytest.raises(ValueError, match="weights for 2 of 3 members"):
            anomaly_map_ensemble(x, [r[0], r[1], r[2]], [m[0], None, m[2]], sigma=sigma)
    assert launched == []
    # a sequence, one member of it not contiguous (it is copied), and volumes as [B, 1, D, H, W]
    strided = torch.stack([r[1], r[1]], dim=-1)[..., 0]
    assert not strided.is_contiguous() and torch.equal(strided, r[1])
    amap, s = anomaly_map_ensemble(x[:, None], [r[0][:, None], strided[:, None], r[2][:, None]], [m[0], m[1], m[2]], sigma=sigma, labels=labels[:, None],
                                   threshold=THRESHOLD, hist_max=HIST_MAX)
    assert amap.shape == x[:, None].shape and amap.cpu().numpy()[:, 0].tobytes() == _run(case, "abs", 3)["map"].tobytes()
    assert s["hist"].cpu().numpy().tobytes() == _run(case, "abs", 3)["hist"].tobytes() and s["members"] == 3
    # without a threshold and labels: no counts, everything class 0
    _, s = anomaly_map_ensemble(x, r[:2], m[:2], sigma=sigma)
    assert s["tp"] is None and not s["hist"][:, 1].any() and bool((s["hist"][:, 0].sum(dim=1) == x[0].numel()).all())
