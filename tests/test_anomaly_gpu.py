"""GPU: sa_anomaly_map (csrc/anomaly.hip) at the smallest shapes at which it can go wrong, every case at B = 2 with a different x, m and
label per volume and once per residual mode:

  wide    24 x 40 x 16, latent 3 x 5 x 2, sigma 4     R = 12: the window crosses more than one cell and covers most of the 16-wide axis
  ragged  18 x 14 x 22, latent 9 x 7 x 11, sigma 1.5  no side is a tile multiple; odd latent sides
  beyond  8 x 12 x 20, latent 2 x 3 x 5, sigma 8      2R + 1 = 49 exceeds every axis
  mixed   16 x 8 x 24, latent 2 x 4 x 3, sigma 2      factors 8, 2, 8
  plain   18 x 14 x 22, no weight grid, sigma 0

The map is held to tests/anomaly_ref.py (fp64) under the element-wise bound of tests/anomaly_bounds.py, which two witnesses must fail; the integer outputs,
the sum and the maximum are held to the kernel's OWN map, exactly (integers, max) or to fp64 rounding (sum)."""
import functools
import math

import numpy as np
import pytest

import anomaly_bounds
import anomaly_ref

pytestmark = pytest.mark.gpu

CASES = {"wide": ((24, 40, 16), (3, 5, 2), 4.0), "ragged": ((18, 14, 22), (9, 7, 11), 1.5), "beyond": ((8, 12, 20), (2, 3, 5), 8.0),
         "mixed": ((16, 8, 24), (2, 4, 3), 2.0), "plain": ((18, 14, 22), None, 0.0)}
MODES = ("abs", "positive", "negative")
THRESHOLD, HIST_MAX = 0.05, 0.5


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """x, r in [0, 1); volume 0 carries a {0, 1} mask, volume 1 an NLL-like grid in nats; labels differ per volume"""
    shape, latent, _ = CASES[case]
    rng = np.random.default_rng(sorted(CASES).index(case))
    x, r = rng.random((2, *shape), dtype=np.float32), rng.random((2, *shape), dtype=np.float32)
    m = None
    if latent is not None:
        m = np.stack([(rng.random(latent) < 0.4).astype(np.float32), (rng.exponential(1.5, latent) * (rng.random(latent) < 0.8)).astype(np.float32)])
    labels = (rng.random((2, *shape)) < np.array([0.3, 0.1]).reshape(2, 1, 1, 1)).astype(np.uint8)
    return x, r, m, labels


@functools.lru_cache(maxsize=None)
def _weights(case):
    """per volume the fp64 weight of the rule and of the two witnesses, computed once and shared by the three residual modes"""
    from synthanatomy_amd.metrics.anomaly import gaussian_taps
    shape, latent, sigma = CASES[case]
    _, _, m, _ = _inputs(case)
    taps = gaussian_taps(sigma)
    return [(anomaly_ref.weight_ref(m[b], shape, taps), anomaly_ref.weight_ref(m[b], shape, taps, cell_shift=1),
             anomaly_ref.weight_ref(m[b], shape, anomaly_ref.unnormalised_taps(sigma))) for b in range(2)]


def _launch(case, mode, pick=slice(None), labelled=True):
    import torch
    from synthanatomy_amd.metrics.anomaly import anomaly_map
    x, r, m, labels = _inputs(case)
    dev = torch.device("cuda", 0)
    t = lambda v: None if v is None else torch.from_numpy(v[pick]).to(dev)      # noqa: E731
    amap, s = anomaly_map(t(x), t(r), t(m), sigma=CASES[case][2], residual=mode, labels=t(labels) if labelled else None, threshold=THRESHOLD,
                          hist_max=HIST_MAX)
    out = {k: s[k].cpu().numpy() for k in ("sum", "max", "tp", "fp", "fn", "hist")}
    out.update(map=amap.cpu().numpy(), inv_bin=s["inv_bin"], threshold=s["threshold"])
    return out


@functools.lru_cache(maxsize=None)
def _run(case, mode):
    return _launch(case, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_map_stays_inside_the_derived_bound_and_the_witnesses_do_not(case, mode):
    shape, latent, sigma = CASES[case]
    x, r, m, _ = _inputs(case)
    got = _run(case, mode)["map"]
    assert got.shape == (2, *shape) and got.dtype == np.float32
    R = math.ceil(3 * sigma)
    c = anomaly_bounds.chain_length(shape, latent, R)
    for b in range(2):
        e = anomaly_ref.residual(x[b], r[b], mode)
        w, w_shift, w_raw = _weights(case)[b] if latent is not None else (np.ones(shape),) * 3
        bound = anomaly_bounds.map_bound(e * w, w, x[b], r[b], c)
        ratio = anomaly_bounds.worst_ratio(got[b], e * w, bound)
        print(f"{case} {mode} volume {b}: c = {c}, worst |err| / bound = {ratio:.4f}, max a = {float(got[b].max()):.6g}")
        assert ratio < 1.0
        if latent is not None:      # (no weight grid: there is no cell boundary and no tap to get wrong)
            for name, wrong in (("cell boundary (p + 1) // f", w_shift), ("unnormalised taps", w_raw)):
                far = anomaly_bounds.worst_ratio(got[b], e * wrong, anomaly_bounds.map_bound(e * wrong, wrong, x[b], r[b], c))
                print(f"    witness {name}: {far:.4g}")
                assert far > 1.0, name


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_integer_outputs_sum_and_max_against_the_kernels_own_map(case, mode):
    _, _, _, labels = _inputs(case)
    got = _run(case, mode)
    assert got["inv_bin"] == np.float32(256.0 / HIST_MAX) and got["threshold"] == np.float32(THRESHOLD)
    for b in range(2):
        a = got["map"][b]
        assert np.array_equal(got["hist"][b], anomaly_ref.histograms(a, labels[b], got["inv_bin"]))
        assert (int(got["tp"][b]), int(got["fp"][b]), int(got["fn"][b])) == anomaly_ref.counts(a, labels[b], got["threshold"])
        exact = math.fsum(a.astype(np.float64).ravel().tolist())
        assert abs(float(got["sum"][b]) - exact) <= 1e-12 * exact
        assert got["max"][b] == a.max() and got["max"].dtype == np.float32
    assert got["hist"][:, 1].sum() == labels.sum() and got["hist"].sum() == labels.size
    if case in ("plain", "ragged"):      # residuals up to 1 (times NLL weights up to several nats) pass hist_max = 0.5: the clamp to bin 255 is exercised
        assert got["hist"][:, :, 255].sum() > 0
    # without labels everything is class 0 and nothing is a true positive
    free = _launch(case, mode, labelled=False)
    assert np.array_equal(free["map"], got["map"]) and np.array_equal(free["hist"][:, 0], got["hist"].sum(axis=1)) and not free["hist"][:, 1].any()
    assert not free["tp"].any() and not free["fn"].any() and np.array_equal(free["fp"], got["tp"] + got["fp"])


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_volume_alone_equals_itself_in_the_batch_and_launches_repeat(case):
    both = _run(case, "abs")
    alone = _launch(case, "abs", pick=slice(1, 2))
    again = _launch(case, "abs")
    for k in ("map", "sum", "max", "tp", "fp", "fn", "hist"):
        assert alone[k].tobytes() == both[k][1:2].tobytes(), k
        assert again[k].tobytes() == both[k].tobytes(), k


def test_the_limits():
    import torch
    from synthanatomy_amd.metrics.anomaly import anomaly_map
    dev = torch.device("cuda", 0)
    x, r, m, labels = (torch.from_numpy(v).to(dev) for v in _inputs("mixed"))
    for mode, e in (("abs", (x - r).abs()), ("positive", (x - r).clamp(min=0)), ("negative", (r - x).clamp(min=0))):
        plain, s = anomaly_map(x, r, None, sigma=3.0, residual=mode, labels=labels)
        assert torch.equal(plain, e) and s["tp"] is None and s["taps"] is None
        ones, _ = anomaly_map(x, r, torch.ones_like(m), sigma=0, residual=mode)
        assert torch.equal(ones, e)
        zero, s = anomaly_map(x, r, torch.zeros_like(m), sigma=2.0, residual=mode, labels=labels, threshold=1e-6)
        assert not zero.any() and float(s["sum"].sum()) == 0.0 and float(s["max"].max()) == 0.0
        hist = s["hist"].cpu().numpy()
        assert not hist[:, :, 1:].any() and np.array_equal(hist[:, 1, 0], _inputs("mixed")[3].reshape(2, -1).sum(axis=1))
        assert not s["tp"].any() and not s["fp"].any() and np.array_equal(s["fn"].cpu().numpy(), hist[:, 1, 0])
        _, s = anomaly_map(x, r, torch.zeros_like(m), sigma=2.0, residual=mode)      # no label: the class-1 histogram is empty
        assert not s["hist"][:, 1].any() and bool((s["hist"][:, 0, 0] == x[0].numel()).all())
    # [B, 1, D, H, W] in, the same shape out, the same numbers
    five, _ = anomaly_map(x[:, None], r[:, None], m, sigma=2.0, labels=labels[:, None])
    assert five.shape == x[:, None].shape and torch.equal(five[:, 0], torch.from_numpy(_run("mixed", "abs")["map"]).to(dev))
