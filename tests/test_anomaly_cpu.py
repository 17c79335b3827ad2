"""CPU: the host side of the anomaly map -- the fp64 reference against the rule written out, the taps, every refusal, the histogram scores,
the matching of healing outputs and labels by stem, the new flags, and the two symbols in the built library.  No launch is made here."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import anomaly_bounds
import anomaly_ref
import run_vqvae as RV
from synthanatomy_amd.engines import anomaly as AS
from synthanatomy_amd.metrics import anomaly as A


def test_the_reference_equals_the_rule_written_out_voxel_by_voxel():
    rng = np.random.default_rng(0)
    x, r = rng.random((6, 5, 4), dtype=np.float32), rng.random((6, 5, 4), dtype=np.float32)
    for latent, sigma in (((3, 5, 2), 0.7), ((6, 5, 4), 1.0), ((1, 1, 1), 1.4), ((2, 1, 4), 0.0)):
        m = rng.random(latent).astype(np.float32) * (rng.random(latent) < 0.7)
        taps = A.gaussian_taps(sigma)
        for mode in ("abs", "positive", "negative"):
            a, _ = anomaly_ref.anomaly_ref(x, r, m, taps, mode)
            brute = anomaly_ref.anomaly_brute(x, r, m, taps, mode)
            assert np.allclose(a, brute, rtol=1e-13, atol=0), (latent, sigma, mode)
    a, w = anomaly_ref.anomaly_ref(x, r, None, None, "positive")
    assert np.array_equal(a, np.maximum(x.astype(np.float64) - r.astype(np.float64), 0)) and np.all(w == 1)
    # sigma = 0: w is the upsampled grid itself
    m = rng.random((3, 5, 2)).astype(np.float32)
    _, w = anomaly_ref.anomaly_ref(x, r, m, A.gaussian_taps(0), "abs")
    assert np.array_equal(w, np.repeat(np.repeat(m.astype(np.float64), 2, axis=0), 2, axis=2))
    # the witnesses differ from the rule
    taps = A.gaussian_taps(1.0)
    good = anomaly_ref.weight_ref(m, (6, 5, 4), taps)
    assert not np.allclose(anomaly_ref.weight_ref(m, (6, 5, 4), taps, cell_shift=1), good, rtol=1e-3)
    assert not np.allclose(anomaly_ref.weight_ref(m, (6, 5, 4), anomaly_ref.unnormalised_taps(1.0)), good, rtol=1e-3)


@pytest.mark.parametrize("sigma", [0, 0.3, 0.5, 1.0, 1.5, 2, 4, 7.99, 8])
def test_the_taps(sigma):
    g = A.gaussian_taps(sigma)
    R = math.ceil(3 * sigma)
    assert g.dtype == np.float32 and g.shape == (2 * R + 1,) and R <= 24
    total = float(np.sum(g.astype(np.float64)))
    assert abs(total - 1.0) <= 2.0 ** -23      # every tap is rounded once, by at most 2^-24 of itself, and they add up to 1: within 2^-24, a few ulp allowed
    assert np.array_equal(g, g[::-1]) and np.all(g > 0) and g[R] == g.max()
    if sigma == 0:
        assert g.tolist() == [1.0]
    else:
        i = np.arange(-R, R + 1, dtype=np.float64)
        e = np.exp(-i * i / (2.0 * sigma * sigma))
        assert np.array_equal(g, (e / e.sum()).astype(np.float32))


@pytest.mark.parametrize("sigma", [-0.1, 8.01, 100, float("nan"), float("inf"), "wide", None])
def test_a_sigma_outside_the_range_is_refused(sigma):
    with pytest.raises(ValueError, match="sigma"):
        A.gaussian_taps(sigma)
    with pytest.raises(ValueError, match="sigma"):
        A.check_arguments((1, 8, 8, 8), (1, 2, 2, 2), sigma, "abs", None, 1.0)


def test_every_other_refusal_names_what_it_refuses():
    ok = dict(shape=(2, 8, 12, 16), weight_shape=(2, 2, 3, 4), sigma=1.0, residual="abs", threshold=None, hist_max=1.0)
    factors, s, mode, t, inv_bin = A.check_arguments(**ok)
    assert factors == (4, 4, 4) and s == 1.0 and mode == 0 and t is None and inv_bin == np.float32(256.0)
    assert A.check_arguments(**dict(ok, weight_shape=None))[0] is None
    assert A.check_arguments(**dict(ok, residual="negative", threshold=0.25, hist_max=0.5))[2:] == (2, 0.25, np.float32(512.0))
    for bad in ((2, 3, 3, 4), (2, 2, 3, 5), (2, 2, 3, 32), (1, 2, 3, 4), (2, 3, 4), (2, 0, 3, 4)):
        with pytest.raises(ValueError, match=r"\(2, 8, 12, 16\)") as e:
            A.check_arguments(**dict(ok, weight_shape=bad))
        assert str(bad) in str(e.value)
    for hm in (0, -1.0, float("inf"), float("nan"), "big", 1e-40):
        with pytest.raises(ValueError, match="hist_max"):
            A.check_arguments(**dict(ok, hist_max=hm))
    with pytest.raises(ValueError, match="residual.*squared"):
        A.check_arguments(**dict(ok, residual="squared"))
    with pytest.raises(ValueError, match="threshold"):
        A.check_arguments(**dict(ok, threshold=float("nan")))


def test_anomaly_map_refuses_before_any_launch(monkeypatch):
    from synthanatomy_amd import _ffi

    def touched():
        raise AssertionError("the device was reached")
    monkeypatch.setattr(_ffi, "require_gpu", touched)
    monkeypatch.setattr(_ffi, "lib", touched)
    x = torch.zeros(2, 1, 8, 12, 16)
    w = torch.zeros(2, 2, 3, 4)
    with pytest.raises(ValueError, match=r"\(2, 3, 3, 4\)"):
        A.anomaly_map(x, x, torch.zeros(2, 3, 3, 4), sigma=1.0)
    with pytest.raises(ValueError, match="sigma"):
        A.anomaly_map(x, x, w, sigma=9)
    with pytest.raises(ValueError, match="hist_max"):
        A.anomaly_map(x, x, w, sigma=1, hist_max=0)
    with pytest.raises(ValueError, match="residual"):
        A.anomaly_map(x, x, w, sigma=1, residual="both")
    with pytest.raises(ValueError, match="reconstruction"):
        A.anomaly_map(x, torch.zeros(2, 1, 8, 12, 15), w, sigma=1)
    with pytest.raises(ValueError, match="labels"):
        A.anomaly_map(x, x, w, sigma=1, labels=torch.zeros(2, 1, 8, 12, 15))
    with pytest.raises(ValueError, match="volumes"):
        A.anomaly_map(torch.zeros(2, 2, 8, 12, 16), torch.zeros(2, 2, 8, 12, 16), w, sigma=1)
    with pytest.raises(AssertionError, match="the device was reached"):      # a valid call goes on to the device
        A.anomaly_map(x, x, w, sigma=1)


def _brute_scores(values, labels):
    """Dice per edge, best Dice and AP straight from the binned values"""
    dice, prec, rec = [], [], []
    n1 = int(labels.sum())
    for k in range(256):
        pred = values >= k
        tp, fp, fn = int((pred & labels).sum()), int((pred & ~labels).sum()), int((~pred & labels).sum())
        dice.append(2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0)
        prec.append(tp / (tp + fp) if tp + fp else 0.0)
        rec.append(tp / n1 if n1 else 0.0)
    ap, last = 0.0, 0.0
    for k in range(255, -1, -1):
        ap += (rec[k] - last) * prec[k]
        last = rec[k]
    return np.array(dice), ap


def test_the_histogram_scores_against_a_brute_force_over_the_binned_values():
    rng = np.random.default_rng(1)
    for trial in range(4):
        n = 3000
        labels = rng.random(n) < (0.1 + 0.2 * trial)
        a = (rng.random(n) ** 3 * (0.3 + 0.9 * labels)).astype(np.float32)      # labelled voxels score higher; some values pass hist_max = 1
        inv_bin = np.float32(256.0 / (1.0 if trial < 3 else 0.25))
        b = anomaly_ref.bins(a, inv_bin)
        assert b.min() >= 0 and b.max() <= 255 and (trial < 3 or (b == 255).sum() > 10)
        hist = anomaly_ref.histograms(a, labels, inv_bin)
        assert hist.sum() == n and hist[1].sum() == labels.sum()
        dice, ap = _brute_scores(b, labels)
        assert np.allclose(A.dice_per_edge(hist[0], hist[1]), dice, rtol=1e-14, atol=0)
        best, thr = A.best_dice(hist[0], hist[1], inv_bin)
        k = int(np.argmax(dice))
        assert best == pytest.approx(dice[k], rel=1e-14) and thr == k / float(inv_bin)
        assert A.average_precision(hist[0], hist[1]) == pytest.approx(ap, rel=1e-12)
        assert 0.0 < ap <= 1.0
    # a perfect separation scores 1, no labelled voxel gives NaN for AP and 0 for Dice
    h0, h1 = np.zeros(256, dtype=np.int64), np.zeros(256, dtype=np.int64)
    h0[:10] = 5
    h1[200:] = 2
    assert A.average_precision(h0, h1) == 1.0 and A.best_dice(h0, h1, 256.0) == (1.0, 10 / 256.0)
    assert math.isnan(A.average_precision(h0, np.zeros(256))) and A.best_dice(h0, np.zeros(256), 256.0)[0] == 0.0
    assert A.dice_from_counts(3, 1, 1) == 0.75 and A.dice_from_counts(0, 0, 0) == 0.0
    assert np.array_equal(A.bin_edges(512.0), np.arange(256) / 512.0)


def test_healing_outputs_are_matched_by_stem(tmp_path):
    import run_transformer as RT
    out = str(tmp_path / "outputs") + "/"
    grid = np.zeros((2, 2, 2))
    for stem in ("s0", "s1", "s10"):
        RT.save_healing(grid, grid, grid, out, f"/codes/{stem}_quantization_0.npy")
    subjects = ["/data/s0.nii.gz", "/data/s1.npy", "/data/s10.nii"]
    recs = AS.find_healing_outputs(subjects, out)
    assert [os.path.relpath(r["healed"], out) for r in recs] == [f"{s}_quantization_0/{s}_quantization_0_healed_sample.npy" for s in ("s0", "s1", "s10")]
    assert all(r["resampled"].endswith("_quantization_0_resampled.npy") and r["nll"].endswith("_quantization_0_nll.npy") for r in recs)
    assert AS.find_healing_outputs(subjects, out + "*/*.npy") == recs      # a glob
    with pytest.raises(ValueError, match=r"s2\.npy.*s2_quantization_0_healed_sample\.npy"):
        AS.find_healing_outputs(subjects + ["/data/s2.npy"], out)
    # a second copy elsewhere under the directory: ambiguous
    RT.save_healing(grid, grid, grid, out + "again/", "/codes/s1_quantization_0.npy")
    with pytest.raises(ValueError, match=r"/data/s1\.npy: 2 healing outputs"):
        AS.find_healing_outputs(subjects, out)
    assert len(AS.find_healing_outputs(subjects, out + "s*_quantization_0")) == 3      # narrowed again
    os.remove(recs[0]["nll"])
    with pytest.raises(ValueError, match=r"s0\.nii\.gz.*s0_quantization_0_nll\.npy"):
        AS.find_healing_outputs(subjects[:1], out + "s*_quantization_0", weight="nll")
    assert AS.find_healing_outputs(subjects[:1], out + "s*_quantization_0", weight="mask")[0] == recs[0]
    assert AS.find_healing_outputs(subjects[:1], out + "s*_quantization_0", weight="none")[0] == recs[0]


def test_labels_are_matched_by_stem(tmp_path):
    for name in ("s0.npy", "s1.nii.gz", "s10.npy"):
        (tmp_path / name).write_bytes(b"")
    subjects = ["/data/s1.npy", "/data/s0.nii"]
    assert AS.match_labels(subjects, str(tmp_path)) == [str(tmp_path / "s1.nii.gz"), str(tmp_path / "s0.npy")]
    with pytest.raises(ValueError, match=r"/data/s2\.npy: 0 label volumes"):
        AS.match_labels(["/data/s2.npy"], str(tmp_path))
    (tmp_path / "s0.nii").write_bytes(b"")
    with pytest.raises(ValueError, match=r"/data/s0\.nii: 2 label volumes"):
        AS.match_labels(subjects, str(tmp_path))


class _DeviceTouched(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    from synthanatomy_amd.runtime import ddp

    def touched():
        raise _DeviceTouched()
    monkeypatch.setattr(ddp, "init_distributed", touched)
    monkeypatch.setattr(torch.cuda, "is_available", touched)


def _argv(tmp_path, *extra):
    return ["run", "--training_subjects=synthetic:2", "--validation_subjects=synthetic:2", f"--project_directory={tmp_path}/", "--experiment_name=e",
            "--mode=anomaly", *extra]


def test_the_new_flags_their_defaults_and_a_full_command_line(tmp_path):
    from synthanatomy_amd.utils.general import parse_flags
    D = RV.DEFAULTS
    assert (D["anomaly_codes"], D["anomaly_weight"], D["anomaly_sigma"], D["anomaly_residual"], D["anomaly_threshold"], D["anomaly_hist_max"],
            D["anomaly_labels"]) == (None, "mask", None, "abs", None, 1.0, None)
    assert D["mode"] == "training" and D["output_ext"] == ".npy" and D["output_dtype"] == "float32"      # nothing else moved
    cfg = parse_flags(_argv(tmp_path, "--anomaly_codes=/h/outputs", "--anomaly_weight=nll", "--anomaly_sigma=2.5", "--anomaly_residual=positive",
                            "--anomaly_threshold=0.125", "--anomaly_hist_max=0.5", "--anomaly_labels=/labels/*.nii.gz", "--output_ext=.nii.gz"), D)
    assert (cfg["mode"], cfg["anomaly_codes"], cfg["anomaly_weight"], cfg["anomaly_sigma"], cfg["anomaly_residual"], cfg["anomaly_threshold"],
            cfg["anomaly_hist_max"], cfg["anomaly_labels"], cfg["output_ext"]) == ("anomaly", "/h/outputs", "nll", 2.5, "positive", 0.125, 0.5,
                                                                                   "/labels/*.nii.gz", ".nii.gz")
    RV._check_output_flags(cfg)
    AS._check_anomaly_flags(cfg)
    # None: half the down-sampling factor of the network the flags describe
    assert AS._anomaly_sigma(parse_flags(_argv(tmp_path), D)) == 4.0
    assert AS._anomaly_sigma(parse_flags(_argv(tmp_path, "--no_levels=2", "--downsample_parameters=((4,2,1,1),(4,2,1,1))"), D)) == 2.0
    assert AS._anomaly_sigma(cfg) == 2.5


@pytest.mark.parametrize("flag, value", [("anomaly_weight", "both"), ("anomaly_weight", "None"), ("anomaly_sigma", "-1"), ("anomaly_sigma", "8.5"),
                                         ("anomaly_sigma", "wide"), ("anomaly_sigma", "True"), ("anomaly_residual", "squared"),
                                         ("anomaly_threshold", "high"), ("anomaly_threshold", "(1,2)"), ("anomaly_hist_max", "0"),
                                         ("anomaly_hist_max", "-2"), ("anomaly_hist_max", "None"), ("anomaly_codes", "7"),
                                         ("no_augmented_extractions", "2")])
def test_a_bad_flag_is_refused_by_name_before_the_device(tmp_path, no_device, flag, value):
    with pytest.raises(ValueError, match="--" + flag):
        RV.run(_argv(tmp_path, f"--{flag}={value}"))
    assert not os.path.exists(tmp_path / "e")


def test_a_default_sigma_beyond_the_range_is_refused_and_valid_flags_go_on(tmp_path, no_device):
    with pytest.raises(ValueError, match="--anomaly_sigma=16"):      # five stride-2 levels: 32 / 2
        RV.run(_argv(tmp_path, "--no_levels=5", "--downsample_parameters=" + "((4,2,1,1),(4,2,1,1),(4,2,1,1),(4,2,1,1),(4,2,1,1))"))
    for extra in ((), ("--anomaly_weight=none", "--anomaly_sigma=0"), ("--anomaly_sigma=8", "--anomaly_threshold=0.1", "--anomaly_labels=/l")):
        with pytest.raises(_DeviceTouched):
            RV.run(_argv(tmp_path, *extra))


def test_the_other_modes_ignore_the_flags_and_an_unknown_mode_lists_the_new_one(tmp_path, no_device):
    with pytest.raises(_DeviceTouched):
        RV.run(_argv(tmp_path, "--anomaly_weight=both")[:-2] + ["--mode=extracting", "--anomaly_weight=both"])
    with pytest.raises(ValueError, match=r"bogus.*\['training', 'extracting', 'decoding', 'anomaly'\]"):
        RV.run(_argv(tmp_path)[:-1] + ["--mode=bogus"])


def test_the_library_exports_the_entry_point_and_its_workspace_query():
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    assert hasattr(lib, "sa_anomaly_map") and hasattr(lib, "sa_anomaly_map_workspace_bytes")
    assert ctypes.sizeof(_ffi.AnomalyParams) == 244 and _ffi.AnomalyParams.taps.offset == 48      # sa_anomaly_params
    assert _ffi.ANOMALY_RESULT_WORDS == 8 + 2 * 256 and 2 * _ffi.ANOMALY_MAX_R + 1 == 49
    # the workspace query runs on the host: eight 64-bit words per block of 16 x 8 x 32 voxels, and its refusals
    q = lib.sa_anomaly_map_workspace_bytes
    q.restype, q.argtypes = ctypes.c_int64, [ctypes.POINTER(_ffi.AnomalyParams)]
    P = _ffi.AnomalyParams(B=2, D=24, H=40, W=16, d=3, h=5, w=2, residual=0, R=12, has_threshold=0, inv_bin=256.0, threshold=0.0)
    assert q(ctypes.byref(P)) == 2 * (2 * 5 * 1) * 64
    for field, bad in (("d", 5), ("R", 25), ("R", -1), ("residual", 3), ("inv_bin", 0.0), ("B", 0), ("W", 0)):
        Q = _ffi.AnomalyParams.from_buffer_copy(P)
        setattr(Q, field, bad)
        assert q(ctypes.byref(Q)) == _ffi.SA_EINVAL, field
    assert anomaly_bounds.chain_length((24, 40, 16), (3, 5, 2), 12) == 1 + 3 * (8 - 1) + 3 + 5 + 2
    assert anomaly_bounds.chain_length((24, 40, 16), None, 0) == 0
