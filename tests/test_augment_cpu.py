"""CPU: the host half of the training augmentations (synthanatomy_amd.utils.vqvae.draw_augmentation and its helpers): what fires at
probability 0 and 1, the ranges of reference src/utils/vqvae.py:257-357, the (seed, epoch, subject) keying, the affine composition, the flip / rot90
composition into one signed permutation, the --patch_size rule, the new CLI switch, and the Box-Muller restatement of tests/augment_ref.py."""
import itertools

import numpy as np
import pytest

import augment_ref
from dropout_ref import philox4x32_10

DIMS = (20, 24, 18)


def _cfg(**kw):
    return dict(dict(augmentation=True, augmentation_probability=0.2, augmentation_strength=0, patch_size=None, no_augmented_extractions=0, seed=4), **kw)


def test_probability_zero_is_identity_with_every_intensity_bit_off():
    from synthanatomy_amd.utils.vqvae import AUG_IDENTITY, draw_augmentation
    for patch in (None, (8, 8, 8)):
        for subject in range(50):
            r = draw_augmentation(_cfg(augmentation_probability=0, patch_size=patch), "training", 4, 1, subject, DIMS)
            assert r["mode"] == AUG_IDENTITY and r["flags"] == 0
            if patch is None:
                assert list(r["off"]) == [0, 0, 0] and list(r["ext"]) == list(DIMS)
            else:
                assert all(0 <= o <= n - 8 for o, n in zip(r["off"], DIMS))


@pytest.mark.parametrize("strength", [0, 3])
def test_probability_one_fires_everything_inside_the_ranges(strength):
    from synthanatomy_amd.utils.vqvae import (AUG_AFFINE, AUG_CLAMP, AUG_GAMMA, AUG_NOISE, AUG_SHIFT, AUG_SIGNED_PERM, AugmentationStrengthScalers,
                                              augmentation_ranges, draw_augmentation)
    S = AugmentationStrengthScalers
    assert (S.AFFINEROTATE.value, S.AFFINETRANSLATE.value, S.AFFINESCALE.value, S.ADJUSTCONTRASTGAMMA.value, S.SHIFTINTENSITYOFFSET.value,
            S.GAUSSIANNOISESTD.value) == (0.2, 1, 0.01, 0.01, 0.025, 0.01)
    rot, tr, sc = 0.04 + 0.2 * strength, 2 + int(round(strength)), 0.05 + 0.01 * strength      # reference src/utils/vqvae.py:292-315
    g_lo, g_hi, sh, sd = 0.99 - 0.01 * strength, 1.01 + 0.01 * strength, 0.05 + 0.025 * strength, 0.02 + 0.01 * strength      # :330-355
    rg = augmentation_ranges(strength)
    assert (rg["rotate"], rg["translate"], rg["scale"], rg["gamma"], rg["shift"], rg["noise_std"]) == (rot, tr, sc, (g_lo, g_hi), sh, sd)
    seen = set()
    for subject in range(200):
        r = draw_augmentation(_cfg(augmentation_probability=1, augmentation_strength=strength), "training", 4, 0, subject, DIMS)
        assert r["mode"] == AUG_AFFINE and r["flags"] == AUG_GAMMA | AUG_SHIFT | AUG_NOISE | AUG_CLAMP
        assert g_lo - 1e-6 <= r["gamma"] <= g_hi + 1e-6 and 0 <= r["shift"] <= sh + 1e-7 and 0 <= r["noise_std"] <= sd + 1e-7
        M = r["M"].astype(np.float64).reshape(3, 4)
        scales = np.linalg.norm(M[:, :3], axis=0)               # columns of R diag(s)
        assert np.all(scales >= 1 - sc - 1e-6) and np.all(scales <= 1 + sc + 1e-6)
        R = M[:, :3] / scales
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-5)
        t = R.T @ M[:, 3]                                       # M[:, 3] = R t
        assert np.all(np.abs(t) <= tr + 1e-4)
        # Rx(r0) Ry(r1) Rz(r2): R[0, 2] = sin r1, and the other two angles from the first row / last column
        r1 = np.arcsin(R[0, 2])
        r0, r2 = np.arctan2(-R[1, 2], R[2, 2]), np.arctan2(-R[0, 1], R[0, 0])
        assert max(abs(r0), abs(r1), abs(r2)) <= rot + 1e-5
        seen.add(float(r["gamma"]))
        p = draw_augmentation(_cfg(augmentation_probability=1, augmentation_strength=strength, patch_size=(8, 8, 8)), "training", 4, 0, subject, DIMS)
        assert p["mode"] == AUG_SIGNED_PERM and p["flags"] == AUG_GAMMA | AUG_SHIFT | AUG_NOISE | AUG_CLAMP
        assert sorted(p["perm"]) == [0, 1, 2] and all(abs(s) == 1 for s in p["sign"])
        assert all(0 <= o <= n - 8 for o, n in zip(p["off"], DIMS)) and list(p["ext"]) == [8, 8, 8]
    assert len(seen) > 150


def test_draws_are_keyed_on_seed_epoch_subject_only():
    from synthanatomy_amd.utils.vqvae import draw_augmentation
    cfg = _cfg(augmentation_probability=1, augmentation_strength=1)
    keys = [(4, 0, 0), (5, 0, 0), (4, 1, 0), (4, 0, 1), (4, 2, 7)]
    first = {k: draw_augmentation(cfg, "training", *k, DIMS) for k in keys}
    again = {k: draw_augmentation(cfg, "training", *k, DIMS) for k in reversed(keys)}      # another call order
    for k in keys:
        assert first[k].tobytes() == again[k].tobytes()
    for a, b in itertools.combinations(keys, 2):
        assert first[a].tobytes() != first[b].tobytes(), (a, b)
    # the switch: without --augmentation training draws nothing but the crop, and extraction augments once no_augmented_extractions is set
    from synthanatomy_amd.utils.vqvae import AUG_IDENTITY
    off = draw_augmentation(dict(cfg, augmentation=False, patch_size=(8, 8, 8)), "training", 4, 0, 0, DIMS)
    assert off["mode"] == AUG_IDENTITY and off["flags"] == 0
    assert list(off["off"]) == list(draw_augmentation(dict(cfg, patch_size=(8, 8, 8)), "training", 4, 0, 0, DIMS)["off"])
    assert draw_augmentation(dict(cfg, augmentation=False), "extracting", 4, 0, 0, DIMS)["flags"] == 0
    assert draw_augmentation(dict(cfg, augmentation=False, no_augmented_extractions=2), "extracting", 4, 0, 0, DIMS)["flags"] != 0


def test_affine_matrix_is_rotate_translate_scale_in_fp64():
    from synthanatomy_amd.utils.vqvae import affine_matrix
    r, t, s = (0.03, -0.11, 0.2), (1.5, -2.0, 0.25), (1.04, 0.97, 1.01)
    c, sn = np.cos, np.sin
    Rx = np.array([[1, 0, 0, 0], [0, c(r[0]), -sn(r[0]), 0], [0, sn(r[0]), c(r[0]), 0], [0, 0, 0, 1.0]])
    Ry = np.array([[c(r[1]), 0, sn(r[1]), 0], [0, 1, 0, 0], [-sn(r[1]), 0, c(r[1]), 0], [0, 0, 0, 1.0]])
    Rz = np.array([[c(r[2]), -sn(r[2]), 0, 0], [sn(r[2]), c(r[2]), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    T = np.eye(4)
    T[:3, 3] = t
    S = np.diag([*s, 1.0])
    want = (Rx @ Ry @ Rz @ T @ S)[:3]
    got = affine_matrix(r, t, s)
    assert got.dtype == np.float64 and got.shape == (3, 4)
    assert np.abs(got - want).max() < 1e-15
    assert np.array_equal(affine_matrix((0, 0, 0), (0, 0, 0), (1, 1, 1)), np.eye(3, 4))


def test_flip_and_rot90_compose_into_one_signed_permutation():
    from synthanatomy_amd.utils.vqvae import compose_signed_perm
    cube = np.arange(27, dtype=np.float64).reshape(3, 3, 3)
    n = 0
    for flips in itertools.product((False, True), repeat=3):
        for ks in itertools.product(range(4), repeat=3):
            want = cube
            for a in range(3):
                if flips[a]:
                    want = np.flip(want, a)
            for k, axes in zip(ks, ((0, 1), (1, 2), (0, 2))):
                want = np.rot90(want, k, axes)
            perm, sign = compose_signed_perm(flips, ks)
            assert np.array_equal(augment_ref.signed_perm(cube, (0, 0, 0), perm, sign, (3, 3, 3)), want), (flips, ks)
            n += 1
    assert n == 2 ** 3 * 4 ** 3


def test_unequal_patch_sides_raise_where_a_rot90_is_reachable():
    from synthanatomy_amd.utils.vqvae import draw_augmentation
    with pytest.raises(ValueError, match="patch_size"):
        draw_augmentation(_cfg(patch_size=(8, 8, 6)), "training", 4, 0, 0, DIMS)
    # not reachable: no augmentation, or probability 0 -- the crop alone works
    r = draw_augmentation(_cfg(patch_size=(8, 8, 6), augmentation=False), "training", 4, 0, 0, DIMS)
    assert list(r["ext"]) == [8, 8, 6]
    assert list(draw_augmentation(_cfg(patch_size=(8, 8, 6), augmentation_probability=0), "training", 4, 0, 0, DIMS)["ext"]) == [8, 8, 6]
    with pytest.raises(ValueError, match="patch_size"):
        draw_augmentation(_cfg(patch_size=(8, 8, 32), augmentation_probability=0), "training", 4, 0, 0, DIMS)      # larger than the volume


def test_roi_window_and_symmetric_padding():
    from synthanatomy_amd.utils.vqvae import pad_to_roi, roi_window
    assert roi_window((8, 8, 6), (12, 11, 6)) == ([2, 1, 0], [8, 8, 6])                       # CenterSpatialCropd: n // 2 - r // 2
    assert roi_window(((1, 9), (0, 8), (2, 8)), (12, 11, 9)) == ([1, 0, 2], [8, 8, 6])        # SpatialCropd
    assert roi_window(((1, 9), (0, 8), (2, 8)), (12, 11, 5)) == ([1, 0, 2], [8, 8, 3])        # clipped: pad_to_roi follows
    v = np.arange(2 * 3 * 3, dtype=np.float32).reshape(1, 2, 3, 3)
    p = pad_to_roi(v, (5, 3, 4))
    assert p.shape == (1, 5, 3, 4)
    assert np.array_equal(p, np.pad(v, [(0, 0), (1, 2), (0, 0), (0, 1)], mode="symmetric"))
    assert pad_to_roi(v, (2, 3, 3)) is v


def test_file_inputs_get_the_roi_as_a_window_or_a_host_pad(tmp_path):
    import torch

    import run_vqvae
    rng = np.random.default_rng(3)
    big, small = rng.random((12, 11, 9)).astype(np.float32) * 7 - 2, rng.random((6, 11, 5)).astype(np.float32)
    np.save(tmp_path / "big.npy", big)
    np.save(tmp_path / "small.npy", small)
    cfg = dict(run_vqvae.DEFAULTS, roi=((1, 9), (0, 8), (2, 8)), normalize=True, seed=4)
    dev = torch.device("cpu")
    v, start = run_vqvae._load_input(str(tmp_path / "big.npy"), cfg, dev)
    assert start == [1, 0, 2] and v.shape == (1, 12, 11, 9)                      # the kernel crops: the record's window starts here
    assert torch.equal(v, run_vqvae._load_volume(str(tmp_path / "big.npy"), cfg, None, dev)) and float(v.min()) == 0.0
    v, start = run_vqvae._load_input(str(tmp_path / "small.npy"), cfg, dev)      # shorter than the ROI along D and W: cropped, then mirror-padded
    assert start == [0, 0, 0] and v.shape == (1, 8, 8, 6)
    norm = run_vqvae._read_volume(str(tmp_path / "small.npy"), cfg).numpy()
    assert np.array_equal(v.numpy(), np.pad(norm[:, 1:6, 0:8, 2:5], [(0, 0), (1, 2), (0, 0), (1, 2)], mode="symmetric"))
    v, start = run_vqvae._load_input(str(tmp_path / "big.npy"), dict(cfg, roi=(8, 8, 6)), dev)
    assert start == [2, 1, 1] and v.shape == (1, 12, 11, 9)                      # three ints: the centre crop


def test_cli_switch_defaults_to_off():
    import run_vqvae
    from synthanatomy_amd.utils.general import parse_flags
    assert run_vqvae.DEFAULTS["augmentation"] is False and run_vqvae.DEFAULTS["augmentation_probability"] == 0.2
    base = ["--training_subjects=synthetic:2", "--validation_subjects=synthetic:1", "--project_directory=/p/", "--experiment_name=e"]
    assert parse_flags(base, run_vqvae.DEFAULTS)["augmentation"] is False
    cfg = parse_flags(base + ["--augmentation=True", "--patch_size=(16,16,16)", "--no_augmented_extractions=2"], run_vqvae.DEFAULTS)
    assert cfg["augmentation"] is True and cfg["patch_size"] == (16, 16, 16) and cfg["no_augmented_extractions"] == 2
    assert run_vqvae._augmented_name("/a/b/vol.npy", 1) == "/a/b/vol_1.npy" and run_vqvae._augmented_name("synthetic_0003", 0) == "synthetic_0003_0"
    assert run_vqvae._noise_seed(4, 1) != run_vqvae._noise_seed(4, 2) != run_vqvae._noise_seed(5, 2) and 0 <= run_vqvae._noise_seed(4, 1) < 2 ** 64


def test_box_muller_restatement():
    # the ends of the word range: finite in both precisions (u = 2^-25 and, after float32 rounding, 1)
    for dt in (np.float64, np.float32):
        for w0, w1 in itertools.product((0, 0xFFFFFFFF), repeat=2):
            a, b = augment_ref.box_muller(np.array([w0], dtype=np.uint64), np.array([w1], dtype=np.uint64), dt)
            assert np.isfinite(a).all() and np.isfinite(b).all()
    assert augment_ref.uniform32([0])[0] == np.float32(2.0 ** -25) and augment_ref.uniform32([0xFFFFFFFF])[0] <= 1.0
    # the indexing: voxel e reads word pair (e & 3) >> 1 of block e >> 2, cosine for even e
    seed, sample = 0x0123456789ABCDEF, 3
    w = philox4x32_10((5, 0, sample, 0), (seed & 0xFFFFFFFF, seed >> 32))
    n = augment_ref.normals(seed, sample, 20, 4)
    for k in range(4):
        u0, u1 = ((w[k & 2] >> 8) + 0.5) * 2.0 ** -24, ((w[(k & 2) + 1] >> 8) + 0.5) * 2.0 ** -24
        want = np.sqrt(-2 * np.log(u0)) * (np.cos if k % 2 == 0 else np.sin)(2 * np.pi * u1)
        assert abs(n[k] - want) < 1e-14
    assert np.array_equal(augment_ref.normals(seed, sample, 0, 40)[3:], augment_ref.normals(seed, sample, 3, 37))      # a window that starts inside a group
    # moments over 40 000 draws: mean within 4 sigma (1 / sqrt N) of 0, variance within 4 sigma (sqrt(2 / N)) of 1
    N = 40000
    z = augment_ref.normals(99, 0, 0, N)
    assert abs(z.mean()) < 4 / np.sqrt(N) and abs(z.var() - 1) < 4 * np.sqrt(2 / N)
    z32 = augment_ref.normals(99, 0, 0, N, np.float32)
    assert z32.dtype == np.float32 and np.abs(z32 - z).max() < 1e-5
