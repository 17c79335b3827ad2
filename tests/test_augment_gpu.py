"""GPU: ``sa_augment`` (csrc/augment.hip) against the restatement of tests/augment_ref.py.  The gathers (IDENTITY, SIGNED_PERM, an integer
AFFINE shift) are bit-exact; the AFFINE resample is held to a per-voxel bound the restatement derives from the fp32 coordinate and blend errors; the
intensity stage and the noise to four times what the same formulas lose in numpy float32 against fp64 (never below 2 eps32 (max - min)).  Shapes: nothing
divides a wave, a vector of four or a block, and the second sample of a batch starts off a 16-byte boundary."""
import numpy as np
import pytest
import torch

import augment_ref as ref
from augment_ref import CLAMP, EPS32, GAMMA, NOISE, SHIFT

pytestmark = pytest.mark.gpu

IN = (13, 10, 7)
SEED = 0x5EEDFACE12345678


def _rec(dims, off=(0, 0, 0), **kw):
    from synthanatomy_amd.utils.vqvae import identity_record
    r = identity_record(dims, off)
    for k, v in kw.items():
        r[k] = v
    return r


@pytest.fixture(scope="module")
def volume():
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.rand(3, 1, *IN, generator=g, device="cuda")
    return x, x.cpu().numpy()


def _run(x, recs, out_dims, seed=SEED, ws=False):
    from synthanatomy_amd.utils.vqvae import hip_augment
    return hip_augment(x, np.stack(recs), out_dims, seed, return_workspace=ws)


def _minmax(ws, b):
    word = int(ws[b, 2].item()) & 0xFFFFFFFFFFFFFFFF
    return np.array([word & 0xFFFFFFFF, word >> 32], dtype=np.uint32).view(np.float32)


def test_identity_copies_and_crops_bit_exact(volume):
    x, xn = volume
    assert torch.equal(_run(x, [_rec(IN)] * 3, IN), x)
    offs = [(0, 0, 0), (7, 4, 2), (3, 0, 1)]      # (7, 4, 2) is the last legal corner of a 6 x 6 x 5 crop
    y = _run(x, [_rec((6, 6, 5), o) for o in offs], (6, 6, 5)).cpu().numpy()
    for b, o in enumerate(offs):
        assert np.array_equal(y[b, 0], xn[b, 0, o[0]:o[0] + 6, o[1]:o[1] + 6, o[2]:o[2] + 5])


@pytest.mark.parametrize("cases", [
    [((True, False, True), (0, 0, 0), "zero"), ((False, False, False), (1, 0, 0), "last"), ((False, False, False), (3, 0, 0), "mixed")],
    [((True, True, True), (1, 2, 3), "last"), ((False, True, False), (0, 1, 0), "zero"), ((True, True, True), (3, 1, 2), "mixed")],
], ids=["flip_rot01_k1_k3", "all_six"])
def test_signed_perm_equals_numpy_flip_rot90_of_the_crop(volume, cases):
    from synthanatomy_amd.utils.vqvae import AUG_SIGNED_PERM, compose_signed_perm
    x, xn = volume
    out = (6, 6, 5)
    recs, want = [], []
    for b, (flips, ks, where) in enumerate(cases):
        perm, sign = compose_signed_perm(flips, ks)
        src = [0, 0, 0]
        for a in range(3):
            src[perm[a]] = out[a]                                   # the crop's sides in source axes
        last = [n - s for n, s in zip(IN, src)]
        off = {"zero": [0, 0, 0], "last": last, "mixed": [last[0], 0, last[2] // 2]}[where]
        recs.append(_rec(src, off, mode=AUG_SIGNED_PERM, perm=perm, sign=sign))
        w = xn[b, 0, off[0]:off[0] + src[0], off[1]:off[1] + src[1], off[2]:off[2] + src[2]]
        for a in range(3):
            if flips[a]:
                w = np.flip(w, a)
        for k, axes in zip(ks, ((0, 1), (1, 2), (0, 2))):
            w = np.rot90(w, k, axes)
        assert w.shape == out
        want.append(w)
    y = _run(x, recs, out)
    assert torch.equal(y.cpu(), torch.from_numpy(np.stack(want)[:, None].copy()))


def _affine_A():
    from synthanatomy_amd.utils.vqvae import affine_matrix
    return affine_matrix((0.05, -0.03, 0.08), (0.7, -0.4, 0.3), (1.04, 0.97, 1.02)).astype(np.float32)


@pytest.fixture(scope="module")
def affine_truth(volume):
    """fp64 value and bound of sample A (computed once, shared)"""
    _, xn = volume
    return ref.affine(xn[0, 0], _affine_A(), IN)


def test_affine_rotation_zero_fill_and_integer_shift(volume, affine_truth):
    from synthanatomy_amd.utils.vqvae import AUG_AFFINE
    x, xn = volume
    far = np.eye(3, 4, dtype=np.float32)
    far[0, 3] = 40.0                                                # further than the volume is long: every corner outside
    shift = np.eye(3, 4, dtype=np.float32)
    shift[:, 3] = (1, 0, -2)
    y = _run(x, [_rec(IN, mode=AUG_AFFINE, M=m.reshape(-1)) for m in (_affine_A(), far, shift)], IN).cpu().numpy()
    val, bound = affine_truth
    err = np.abs(y[0, 0].astype(np.float64) - val)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"affine {IN}->{IN}: max |error| {err.max():.3e}, largest error / bound {ratio:.3f}")
    assert np.all(err <= bound)
    assert np.all(bound[np.abs(val) > 0] > 0) and float(np.abs(val).max()) > 0.5
    assert not y[1].any()
    want = np.zeros(IN, dtype=np.float32)
    want[:12, :, 2:] = xn[2, 0, 1:, :, :5]                         # y[o] = x[o + (1, 0, -2)] where that is inside
    assert np.array_equal(y[2, 0], want)


def test_affine_into_another_output_size(volume):
    from synthanatomy_amd.utils.vqvae import AUG_AFFINE
    x, xn = volume
    out = (8, 8, 6)
    y = _run(x, [_rec(IN, mode=AUG_AFFINE, M=_affine_A().reshape(-1))] * 3, out).cpu().numpy()
    for b in range(3):
        val, bound = ref.affine(xn[b, 0], _affine_A(), out)
        err = np.abs(y[b, 0].astype(np.float64) - val)
        print(f"affine {IN}->{out} sample {b}: largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert np.all(err <= bound)
    # a window inside the volume: positions are relative to it and everything outside counts as 0
    off, ext = (2, 1, 1), (9, 8, 5)
    y = _run(x, [_rec(ext, off, mode=AUG_AFFINE, M=_affine_A().reshape(-1))] * 3, out).cpu().numpy()
    val, bound = ref.affine(xn[1, 0], _affine_A(), out, off, ext)
    assert np.all(np.abs(y[1, 0].astype(np.float64) - val) <= bound)


def _allowed(truth, yard):
    """four times the yardstick's own largest error against fp64, not below 2 eps32 (max - min)"""
    return max(4.0 * float(np.abs(yard.astype(np.float64) - truth).max()), 2.0 * EPS32 * float(truth.max() - truth.min()))


@pytest.fixture(scope="module")
def intensity_volume():
    g = torch.Generator(device="cuda").manual_seed(12)
    x = torch.rand(2, 1, 9, 6, 5, generator=g, device="cuda")
    x[1] = x[1] * 1.7 - 0.3                                         # [-0.3, 1.4): min / max matter and the clamp bites
    return x, x.cpu().numpy()


@pytest.mark.parametrize("flags", [GAMMA, SHIFT, CLAMP, GAMMA | SHIFT | CLAMP], ids=["gamma", "shift", "clamp", "together"])
def test_gamma_shift_clamp_against_fp64(intensity_volume, flags):
    x, xn = intensity_volume
    dims = xn.shape[2:]
    gam, sh = (np.float32(0.7), np.float32(1.6)), (np.float32(0.0625 + 0.01), np.float32(0.21))
    y, ws = _run(x, [_rec(dims, flags=flags, gamma=gam[b], shift=sh[b]) for b in range(2)], dims, ws=True)
    y = y.cpu().numpy()
    for b in range(2):
        truth, mn, mx = ref.intensity(xn[b, 0], flags, float(gam[b]), float(sh[b]))
        yard, _, _ = ref.intensity(xn[b, 0], flags, gam[b], sh[b], dtype=np.float32)
        allowed = _allowed(truth, yard)
        err = float(np.abs(y[b, 0].astype(np.float64) - truth).max())
        print(f"intensity flags {flags} sample {b}: max |error| {err:.3e}, allowed {allowed:.3e}, ratio {err / allowed:.3f}")
        assert err <= allowed
        if flags & GAMMA:
            got = _minmax(ws, b)
            assert got[0] == xn[b, 0].min() and got[1] == xn[b, 0].max()
        if flags & CLAMP:
            assert y[b].min() >= 0 and y[b].max() <= 1
    if flags & CLAMP:
        assert (y[1] == 0).any() and (y[1] == 1).any()               # the clamp did bite on the [-0.3, 1.4) sample


@pytest.mark.parametrize("dims", [(9, 6, 5), (5, 3, 7)])
def test_noise_is_the_philox_box_muller_restatement(dims):
    n = int(np.prod(dims))
    assert n % 4 != 0 and dims[2] % 2 == 1                           # a partial last group; sample 1 starts off a 16-byte boundary; odd rows
    std = np.float32(0.05)
    x = torch.full((2, 1, *dims), 0.5, device="cuda")
    recs = [_rec(dims, flags=NOISE | CLAMP, noise_std=std)] * 2
    y = _run(x, recs, dims)
    assert torch.equal(_run(x, recs, dims), y)                       # the same seed: the same noise
    assert not torch.equal(_run(x, recs, dims, seed=SEED + 1), y)
    y = y.cpu().numpy().reshape(2, n)
    assert y.min() > 0 and y.max() < 1                               # |n| <= sqrt(-2 ln 2^-25) = 5.9: the clamp cannot act, and did not
    assert not np.array_equal(y[0], y[1])                            # the sample index is part of the counter
    for b in range(2):
        got = (y[b].astype(np.float64) - 0.5) / float(std)
        truth = ref.normals(SEED, b, 0, n)
        yard = ((np.float32(0.5) + std * ref.normals(SEED, b, 0, n, np.float32)).astype(np.float64) - 0.5) / float(std)
        allowed = _allowed(truth, yard)
        err = float(np.abs(got - truth).max())
        print(f"noise {dims} sample {b}: max |error| {err:.3e}, allowed {allowed:.3e}, ratio {err / allowed:.3f}")
        assert err <= allowed
        for start in (1, 2, 3, 5, n - 2):                            # a window that starts inside a group of four reads the same words
            assert np.abs(got[start:] - ref.normals(SEED, b, start, n - start)).max() <= allowed
    z = np.concatenate([(y[b].astype(np.float64) - 0.5) / float(std) for b in range(2)])
    assert abs(z.mean()) < 4 / np.sqrt(z.size) and abs(z.var() - 1) < 4 * np.sqrt(2 / z.size)


def test_all_stages_together_on_the_affine_sample(volume, affine_truth):
    """The spatial error enters the intensity stage; the gate is the sum of the three bounds: the affine per-voxel bound, the intensity allowance and the
    noise allowance scaled by the std."""
    from synthanatomy_amd.utils.vqvae import AUG_AFFINE
    x, _ = volume
    flags, gam, sh, std = GAMMA | SHIFT | NOISE | CLAMP, np.float32(1.2), np.float32(0.03), np.float32(0.02)
    rec = _rec(IN, mode=AUG_AFFINE, M=_affine_A().reshape(-1), flags=flags, gamma=gam, shift=sh, noise_std=std)
    y, ws = _run(x, [rec] * 3, IN, ws=True)
    y = y.cpu().numpy()
    val, bound = affine_truth
    n = int(np.prod(IN))
    nz = ref.normals(SEED, 0, 0, n)
    truth, mn, mx = ref.intensity(val, flags, float(gam), float(sh), float(std), nz)
    v32 = val.astype(np.float32)
    yard, _, _ = ref.intensity(v32, flags, gam, sh, std, ref.normals(SEED, 0, 0, n, np.float32), dtype=np.float32)
    exact32, _, _ = ref.intensity(v32, flags, float(gam), float(sh), float(std), nz)        # fp64 on the same rounded input: the yardstick's truth
    noise_allowed = _allowed(nz, ref.normals(SEED, 0, 0, n, np.float32))
    allowed = bound + _allowed(exact32, yard) + float(std) * noise_allowed
    err = np.abs(y[0, 0].astype(np.float64) - truth)
    print(f"all stages: max |error| {err.max():.3e}, largest error / allowed {float((err / allowed).max()):.3f}")
    assert np.all(err <= allowed)
    got = _minmax(ws, 0)
    assert abs(got[0] - mn) <= bound.max() and abs(got[1] - mx) <= bound.max()
    assert int(ws[:, 3].abs().sum().item()) == 0                     # every record was accepted


def test_a_broken_record_is_refused_on_the_host():
    from synthanatomy_amd.utils.vqvae import AUG_SIGNED_PERM
    x = torch.zeros(1, 1, 4, 4, 4, device="cuda")
    with pytest.raises(ValueError, match="does not fit"):
        _run(x, [_rec((4, 4, 4), (1, 0, 0))], (4, 4, 4))
    with pytest.raises(ValueError, match="does not fit"):
        _run(x, [_rec((4, 4, 4), mode=AUG_SIGNED_PERM, perm=(0, 0, 2))], (4, 4, 4))
