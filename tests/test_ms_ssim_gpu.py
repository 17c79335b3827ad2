"""GPU: ``sa_ms_ssim`` (csrc/metrics.hip) against the fp64 restatement of tests/ms_ssim_ref.py on structured volumes, with witnesses that show the
gate sees a dropped odd-side padding and a wrong sigma; bitwise exactness (X vs X, repeated calls, a volume alone vs inside a batch); the refusals;
and MAE / MSE from ``sa_baur_loss`` against torch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ms_ssim_ref as R
from synthanatomy_amd.metrics import _ms_ssim, ms_ssim
from synthanatomy_amd.metrics.vqvae import MAE, MSE, MultiScaleSSIM

pytestmark = pytest.mark.gpu


def _blur(v, k):
    """separable k^3 box filter, replicate padding"""
    v = F.pad(v, (k // 2,) * 6, mode="replicate")
    for ks in ((k, 1, 1), (1, k, 1), (1, 1, k)):
        v = F.avg_pool3d(v, kernel_size=ks, stride=1)
    return v


def _volumes(shape, seed):
    """Smoothed blobs plus noise; y is a blurred, noised copy of x (values spread between about 0.3 and 0.99)."""
    g = torch.Generator().manual_seed(seed)
    B, C = shape[:2]
    base = torch.rand(B * C, 1, *shape[2:], generator=g)
    x = _blur(_blur(base, 7), 5)
    x = (x - x.amin()) / (x.amax() - x.amin())
    x = (x + 0.05 * torch.randn(x.shape, generator=g)).clamp(0, 1)
    noise = torch.linspace(0.02, 0.25, B * C).view(-1, 1, 1, 1, 1)
    y = (_blur(x, 3) + noise * torch.randn(x.shape, generator=g)).clamp(0, 1)
    return x.reshape(shape).contiguous(), y.reshape(shape).contiguous()


def _tolerance(ref_vals, torch_vals):
    """per value: max(2 |torch fp32 on the GPU - fp64 restatement|, 1e-5)"""
    return np.maximum(2 * np.abs(torch_vals - ref_vals), 1e-5)


CASES = [((2, 1, 160, 224, 160), 5), ((3, 2, 49, 67, 53), 3), ((1, 1, 177, 177, 177), 11)]


@pytest.mark.parametrize("shape,w", CASES, ids=["roi160x224x160_w5", "ragged49x67x53_w3", "cube177_w11"])
def test_hip_matches_the_fp64_restatement(shape, w):
    x, y = _volumes(shape, seed=shape[2])
    xd, yd = x.cuda(), y.cuda()
    out, lm = _ms_ssim(xd, yd, data_range=1, win_size=w, level_means=True)
    got = np.concatenate([out.cpu().double().numpy(), lm.cpu().double().numpy().ravel()])
    lv_t = []
    tv = R.torch_ms_ssim(xd, yd, win_size=w, levels_out=lv_t)
    tvals = np.concatenate([tv.cpu().double().numpy(), torch.stack(lv_t).cpu().double().numpy().ravel()])

    def ref(**kw):
        lv = []
        v = R.ms_ssim(x.numpy(), y.numpy(), win_size=w, levels_out=lv, **kw)
        return np.concatenate([v, np.stack(lv).ravel()])

    r = ref()
    assert 0.2 <= r[:shape[0]].min() and r[:shape[0]].max() <= 0.999, r[:shape[0]]
    tol = _tolerance(r, tvals)
    ok = np.abs(got - r) <= tol
    assert ok.all(), (np.abs(got - r).max(), got[~ok], r[~ok], tvals[~ok])
    # witnesses: the same gate (these tolerances) must fail against a restatement with a planted mistake
    assert not (np.abs(got - ref(win_sigma=1.4)) <= tol).all()
    if any(s % 2 for s in shape[2:]):
        assert not (np.abs(got - ref(odd_padding=False)) <= tol).all()


def test_identical_inputs_give_exactly_one():
    x, _ = _volumes((2, 2, 49, 67, 53), seed=1)
    xd = x.cuda()
    v = ms_ssim(xd, xd.clone(), data_range=1, size_average=False, win_size=3)
    assert torch.equal(v.cpu(), torch.ones(2))
    assert ms_ssim(xd, xd, data_range=1, win_size=3).item() == 1.0


def test_bitwise_reproducible_and_independent_of_the_batch():
    x, y = _volumes((3, 2, 49, 67, 53), seed=2)
    xd, yd = x.cuda(), y.cuda()
    a, la = _ms_ssim(xd, yd, data_range=1, win_size=3, level_means=True)
    b, lb = _ms_ssim(xd, yd, data_range=1, win_size=3, level_means=True)
    assert torch.equal(a, b) and torch.equal(la, lb)
    for i in range(3):
        s, ls = _ms_ssim(xd[i:i + 1], yd[i:i + 1], data_range=1, win_size=3, level_means=True)
        assert torch.equal(s[0], a[i]) and torch.equal(ls[:, 0], la[:, i])
    big_x = torch.cat([xd, torch.flip(xd, [0]), xd[:1]], 0)           # same volume among others, at another batch index
    big_y = torch.cat([yd, torch.flip(yd, [0]), yd[:1]], 0)
    c = _ms_ssim(big_x, big_y, data_range=1, win_size=3)
    assert torch.equal(c[:3], a) and torch.equal(c[3], a[2]) and torch.equal(c[6], a[0])


def test_refusals():
    x = torch.rand(1, 1, 40, 40, 40, device="cuda")
    with pytest.raises(ValueError, match="same dimensions"):
        ms_ssim(x, x[..., :39], data_range=1, win_size=3)
    with pytest.raises(ValueError, match="odd"):
        ms_ssim(x, x, data_range=1, win_size=4)
    with pytest.raises(AssertionError):
        ms_ssim(x[..., :32], x[..., :32], data_range=1, win_size=3)
    with pytest.raises(ValueError):
        ms_ssim(x[0], x[0], data_range=1, win_size=3)                   # 4-D: the 2-D path is out of scope
    with pytest.raises(ValueError):
        ms_ssim(x[:, :, :8], x[:, :, :8], data_range=1, win_size=3)     # level 4's D side (1) shorter than the window
    from synthanatomy_amd import _ffi
    lib = _ffi.lib()
    assert lib.sa_ms_ssim_workspace_bytes(1, 1, 40, 40, 40, 4, 5) == _ffi.SA_EINVAL
    assert lib.sa_ms_ssim_workspace_bytes(1, 1, 40, 40, 32, 3, 5) == _ffi.SA_EINVAL
    assert lib.sa_ms_ssim_workspace_bytes(1, 1, 40, 40, 40, 3, 5) > 0


def test_mae_and_mse_match_torch():
    x, y = _volumes((2, 1, 48, 40, 56), seed=3)
    xd, yd = x.cuda(), y.cuda()
    mae, mse, ms = MAE(), MSE(), MultiScaleSSIM(ms_ssim_kwargs={"win_size": 3})
    for i in (slice(0, 1), slice(1, 2)):
        for m in (mae, mse, ms):
            m.update((yd[i], xd[i]))
    want1 = (F.l1_loss(yd[:1], xd[:1]).item() + F.l1_loss(yd[1:], xd[1:]).item()) / 2
    want2 = (F.mse_loss(yd[:1], xd[:1]).item() + F.mse_loss(yd[1:], xd[1:]).item()) / 2
    assert mae.compute() == pytest.approx(want1, rel=1e-5)
    assert mse.compute() == pytest.approx(want2, rel=1e-5)
    assert ms.compute() == pytest.approx(float(ms_ssim(xd, yd, data_range=1, win_size=3).item()), abs=1e-6)
