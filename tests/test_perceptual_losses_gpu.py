"""GPU: the 2.5D LPIPS-alex perceptual term on HIP (losses/lpips.py, csrc/lpips.hip) against the fp64 restatement of
tests/lpips_ref.py on the same kept slices -- real AlexNet widths, seeded stand-in weights.

fp32 mode is the parity contract: loss and per-view summaries |got - ref| <= 1e-3 |ref|, gradient max|got - ref| <= 1e-3 max|ref|.  bf16 mode is held to
the reference side only: with delta the discrepancy (same norms) between lpips_ref in fp64 and its own bf16 model on the case, the kernel must lie within
4 delta of the fp64 result; delta and the observed ratio are printed (run with -s).  Run with -s to read every figure.
"""
import functools
import glob
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(16, torch.get_num_threads()))
DEV = "cuda"
SEED, STEP = 11, 3
TOL = 1e-3
CASES = {
    # deep taps collapse to 1 x 1; sides 31 / 33 give conv1 output 7, side 35 gives 8: slice shapes of mixed output parity; 31 is the minimum side
    "A": dict(shape=(2, 1, 31, 33, 35), drop=0.0),
    # ~44 kept slices with 3 x 3 deep taps; side 77 -> conv1 output 18 -> pool 8 -> the second pool's floor drops a column
    "B": dict(shape=(1, 1, 31, 70, 77), drop=0.75),
}


def _weights(seed=0):
    return lpips_ref.draw_weights(seed)


def _ids(shape, drop, seed=SEED, step=STEP):
    B, _, D, H, W = shape
    return [lpips_ref.draw_slices(seed, step, v, B * n, int(B * n * (1 - drop))) for v, n in enumerate((D, H, W))]


def _ref(pred, y, sd, ids, rounded=False):
    p = pred.double().requires_grad_(True)
    terms = lpips_ref.perceptual_terms(p, y, sd, ids, rounded=rounded)
    total = sum(terms)
    total.backward()
    return float(total.detach()), [float(t.detach()) for t in terms], p.grad.clone()


@functools.lru_cache(maxsize=None)
def _case(name):
    c = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 40)
    y = torch.rand(c["shape"], generator=g)
    pred = (y + 0.1 * torch.randn(c["shape"], generator=g)).clamp(0, 1)
    sd = _weights()
    ids = _ids(c["shape"], c["drop"])
    return y, pred, sd, ids, _ref(pred, y, sd, ids), _ref(pred, y, sd, ids, rounded=True)


def _loss_fn(sd, drop, dtype, chunk=None, cls=None, **kw):
    from synthanatomy_amd.losses import lpips, vqvae
    fn = (cls or vqvae.PerceptualLoss)(dimensions=3, drop_ratio=drop, perceptual_weights=lpips.validate_state_dict(sd, "test"), compute_dtype=dtype, seed=SEED,
                                       **kw).to(DEV)
    fn.set_step(STEP)
    fn.chunk_slices = chunk
    return fn


def _run(y, pred, sd, drop, dtype, chunk=None):
    fn = _loss_fn(sd, drop, dtype, chunk, include_pixel_loss=False)
    p = pred.to(DEV).requires_grad_(True)
    loss = fn({"reconstruction": [p], "quantization_losses": []}, y.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    terms = [float(fn.get_summaries()["scalar"][f"Loss-Perceptual_{i}-Reconstruction"]) for i in range(3)]
    return float(loss.detach()), terms, p.grad.detach().cpu()


def _check_fp32(tag, got, ref, tied=False):
    """tied: volumes with constant regions.  Their feature maps hold EXACT ties inside the max-pool windows, and which tied position receives a window's
    gradient is decided by the last bit of the convolution before it: perturbing the reference's own pool inputs by 1e-13 moves its gradient by 0.7 - 1.1
    of max|ref| on these volumes while loss and sum(gradient) stay put (measured on the CPU).  The element-wise gradient is therefore not a function of
    the arithmetic there; what IS tie-independent is the derivative along the constant direction, sum(gradient) -- every tied position moves together --
    and that is held to the same 1e-3 rule, next to finiteness everywhere."""
    (gl, gt, gg), (rl, rt, rg) = got, ref
    el = abs(gl - rl) / abs(rl)
    if tied:
        eg = abs(float(gg.double().sum()) - float(rg.sum())) / abs(float(rg.sum()))
    else:
        eg = float((gg.double() - rg).abs().max() / rg.abs().max())
    print(f"[{tag} fp32] loss {gl:.9g} ref {rl:.9g} rel err {el:.2e}; gradient {'|sum err| / |sum ref|' if tied else 'max err / max|ref|'} {eg:.2e}; per view " +
          ", ".join(f"{abs(a - b) / abs(b):.2e}" for a, b in zip(gt, rt)))
    assert bool(torch.isfinite(gg).all())
    assert el <= TOL and eg <= TOL
    for a, b in zip(gt, rt):
        assert abs(a - b) <= TOL * abs(b)


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_mode_matches_the_fp64_reference(name):
    y, pred, sd, ids, ref, _ = _case(name)
    _check_fp32(name, _run(y, pred, sd, CASES[name]["drop"], torch.float32), ref)


@pytest.mark.parametrize("name", list(CASES))
def test_bf16_mode_within_four_delta_of_the_fp64_reference(name):
    y, pred, sd, ids, ref, rnd = _case(name)
    gl, gt, gg = _run(y, pred, sd, CASES[name]["drop"], torch.bfloat16)
    d_loss, d_grad = abs(rnd[0] - ref[0]), float((rnd[2] - ref[2]).abs().max())
    e_loss, e_grad = abs(gl - ref[0]), float((gg.double() - ref[2]).abs().max())
    print(f"[{name} bf16] delta loss {d_loss:.3e} (rel {d_loss / abs(ref[0]):.2e}), kernel err {e_loss:.3e}, ratio {e_loss / d_loss:.2f}; "
          f"delta gradient {d_grad:.3e} (rel {d_grad / float(ref[2].abs().max()):.2e}), kernel err {e_grad:.3e}, ratio {e_grad / d_grad:.2f}")
    assert bool(torch.isfinite(gg).all())
    assert e_loss <= 4 * d_loss and e_grad <= 4 * d_grad


def test_constant_volumes_exercise_the_padding_rule():
    """a constant image: every border output of conv1 reads padded taps, where the scaling layer's shift must not leak"""
    shape = (1, 1, 31, 33, 35)
    y, pred = torch.full(shape, 0.3), torch.full(shape, 0.6)
    sd, ids = _weights(), _ids(shape, 0.0)
    ref = _ref(pred, y, sd, ids)
    _check_fp32("C constant", _run(y, pred, sd, 0.0, torch.float32), ref, tied=True)
    # the witness on these volumes: with the shift leaked into the padding the reference itself moves by more than the tolerance
    p = pred.double()
    leaked = float(sum(lpips_ref.perceptual_terms(p, y, sd, ids, defect="pad_shift")))
    print(f"[C constant] leaked-shift reference {leaked:.9g} vs {ref[0]:.9g}")
    assert abs(leaked - ref[0]) > 10 * TOL * abs(ref[0])


def test_zero_feature_vectors_take_the_subgradient_zero():
    """conv1's bias is set so that a zero block of the prediction gives all-zero feature vectors at the first tap while the target's are not zero there:
    upstream's autograd returns NaN; the kernel's gradient is finite everywhere and equals the reference with the subgradient 0"""
    shape = (1, 1, 31, 33, 35)
    g = torch.Generator().manual_seed(9)
    y = torch.rand(shape, generator=g)
    pred = (y + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
    pred[:, :, 4:, 4:, 4:] = 0
    sd = dict(_weights())
    w1 = sd["net.slice1.0.weight"].double()
    shift, scale = (torch.tensor(v, dtype=torch.float64).view(1, 3, 1, 1) for v in (lpips_ref.SHIFT, lpips_ref.SCALE))
    pre = F.conv2d(((-1 - shift) / scale).expand(1, 3, 11, 11), w1).reshape(-1)      # interior pre-activation of a zero image, bias 0
    sd["net.slice1.0.bias"] = (-pre - 0.05).float()
    ids = _ids(shape, 0.0)
    f1 = lpips_ref.features(lpips_ref.slices(pred.double(), 0), sd)[0]
    assert int(((f1 * f1).sum(1) == 0).sum()) > 0, "the case must contain all-zero feature vectors"
    ref = _ref(pred, y, sd, ids)
    assert bool(torch.isfinite(ref[2]).all())
    for dtype in (torch.float32, torch.bfloat16):
        got = _run(y, pred, sd, 0.0, dtype)
        assert bool(torch.isfinite(got[2]).all()) and np.isfinite(got[0]), dtype
        if dtype == torch.float32:
            _check_fp32("C zero block", got, ref, tied=True)


def test_repeatable_reentrant_and_chunk_independent():
    y, pred, sd, ids, _, _ = _case("B")
    drop = CASES["B"]["drop"]
    for dtype in (torch.float32, torch.bfloat16):
        a = _run(y, pred, sd, drop, dtype)
        b = _run(y, pred, sd, drop, dtype)
        assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2]), f"{dtype}: two runs differ"
        c = _run(y, pred, sd, drop, dtype, chunk=5)       # chunks of 5 slices instead of one chunk per view
        h = _run(y, pred, sd, drop, dtype, chunk=3)
        assert c[0] == a[0] and torch.equal(c[2], a[2]) and h[0] == a[0] and torch.equal(h[2], a[2]), f"{dtype}: the chunk size changes the result"
    fn = _loss_fn(sd, drop, torch.float32, include_pixel_loss=False)
    p = pred.to(DEV).requires_grad_(True)
    loss = fn({"reconstruction": [p], "quantization_losses": []}, y.to(DEV))
    g1, = torch.autograd.grad(loss, p, retain_graph=True)       # what AdversarialTrainer's adaptive weight does before the real backward
    loss.backward()
    assert torch.equal(g1, p.grad)
    assert not list(fn.parameters()) and not fn.state_dict()


def test_maxpool_kernels_match_torch_with_ties_and_a_dropped_column():
    """MaxPool2d(3, 2) channels-last against torch on an 7 x 8 map (the floor drops column 7: its gradient is exactly zero) with many ties"""
    from synthanatomy_amd import _ffi
    lib = _ffi.lib()
    g = torch.Generator().manual_seed(3)
    S, Hi, Wi, C = 3, 7, 8, 40
    x = torch.randint(0, 4, (S, C, Hi, Wi), generator=g).float()          # few distinct values: ties in most windows
    x64 = x.double().requires_grad_(True)
    yr = F.max_pool2d(x64, 3, 2)
    gy = torch.randn(yr.shape, generator=g).bfloat16().float()
    yr.backward(gy.double())
    add = torch.randn(S, Hi, Wi, C, generator=g).bfloat16().float()
    mask = torch.relu(torch.randn(S, Hi, Wi, C, generator=g)).bfloat16().float()
    for dt in (torch.float32, torch.bfloat16):
        did = _ffi.dtype_id(dt)
        xc = x.permute(0, 2, 3, 1).contiguous().to(DEV).to(dt)
        y = torch.empty((S, 3, 3, C), dtype=dt, device=DEV)
        idx = torch.empty((S, 3, 3, C), dtype=torch.uint8, device=DEV)
        _ffi.check(lib.sa_lpips_maxpool_fwd(_ffi.ptr(xc), did, _ffi.ptr(y), _ffi.ptr(idx), S, Hi, Wi, C, _ffi.stream()), "fwd")
        gx = torch.empty_like(xc)
        gyc = gy.permute(0, 2, 3, 1).contiguous().to(DEV).to(dt)
        _ffi.check(lib.sa_lpips_maxpool_bwd(_ffi.ptr(gyc), _ffi.ptr(idx), None, None, did, _ffi.ptr(gx), S, Hi, Wi, C, _ffi.stream()), "bwd")
        gm = torch.empty_like(xc)
        addc, maskc = add.to(DEV).to(dt), mask.to(DEV).to(dt)
        _ffi.check(lib.sa_lpips_maxpool_bwd(_ffi.ptr(gyc), _ffi.ptr(idx), _ffi.ptr(addc), _ffi.ptr(maskc), did, _ffi.ptr(gm), S, Hi, Wi, C, _ffi.stream()),
                   "bwd + addend + mask")
        torch.cuda.synchronize()
        assert torch.equal(y.float().cpu().permute(0, 3, 1, 2).double(), yr.detach())
        got = gx.float().cpu().permute(0, 3, 1, 2).double()
        # (a position that is the first maximum of several windows sums their gradients: exact in fp32, one rounding in bf16)
        assert float((got - x64.grad).abs().max()) <= (0 if dt == torch.float32 else 2.0 ** -7 * float(x64.grad.abs().max()))
        assert bool((got[..., 7] == 0).all()), "the column no window covers must get an exactly zero gradient"
        want = (x64.grad.permute(0, 2, 3, 1) + add.double()) * (mask > 0)
        assert float((gm.float().cpu().double() - want).abs().max()) <= (1e-6 if dt == torch.float32 else 2.0 ** -7) * float(want.abs().max())
        assert bool((gm.float().cpu()[mask == 0] == 0).all())


@functools.lru_cache(maxsize=None)
def _golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "losses_perceptual.npz"))


@pytest.mark.parametrize("sname", ["small", "background"])
@pytest.mark.parametrize("lname", ["perceptual", "jukebox_perceptual", "hartley_perceptual"])
def test_full_classes_match_the_reference_fixture(lname, sname):
    from synthanatomy_amd.losses import vqvae
    gold = _golden()
    y = torch.from_numpy(gold[f"input/{sname}/y_u8"]).float() / 255
    pred = torch.from_numpy(gold[f"input/{sname}/pred_u8"]).float() / 255
    q = torch.from_numpy(gold[f"input/{sname}/qloss"])
    cls = {"perceptual": vqvae.PerceptualLoss, "jukebox_perceptual": vqvae.JukeboxPerceptualLoss, "hartley_perceptual": vqvae.HartleyPerceptualLoss}[lname]
    fn = _loss_fn(lpips_ref.draw_weights(int(gold["seed"])), 0.0, torch.float32, cls=cls)
    p = pred.to(DEV).requires_grad_(True)
    loss = fn({"reconstruction": [p], "quantization_losses": [q[0].to(DEV)]}, y.to(DEV))
    loss.backward()
    c = f"case/{lname}/{sname}/"
    ref = float(gold[c + "loss"])
    print(f"[{lname} {sname}] loss {float(loss):.9g} ref {ref:.9g}")
    assert abs(float(loss) - ref) <= TOL * abs(ref)
    summ = fn.get_summaries()["scalar"]
    keys = [k[len(c):] for k in gold.files if k.startswith(c) and k[len(c):] not in ("loss", "dpred_strided")]
    assert any(k.startswith("Loss-Perceptual_2") for k in keys)
    for k in keys:
        assert k in summ, k
        assert abs(float(summ[k]) - float(gold[c + k])) <= TOL * abs(float(gold[c + k])), k
    assert summ["Auxiliary-Perceptual_Factor"] == 0.001
    gref = torch.from_numpy(gold[c + "dpred_strided"])
    got = p.grad.detach().cpu().double().reshape(-1)[::8]
    assert float((got - gref).abs().max()) <= TOL * float(gref.abs().max())


def test_cli_training_smoke(tmp_path, capsys):
    import run_vqvae
    proj = str(tmp_path) + "/"
    run_vqvae.run(["--project_directory=" + proj, "--experiment_name=lp", "--no_levels=2", "--downsample_parameters=((4,2,1,1),(4,2,1,1))",
                   "--upsample_parameters=((4,2,1,0,1),(4,2,1,0,1))", "--no_channels=32", "--num_embeddings=(64,)", "--embedding_dim=(16,)", "--decay=(0.5,)",
                   "--roi=((0,32),(0,32),(0,32))", "--batch_size=2", "--eval_batch_size=2", "--learning_rate=1e-3", "--gamma=0.9", "--training_subjects=synthetic:4",
                   "--validation_subjects=synthetic:2", "--mode=training", "--eval_every=1", "--epochs=1", "--loss=jukebox_perceptual",
                   "--perceptual_weights=random:0"])
    out = capsys.readouterr().out
    its = re.findall(r"^epoch 0 it (\d+) loss (\S+) (.*)$", out, flags=re.M)
    assert len(its) == 2, out
    for _, loss, rest in its:
        assert np.isfinite(float(loss))
        vals = re.findall(r"Loss-Perceptual_(\d)-Reconstruction (\S+)", rest)
        assert [v[0] for v in vals] == ["0", "1", "2"] and all(np.isfinite(float(v[1])) and float(v[1]) > 0 for v in vals), rest
    assert "STAND-IN weights" in out
    ckpt = torch.load(glob.glob(proj + "lp/baseline_vqvae/checkpoints/checkpoint_epoch=1.pt")[0], map_location="cpu", weights_only=False)

    def names(o, pre=""):
        if isinstance(o, dict):
            for k, v in o.items():
                yield from names(v, f"{pre}{k}.")
        else:
            yield pre

    assert not [n for n in names(ckpt) if "lin" in n.split(".")[0:1] or "slice" in n or "perceptual" in n.lower() or "lpips" in n.lower()]
