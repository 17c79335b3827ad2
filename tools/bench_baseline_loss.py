"""``BaselineLoss`` (``--loss=baseline``) on the HIP path (losses/vqvae.py, losses/lpips_squeeze.py, csrc/lpips_squeeze.hip) against
the same rule composed from torch operators on the same box (``permute().contiguous()`` / index / ``F.conv2d`` / ``F.max_pool2d(ceil_mode=True)`` /
``torch.cat`` / autograd, as upstream's ``_calculate_perceptual_loss`` with a torch SqueezeNet-1.1), at the production reconstruction volume with
upstream's ``n_slices = 512`` and seeded stand-in weights; then the time of a ``--loss=baseline`` training step against ``--loss=jukebox``.

    python tools/bench_baseline_loss.py [--shape 8 1 160 224 160] [--iters 3] [--warmup 1] [--step_iters 3] [--skip_step] [--skip_torch] [--out FILE]

Device events, median over iterations; each iteration is forward plus gradient to the prediction for one batch, of the whole loss and of the perceptual
term alone.  Prints (and with --out writes) one JSON line: milliseconds per mode (HIP bf16 / fp32, torch fp32 / bf16 autocast), the kept slices, the GMAC of
the SqueezeNet stack per pass derived from the layer shapes (merged expands counted as launched), the agreement of the two fp32 results, the step times."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_lpips import _time  # noqa: E402

VIEWS = (0, 2, 1)       # sagittal, axial, coronal
PERMUTES = ((0, 2, 1, 3, 4), (0, 3, 1, 2, 4), (0, 4, 1, 2, 3))


def torch_perceptual(pred, y, sd, ids, factor, autocast):
    """the perceptual term as upstream composes it, with a torch SqueezeNet holding the same weights: factor * sum of the three means (differentiable)"""
    from synthanatomy_amd.losses import lpips, lpips_squeeze
    shift = torch.tensor(lpips.SHIFT, device=pred.device).view(1, 3, 1, 1)
    scale = torch.tensor(lpips.SCALE, device=pred.device).view(1, 3, 1, 1)
    total = 0
    for view, idx in zip(VIEWS, ids):
        def feats(v):
            s = v.permute(*PERMUTES[view]).contiguous()
            s = s.view(-1, *s.shape[2:])[idx.long()]
            x = (s - shift) / scale
            out = []
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                x = F.relu(F.conv2d(x, sd["net.slice1.0.weight"], sd["net.slice1.0.bias"], stride=2))
                out.append(x)
                for i, (feat, key, *_r) in enumerate(lpips_squeeze.FIRES):
                    if feat in (3, 6, 9):
                        x = F.max_pool2d(x, 3, 2, ceil_mode=True)
                    z = F.relu(F.conv2d(x, sd[key + ".squeeze.weight"], sd[key + ".squeeze.bias"]))
                    x = torch.cat([F.relu(F.conv2d(z, sd[key + ".expand1x1.weight"], sd[key + ".expand1x1.bias"])),
                                   F.relu(F.conv2d(z, sd[key + ".expand3x3.weight"], sd[key + ".expand3x3.bias"], padding=1))], 1)
                    if i in lpips_squeeze.TAP_FIRES:
                        out.append(x)
            return out

        with torch.no_grad():
            f0 = feats(y)
        f1 = feats(pred)
        d = 0
        for l, (a, b) in enumerate(zip(f0, f1)):
            a, b = a.float(), b.float()
            a = a / (a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            b = b / (b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            d = d + (sd[lpips_squeeze.LIN_KEYS[l]].view(1, -1, 1, 1) * (a - b) ** 2).sum(1).mean((1, 2))
        total = total + d.mean()
    return total * factor


def torch_loss(pred, y, sd, ids, autocast, perceptual_only):
    p = pred.detach().requires_grad_(True)
    total = torch_perceptual(p, y, sd, ids, 0.002, autocast)
    if not perceptual_only:
        amp = lambda t: torch.abs(torch.fft.fftn((t + 1.0) / 2.0, norm="ortho"))      # noqa: E731
        total = total + F.l1_loss(p, y) + F.mse_loss(amp(y), amp(p))
    total.backward()
    return total.detach(), p.grad


def squeeze_gmac_per_slice(h, w):
    from synthanatomy_amd.losses import lpips_squeeze
    (h1, h2, h3, h4), (w1, w2, w3, w4) = lpips_squeeze.extents(h), lpips_squeeze.extents(w)
    mac = h1 * w1 * 9 * 64
    for feat, _, ci, s, e1, e3 in lpips_squeeze.FIRES:
        pos = h2 * w2 if feat in (3, 4) else h3 * w3 if feat in (6, 7) else h4 * w4
        mac += pos * (ci * s + s * (e1 + e3) * 9)       # the merged expand runs nine taps on both halves
    return mac / 1e9


def step_times(shape, iters, warmup, weights):
    """one training step of run_vqvae.py's loop (forward, loss, backward, Adam) on bench.py's flagship network (bf16), per loss"""
    import bench
    from synthanatomy_amd.losses.vqvae import get_vqvae_loss
    from synthanatomy_amd.networks.vqvae.baseline import BaselineVQVAE
    from synthanatomy_amd.runtime.ddp import GradReducer
    from synthanatomy_amd.runtime.optim import FlatParams, FusedAdam
    dev = torch.device("cuda:0")
    x = torch.rand(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    out = {}
    for name in ("jukebox", "baseline"):
        torch.manual_seed(4)
        net = BaselineVQVAE(**bench.NET, compute_dtype=torch.bfloat16).to(dev).train()
        flat = FlatParams(net.parameters())
        red = GradReducer(flat)
        net.set_grad_sink(red)
        opt = FusedAdam(flat, lr=1.65e-4)
        opt.on_step.append(net.invalidate_packed_weights)
        loss_fn = get_vqvae_loss({"loss": name, "perceptual_weights": weights, "compute_dtype": torch.bfloat16, "seed": 0})
        if hasattr(loss_fn, "set_step"):
            loss_fn.to(dev)
        it = [0]

        def step():
            if hasattr(loss_fn, "set_step"):
                loss_fn.set_step(it[0])
            it[0] += 1
            flat.zero_grad()
            loss = loss_fn(net(x), x)
            loss.backward()
            opt.step(grad_scale=red.finish())

        med, best = _time(step, iters, warmup)
        out[name] = {"ms_median": round(med, 2), "ms_min": round(best, 2)}
        del net, flat, red, opt, loss_fn
        torch.cuda.empty_cache()
    out["baseline_over_jukebox"] = round(out["baseline"]["ms_median"] / out["jukebox"]["ms_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=5, default=[8, 1, 160, 224, 160])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step_iters", type=int, default=3)
    ap.add_argument("--skip_step", action="store_true")
    ap.add_argument("--skip_torch", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from synthanatomy_amd.losses import lpips, vqvae

    assert torch.cuda.is_available(), "bench_baseline_loss needs a HIP device"
    dev = torch.device("cuda:0")
    B, C, D, H, W = args.shape
    gen = torch.Generator(device=dev).manual_seed(1)
    y = torch.rand(args.shape, generator=gen, device=dev)
    pred = (y + 0.05 * torch.randn(args.shape, generator=gen, device=dev)).clamp(0, 1)
    weights = lpips.load_weights("random:0", net="squeeze")
    fns = {dt: vqvae.BaselineLoss(perceptual_weights=weights, compute_dtype=dt, seed=0).to(dev) for dt in (torch.bfloat16, torch.float32)}
    ids = [torch.from_numpy(lpips.draw_slices(0, 0, v, B * (D, H, W)[v], min(512, B * (D, H, W)[v]))).to(dev) for v in VIEWS]
    kept = [int(i.numel()) for i in ids]
    gmac = sum(k * squeeze_gmac_per_slice(*((H, W), (D, W), (D, H))[v]) for k, v in zip(kept, VIEWS))
    out = {"shape": args.shape, "n_slices": 512, "kept_slices_sagittal_axial_coronal": kept, "squeezenet_gmac_per_pass": round(gmac, 1), "weights": "random:0"}
    sd = {k: v.to(dev) for k, v in weights.items() if v.dtype == torch.float32}
    results = {}

    def hip(dt, perceptual_only):
        fn = fns[dt]
        p = pred.detach().requires_grad_(True)
        if perceptual_only:
            fn.summaries = {"scalar": {}}
            total = fn._calculate_perceptual_loss(p, y)
        else:
            total = fn({"reconstruction": [p], "quantization_losses": []}, y)
        total.backward()
        results[(dt, perceptual_only)] = (total.detach(), p.grad)

    for only in (False, True):
        tag = "perceptual" if only else "loss"
        modes = [(f"hip_bf16_{tag}", lambda o=only: hip(torch.bfloat16, o)), (f"hip_fp32_{tag}", lambda o=only: hip(torch.float32, o))]
        if not args.skip_torch:
            modes += [(f"torch_fp32_{tag}", lambda o=only: results.__setitem__(("t32", o), torch_loss(pred, y, sd, ids, False, o))),
                      (f"torch_bf16_autocast_{tag}", lambda o=only: results.__setitem__(("t16", o), torch_loss(pred, y, sd, ids, True, o)))]
        for name, fn in modes:
            med, best = _time(fn, args.iters, args.warmup)
            out[name] = {"ms_median": round(med, 2), "ms_min": round(best, 2)}
            if only:
                out[name]["effective_TFLOPs"] = round(3 * 2 * gmac / med, 1)
            torch.cuda.empty_cache()
        if not args.skip_torch:
            (l_h, g_h), (l_t, g_t) = results[(torch.float32, only)], results[("t32", only)]
            out[f"fp32_{tag}_rel_diff_vs_torch"] = abs(float(l_h) - float(l_t)) / abs(float(l_t))
            out[f"fp32_{tag}_grad_max_diff_over_max_vs_torch"] = float((g_h - g_t).abs().max() / g_t.abs().max())
            out[f"speedup_bf16_vs_torch_bf16_autocast_{tag}"] = round(out[f"torch_bf16_autocast_{tag}"]["ms_median"] / out[f"hip_bf16_{tag}"]["ms_median"], 2)
            out[f"speedup_fp32_vs_torch_fp32_{tag}"] = round(out[f"torch_fp32_{tag}"]["ms_median"] / out[f"hip_fp32_{tag}"]["ms_median"], 2)
        results.clear()
    del fns, results
    torch.cuda.empty_cache()
    if not args.skip_step:
        out["training_step"] = step_times(args.shape, args.step_iters, 1, weights)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
