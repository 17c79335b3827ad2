"""The 2.5D LPIPS-alex perceptual term on the HIP path (losses/lpips.py, csrc/lpips.hip) against the same rule composed from torch
operators on the same box (``permute().contiguous()`` / index / ``F.conv2d`` / ``F.max_pool2d`` / autograd, as upstream's ``_calculate_fake_3d_loss``
with a torch AlexNet), at the production reconstruction volume with upstream's ``drop_ratio=0.5`` and seeded stand-in weights; then the time of a
``--loss=jukebox_perceptual`` training step against ``--loss=jukebox``.

    python tools/bench_lpips.py [--shape 8 1 160 224 160] [--iters 5] [--warmup 2] [--step_iters 4] [--skip_step]

Device events, median over iterations; each iteration is the forward of the term plus its gradient to the prediction for one batch.  Prints one JSON
line: milliseconds per mode (HIP bf16 / fp32, torch fp32 / bf16 autocast), the kept slices, the GMAC of the AlexNet stack derived from the layer shapes,
the effective TFLOP/s (3 passes: two forwards and one data gradient), the agreement of the two fp32 results, and the two step times."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def torch_term(pred, y, net, ids, factor, autocast):
    """the term as upstream composes it, with a torch AlexNet holding the same weights; returns (sum of the per-view terms, gradient)"""
    from synthanatomy_amd.losses import lpips
    p = pred.detach().requires_grad_(True)
    shift = net.shift.float().view(1, 3, 1, 1)
    scale = net.scale.float().view(1, 3, 1, 1)
    total = 0
    for view, perm in enumerate(((0, 2, 1, 3, 4), (0, 3, 1, 2, 4), (0, 4, 1, 2, 3))):
        idx = ids[view].long()

        def feats(v):
            s = v.permute(*perm).contiguous()
            s = s.view(-1, *s.shape[2:])[idx]
            x = ((2 * s - 1) - shift) / scale
            out = []
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                for i, (_, _, _, st, pd) in enumerate(lpips.ALEX_CONVS):
                    if i in (1, 2):
                        x = F.max_pool2d(x, 3, 2)
                    x = F.relu(F.conv2d(x, getattr(net, f"w{i}"), getattr(net, f"b{i}"), stride=st, padding=pd))
                    out.append(x)
            return out

        with torch.no_grad():
            f0 = feats(y)
        f1 = feats(p)
        d = 0
        for l, (a, b) in enumerate(zip(f0, f1)):
            a, b = a.float(), b.float()
            a = a / (a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            b = b / (b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            d = d + (getattr(net, f"lin{l}").view(1, -1, 1, 1) * (a - b) ** 2).sum(1).mean((1, 2))
        total = total + d.mean() * factor
    total.backward()
    return total.detach(), p.grad


def conv_gmac_per_slice(h, w):
    from synthanatomy_amd.losses import lpips
    h1, w1 = lpips.conv1_extent(h), lpips.conv1_extent(w)
    h2, w2 = lpips.pool_extent(h1), lpips.pool_extent(w1)
    h3, w3 = lpips.pool_extent(h2), lpips.pool_extent(w2)
    pos = (h1 * w1, h2 * w2, h3 * w3, h3 * w3, h3 * w3)
    return sum(p * ci * co * k * k for p, (ci, co, k, _, _) in zip(pos, lpips.ALEX_CONVS)) / 1e9


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
    for name in ("jukebox", "jukebox_perceptual"):
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
    out["perceptual_share_of_step"] = round(1 - out["jukebox"]["ms_median"] / out["jukebox_perceptual"]["ms_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=5, default=[8, 1, 160, 224, 160])
    ap.add_argument("--drop_ratio", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step_iters", type=int, default=4)
    ap.add_argument("--skip_step", action="store_true")
    ap.add_argument("--skip_torch", action="store_true")
    args = ap.parse_args()
    from synthanatomy_amd.losses import lpips

    assert torch.cuda.is_available(), "bench_lpips needs a HIP device"
    dev = torch.device("cuda:0")
    B, C, D, H, W = args.shape
    gen = torch.Generator(device=dev).manual_seed(1)
    y = torch.rand(args.shape, generator=gen, device=dev)
    pred = (y + 0.05 * torch.randn(args.shape, generator=gen, device=dev)).clamp(0, 1)
    weights = lpips.load_weights("random:0")
    factor = 0.001
    ids = [torch.from_numpy(lpips.draw_slices(0, 0, v, B * n, int(B * n * (1 - args.drop_ratio)))).to(dev) for v, n in enumerate((D, H, W))]
    kept = [int(i.numel()) for i in ids]
    gmac = sum(k * conv_gmac_per_slice(*hw) for k, hw in zip(kept, ((H, W), (D, W), (D, H))))
    out = {"shape": args.shape, "drop_ratio": args.drop_ratio, "kept_slices": kept, "alexnet_gmac_per_pass": round(gmac, 1), "weights": "random:0"}
    nets = {dt: lpips.LpipsAlex(weights, dt).to(dev) for dt in (torch.bfloat16, torch.float32)}
    results = {}

    def hip(dt):
        p = pred.detach().requires_grad_(True)
        total, *_ = lpips.PerceptualFn.apply(p, y, nets[dt], (0, 1, 2), ids, factor, True, None)
        total.backward()
        results[dt] = (total.detach(), p.grad)

    modes = [("hip_bf16", lambda: hip(torch.bfloat16)), ("hip_fp32", lambda: hip(torch.float32))]
    if not args.skip_torch:
        modes += [("torch_fp32", lambda: results.__setitem__("t32", torch_term(pred, y, nets[torch.float32], ids, factor, False))),
                  ("torch_bf16_autocast", lambda: results.__setitem__("t16", torch_term(pred, y, nets[torch.float32], ids, factor, True)))]
    for name, fn in modes:
        med, best = _time(fn, args.iters, args.warmup)
        out[name] = {"ms_median": round(med, 2), "ms_min": round(best, 2), "effective_TFLOPs": round(3 * 2 * gmac / med, 1)}
    if not args.skip_torch:
        (l_h, g_h), (l_t, g_t) = results[torch.float32], results["t32"]
        out["fp32_loss_rel_diff_vs_torch"] = abs(float(l_h) - float(l_t)) / abs(float(l_t))
        out["fp32_grad_max_diff_over_max_vs_torch"] = float((g_h - g_t).abs().max() / g_t.abs().max())
        out["speedup_bf16_vs_torch_bf16_autocast"] = round(out["torch_bf16_autocast"]["ms_median"] / out["hip_bf16"]["ms_median"], 2)
        out["speedup_fp32_vs_torch_fp32"] = round(out["torch_fp32"]["ms_median"] / out["hip_fp32"]["ms_median"], 2)
    del nets, results
    torch.cuda.empty_cache()
    if not args.skip_step:
        out["training_step"] = step_times(args.shape, args.step_iters, 2, weights)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
