"""Fused BaurLoss (``sa_baur_loss``: L1 + L2 + gdl_factor * gradient-difference loss and d loss / d pred, csrc/losses.hip) against the same loss and
gradient as the reference writes them in torch (src/losses/vqvae/vqvae.py:131-170: ConstantPad3d shifts, [1:-1] crops, autograd), at the production
reconstruction volume.

    python tools/bench_baur_loss.py [--shape 8 1 160 224 160] [--factor 2.5] [--iters 50] [--warmup 5]

Times both with device events (median over iterations, each the loss + gradient for one batch) and prints one JSON line: microseconds, GB/s
counting 12 bytes per voxel (read pred and target, write the gradient once) and that rate as a fraction of 6.3 TB/s, the achievable HBM bandwidth."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 6.3e12


def torch_reference_way(pred, y, factor):
    """Loss + gradient as upstream's BaurLoss computes them (reduction "mean")."""
    dx = torch.nn.ConstantPad3d((1, -1, 0, 0, 0, 0), 0)
    dy = torch.nn.ConstantPad3d((0, 0, 1, -1, 0, 0), 0)
    dz = torch.nn.ConstantPad3d((0, 0, 0, 0, 1, -1), 0)
    p = pred.detach().requires_grad_(True)
    c = (slice(None), slice(None), slice(1, -1), slice(1, -1), slice(1, -1))
    l1 = torch.nn.functional.l1_loss(p, y)
    l2 = torch.nn.functional.mse_loss(p, y)
    gdl = (torch.abs(torch.abs(dx(y) - y)[c] - torch.abs(dx(p) - p)[c]) + torch.abs(torch.abs(dy(y) - y)[c] - torch.abs(dy(p) - p)[c])
           + torch.abs(torch.abs(dz(y) - y)[c] - torch.abs(dz(p) - p)[c])).mean() * factor
    loss = l1 + l2 + gdl
    loss.backward()
    return loss.detach(), p.grad


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
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=5, default=[8, 1, 160, 224, 160])
    ap.add_argument("--factor", type=float, default=2.5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from synthanatomy_amd import _ffi

    assert torch.cuda.is_available(), "bench_baur_loss needs a HIP device"
    dev = torch.device("cuda:0")
    B, C, D, H, W = args.shape
    gen = torch.Generator(device=dev).manual_seed(1)
    y = torch.rand(args.shape, generator=gen, device=dev)
    pred = y + 0.05 * torch.randn(args.shape, generator=gen, device=dev)
    grad = torch.empty_like(pred)
    sums = torch.empty(3, device=dev)
    lib = _ffi.lib()
    ws = torch.empty(lib.sa_baur_loss_workspace_bytes(B * C, D, H, W) // 4, device=dev)

    def fused(factor=args.factor):
        _ffi.check(lib.sa_baur_loss(_ffi.ptr(pred), _ffi.ptr(y), B * C, D, H, W, factor, 0, 1.0, _ffi.ptr(sums), _ffi.ptr(grad), _ffi.ptr(ws),
                                    _ffi.stream()), "sa_baur_loss")

    bytes_moved = 12 * pred.numel()
    out = {"shape": args.shape, "gdl_factor": args.factor, "bytes_per_voxel": 12}
    for name, fn in (("fused", fused), ("fused_factor0", lambda: fused(0.0)), ("torch", lambda: torch_reference_way(pred, y, args.factor))):
        med, best = _time(fn, args.iters, args.warmup)
        out[name] = {"us_median": round(med, 1), "us_min": round(best, 1), "GB_s": round(bytes_moved / (med * 1e-6) / 1e9, 1),
                     "frac_6p3TBs": round(bytes_moved / (med * 1e-6) / HBM_BYTES_PER_S, 3)}
    fused()
    ref_loss, ref_grad = torch_reference_way(pred, y, args.factor)
    n, m = pred.numel(), B * C * (D - 2) * (H - 2) * (W - 2)
    loss = float(sums[0] / n + sums[1] / n + sums[2] / m * args.factor)
    out["loss_rel_diff"] = abs(loss - float(ref_loss)) / abs(float(ref_loss))
    out["grad_max_abs_diff"] = float((grad - ref_grad).abs().max())
    out["speedup_vs_torch"] = round(out["torch"]["us_median"] / out["fused"]["us_median"], 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
