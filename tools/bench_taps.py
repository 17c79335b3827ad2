"""The one-channel rearrangements of csrc/taps.hip at the production size: 80 x 112 x 80 cells, batch 8.

    python tools/bench_taps.py [--cells 80 112 80] [--batch 8] [--iters 20] [--warmup 3] [--step]

Prints one JSON line with, all on the same box in the same process (device events, median and minimum):
  k4s2p1      ``sa_taps_unfold`` (bf16 and fp32 rows) and ``sa_taps_fold`` beside their specialised twins ``sa_convt1_im2col`` / ``sa_convt1_gather`` on the same
              volume and cells, with the achieved bytes per second over the algorithmic bytes (unfold: the volume read once + the rows written once; fold: the
              rows read once + the volume written once) and whether the general kernel reproduces its twin bit for bit
  k3s2p1, k2s2p0   the same two general kernels for tuples that have no twin
  step        (``--step``) one training step of BaselineVQVAE with five levels of (4,2,1,1) at 176 x 208 x 176 (latent 5 x 6 x 5: the first up-sampling level is
              (4,2,1,1,1) to come back to 11 x 13 x 11), batch 1, beside the default five-level
              tuples at 160 x 224 x 160: ms per step, what an odd-extent run costs"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _events(fn, iters, warmup):
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


def _row(med, best, nbytes):
    return {"us_median": round(med * 1e3, 1), "us_min": round(best * 1e3, 1), "GB_s": round(nbytes / (med * 1e-3) / 1e9, 1)}


def _kernels(args, out):
    from synthanatomy_amd import _ffi
    lib, st = _ffi.lib(), _ffi.stream()
    dev = torch.device("cuda:0")
    N, cells = args.batch, tuple(args.cells)
    for name, (k, s, p, d) in (("k4s2p1", (4, 2, 1, 1)), ("k3s2p1", (3, 2, 1, 1)), ("k2s2p0", (2, 2, 0, 1))):
        vol = tuple((c - 1) * s - 2 * p + d * (k - 1) + 1 for c in cells)            # the transposed convolution's output = the strided convolution's input
        x = torch.rand((N, *vol), device=dev)
        res = {"volume": list(vol)}
        for dt, vec in ((torch.bfloat16, 8), (torch.float32, 4)):
            ld = (k ** 3 + vec - 1) // vec * vec
            Xc = torch.empty((N, *cells, ld), dtype=dt, device=dev)
            nbytes = x.numel() * 4 + Xc.numel() * Xc.element_size()
            med, best = _events(lambda: _ffi.check(lib.sa_taps_unfold(_ffi.ptr(x), _ffi.dtype_id(dt), _ffi.ptr(Xc), None, N, *vol, *cells, k, s, d, -p, ld, st), "unfold"),
                                args.iters, args.warmup)
            key = "bf16" if dt == torch.bfloat16 else "f32"
            res[f"unfold_{key}"] = _row(med, best, nbytes)
            if name == "k4s2p1":
                Xt = torch.empty_like(Xc)
                med, best = _events(lambda: _ffi.check(lib.sa_convt1_im2col(_ffi.ptr(x), _ffi.dtype_id(dt), _ffi.ptr(Xt), None, N, *cells, st), "im2col"), args.iters, args.warmup)
                res[f"convt1_im2col_{key}"] = _row(med, best, nbytes)
                res[f"unfold_{key}_equals_twin"] = bool(torch.equal(Xc.view(torch.int16 if dt == torch.bfloat16 else torch.int32), Xt.view(torch.int16 if dt == torch.bfloat16 else torch.int32)))
            del Xc
        ld = (k ** 3 + 3) // 4 * 4
        P = torch.randn((N, *cells, ld), device=dev)
        bias = torch.full((1,), 0.1, device=dev)
        y = torch.empty((N, *vol), device=dev)
        nbytes = (P.numel() + y.numel()) * 4
        med, best = _events(lambda: _ffi.check(lib.sa_taps_fold(_ffi.ptr(P), _ffi.ptr(bias), _ffi.ptr(y), N, *cells, *vol, k, s, p, d, ld, st), "fold"), args.iters, args.warmup)
        res["fold"] = _row(med, best, nbytes)
        if name == "k4s2p1":
            yt = torch.empty_like(y)
            med, best = _events(lambda: _ffi.check(lib.sa_convt1_gather(_ffi.ptr(P), _ffi.ptr(bias), _ffi.ptr(yt), N, *cells, st), "gather"), args.iters, args.warmup)
            res["convt1_gather"] = _row(med, best, nbytes)
            res["fold_max_abs_diff_to_twin"] = float((y - yt).abs().max())
        out[name] = res
        del x, P, y


def _step(out):
    from synthanatomy_amd.networks.vqvae.baseline import BaselineVQVAE
    res = {}
    for name, up, dims in (("odd_176x208x176", ((4, 2, 1, 1, 1),) + ((4, 2, 1, 0, 1),) * 4, (176, 208, 176)), ("default_160x224x160", ((4, 2, 1, 0, 1),) * 5, (160, 224, 160))):
        torch.manual_seed(0)
        net = BaselineVQVAE(n_levels=5, downsample_parameters=((4, 2, 1, 1),) * 5, upsample_parameters=up).cuda().train()
        x = torch.rand(1, 1, *dims, device="cuda")

        def step():
            net.zero_grad(set_to_none=True)
            o = net(x)
            assert o["reconstruction"][0].shape == x.shape, (o["reconstruction"][0].shape, x.shape)
            (torch.nn.functional.mse_loss(o["reconstruction"][0].float(), x) + o["quantization_losses"][0]).backward()

        med, best = _events(step, 5, 2)
        res[name] = {"ms_median": round(med, 2), "ms_min": round(best, 2)}
        del net, x
        torch.cuda.empty_cache()
    out["step"] = res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs=3, default=[80, 112, 80])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_taps needs a HIP device"
    out = {"cells": list(args.cells), "batch": args.batch}
    _kernels(args, out)
    if args.step:
        print(json.dumps(out), file=sys.stderr, flush=True)       # (the kernel rows survive a failing step)
        _step(out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
