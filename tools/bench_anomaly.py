"""The anomaly map (csrc/anomaly.hip) for one volume of the production size: 160 x 224 x 160, factor 8, sigma 4.

    python tools/bench_anomaly.py [--dims 160 224 160] [--factor 8] [--sigma 4] [--iters 50] [--warmup 5] [--no_torch]

Prints one JSON line with, all on the same box in the same process (device events, median and minimum):
  kernel   ``sa_anomaly_map`` (its clear, the map launch and the per-volume sums) for the mask weight with and without a label volume and a threshold,
           and without a weight grid; us, and GB/s over the traffic model: 4 n (x) + 4 n (r) + 4 n (a) + n (label, when given) + the latent grid
  torch    the same rule composed from torch operators on the same tensors: ``repeat_interleave`` per axis, three ``conv1d`` passes with zero padding,
           ``abs`` and ``mul``; and how far its map is from the kernel's
  egress   ``sa_volume_egress`` float32 of the same volume (8 bytes per voxel), for orientation"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 6.29e12      # bytes / s, the measured float4-copy rate of the MI355X


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


def _line(med, best, moved):
    return {"us_median": round(med * 1e3, 1), "us_min": round(best * 1e3, 1), "bytes": moved, "GB_s": round(moved / (med * 1e-3) / 1e9, 1),
            "share_of_hbm_peak": round(moved / (med * 1e-3) / HBM_PEAK, 3)}


def torch_composition(x, r, m, taps, factors):
    """a = |x - r| * (m upsampled by repeat_interleave and filtered by three zero-padded conv1d passes)"""
    import torch.nn.functional as F
    u = m
    for axis, f in enumerate(factors):
        u = u.repeat_interleave(f, dim=axis)
    k = taps.reshape(1, 1, -1)
    R = (taps.numel() - 1) // 2
    for axis in range(3):
        v = u.movedim(axis, -1)
        shape = v.shape
        v = F.conv1d(v.reshape(-1, 1, shape[-1]), k, padding=R).reshape(shape)
        u = v.movedim(-1, axis)
    return (x - r).abs() * u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=[160, 224, 160])
    ap.add_argument("--factor", type=int, default=8)
    ap.add_argument("--sigma", type=float, default=4.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no_torch", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_anomaly needs a HIP device"
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.metrics.anomaly import anomaly_map, gaussian_taps
    lib = _ffi.lib()
    dev = torch.device("cuda:0")
    D, H, W = args.dims
    f = args.factor
    lat = (D // f, H // f, W // f)
    n = D * H * W
    torch.manual_seed(0)
    x, r = torch.rand(1, D, H, W, device=dev), torch.rand(1, D, H, W, device=dev)
    m = (torch.rand(1, *lat, device=dev) < 0.1).float()
    label = (torch.rand(1, D, H, W, device=dev) < 0.05).to(torch.uint8)
    taps = gaussian_taps(args.sigma)
    out = {"dims": [D, H, W], "factor": f, "sigma": args.sigma, "R": (len(taps) - 1) // 2, "kernel": {}}

    a_out = torch.empty_like(x)
    res = torch.empty(1, _ffi.ANOMALY_RESULT_WORDS, dtype=torch.int64, device=dev)
    for name, weighted, labelled in (("mask", True, False), ("mask_label_threshold", True, True), ("none", False, False)):
        P = _ffi.AnomalyParams(B=1, D=D, H=H, W=W, residual=0, has_threshold=int(labelled), inv_bin=256.0, threshold=0.05)
        if weighted:
            P.d, P.h, P.w = lat
            P.R = (len(taps) - 1) // 2
            for i, g in enumerate(taps.tolist()):
                P.taps[i] = g
        nbytes = lib.sa_anomaly_map_workspace_bytes(ctypes.byref(P))
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)

        def run():
            _ffi.check(lib.sa_anomaly_map(_ffi.ptr(x), _ffi.ptr(r), _ffi.ptr(m) if weighted else None, _ffi.ptr(label) if labelled else None,
                                          _ffi.ptr(a_out), ctypes.byref(P), _ffi.ptr(res), _ffi.ptr(ws), _ffi.stream()), "sa_anomaly_map")

        med, best = _events(run, args.iters, args.warmup)
        moved = 12 * n + (n if labelled else 0) + (4 * m.numel() if weighted else 0)
        out["kernel"][name] = _line(med, best, moved)
        out["kernel"][name]["bytes_per_voxel"] = round(moved / n, 3)

    if not args.no_torch:
        try:
            tk = torch.from_numpy(taps).to(dev)
            fn = lambda: torch_composition(x[0], r[0], m[0], tk, (f, f, f))      # noqa: E731
            med, best = _events(fn, max(args.iters // 5, 5), 2)
            ours, _ = anomaly_map(x, r, m, sigma=args.sigma)
            out["torch"] = {"us_median": round(med * 1e3, 1), "us_min": round(best * 1e3, 1),
                            "max_abs_difference_from_kernel": float((fn() - ours[0]).abs().max())}
        except Exception as e:      # (a convolution back end that is missing or refuses the shape: reported, not hidden)
            out["torch"] = {"error": f"{type(e).__name__}: {e}"[:300]}

    P = _ffi.EgressParams(x_dtype=0, dtype=16, flags=0, slope=1.0, inter=0.0)
    P.ext[:], P.perm[:], P.sign[:] = (D, H, W), (1, 2, 0), (1, 1, 1)
    raw = torch.empty(n * 4, dtype=torch.uint8, device=dev)
    ws_e = torch.zeros(8, dtype=torch.int64, device=dev)

    def egress():
        _ffi.check(lib.sa_volume_egress(_ffi.ptr(x), _ffi.ptr(raw), raw.numel(), ctypes.byref(P), _ffi.ptr(ws_e), _ffi.stream()), "sa_volume_egress")

    med, best = _events(egress, args.iters, args.warmup)
    out["egress"] = {"straight_float32": _line(med, best, 8 * n)}
    out["model_floor_us"] = round(12 * n / HBM_PEAK * 1e6, 1)
    assert math.isfinite(out["kernel"]["mask"]["us_median"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
