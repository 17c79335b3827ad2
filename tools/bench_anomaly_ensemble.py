"""The ensemble anomaly map (csrc/anomaly.hip: sa_anomaly_map_ensemble) for one volume of the production size: 160 x 224 x 160, factor 8,
sigma 4, with and without a label volume, for K in {1, 2, 4, 8} members.

    python tools/bench_anomaly_ensemble.py [--dims 160 224 160] [--factor 8] [--sigma 4] [--members 1 2 4 8] [--iters 50] [--warmup 5]

Prints one JSON line with, all on the same box in the same process (device events, median and minimum):
  fused        ``sa_anomaly_map_ensemble`` (its clear, the map launch and the per-volume sums); us, and GB/s over the traffic model
               4 n (x) + 4 K n (r_k) + 4 n (a) + n (label, when given) + K latent grids: (K + 2) 4 bytes per voxel
  composition  what the surface offered before: K x ``anomaly_map`` (each with the label and the threshold when there is a label), ``torch.stack`` and
               ``mean`` of the K maps, and one unweighted ``anomaly_map(mean, 0)`` for the summaries of the mean; us, and its model of
               (4 K + 6) 4 bytes per voxel (+ (K + 1) label bytes)
  single       ``sa_anomaly_map`` next to the K = 1 fused call, timed twice (the spread of two runs of the same call)
The composition's mean differs from the fused map in the last place (a torch mean is not the sequential sum times inv_K); the figure is reported."""
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


def _line(med, best, moved, n):
    return {"us_median": round(med * 1e3, 1), "us_min": round(best * 1e3, 1), "bytes_per_voxel": round(moved / n, 3),
            "GB_s": round(moved / (med * 1e-3) / 1e9, 1), "share_of_hbm_peak": round(moved / (med * 1e-3) / HBM_PEAK, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=[160, 224, 160])
    ap.add_argument("--factor", type=int, default=8)
    ap.add_argument("--sigma", type=float, default=4.0)
    ap.add_argument("--members", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_anomaly_ensemble needs a HIP device"
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.metrics.anomaly import anomaly_map, anomaly_map_ensemble, gaussian_taps
    lib = _ffi.lib()
    dev = torch.device("cuda:0")
    D, H, W = args.dims
    f = args.factor
    lat = (D // f, H // f, W // f)
    n = D * H * W
    kmax = max(args.members)
    torch.manual_seed(0)
    x = torch.rand(1, D, H, W, device=dev)
    r = torch.rand(kmax, 1, D, H, W, device=dev)
    m = (torch.rand(kmax, 1, *lat, device=dev) < 0.1).float()
    label = (torch.rand(1, D, H, W, device=dev) < 0.05).to(torch.uint8)
    zero = torch.zeros_like(x)
    taps = gaussian_taps(args.sigma)
    out = {"dims": [D, H, W], "factor": f, "sigma": args.sigma, "R": (len(taps) - 1) // 2, "members": {}}

    P = _ffi.AnomalyParams(B=1, D=D, H=H, W=W, residual=0, has_threshold=0, inv_bin=256.0, threshold=0.05)
    P.d, P.h, P.w = lat
    P.R = (len(taps) - 1) // 2
    for i, g in enumerate(taps.tolist()):
        P.taps[i] = g
    ws = torch.empty(lib.sa_anomaly_map_workspace_bytes(ctypes.byref(P)) // 8, dtype=torch.float64, device=dev)
    res = torch.empty(1, _ffi.ANOMALY_RESULT_WORDS, dtype=torch.int64, device=dev)
    a_out = torch.empty_like(x)

    for K in args.members:
        entry = {}
        for name, labelled in (("no_label", False), ("label_threshold", True)):
            P.has_threshold = int(labelled)
            lab = label if labelled else None
            kw = dict(sigma=args.sigma, labels=lab, threshold=0.05 if labelled else None)

            def fused():
                _ffi.check(lib.sa_anomaly_map_ensemble(_ffi.ptr(x), _ffi.ptr(r), n, _ffi.ptr(m), m[0].numel(), _ffi.ptr(lab), _ffi.ptr(a_out),
                                                       ctypes.byref(P), K, _ffi.ptr(res), _ffi.ptr(ws), _ffi.stream()), "sa_anomaly_map_ensemble")

            def composition():
                maps = [anomaly_map(x, r[k], m[k], **kw)[0] for k in range(K)]
                mean = torch.stack(maps).mean(dim=0)
                return anomaly_map(mean, zero, None, **kw)

            med, best = _events(fused, args.iters, args.warmup)
            entry[name] = {"fused": _line(med, best, 4 * n * (K + 2) + (n if labelled else 0) + 4 * K * m[0].numel(), n)}
            med, best = _events(composition, max(args.iters // 5, 5), 2)
            entry[name]["composition"] = _line(med, best, 4 * n * (4 * K + 6) + ((K + 1) * n if labelled else 0) + 4 * K * m[0].numel(), n)
            entry[name]["composition_over_fused"] = round(entry[name]["composition"]["us_median"] / entry[name]["fused"]["us_median"], 2)
            ours, _ = anomaly_map_ensemble(x, r[:K], m[:K], **kw)
            theirs, _ = composition()
            entry[name]["max_abs_difference_composition_from_fused"] = float((ours - theirs).abs().max())
        out["members"][str(K)] = entry

    # K = 1 fused next to sa_anomaly_map, the latter twice: is the member loop's frame visible beside the spread of two runs of the same call?
    P.has_threshold = 0

    def single():
        _ffi.check(lib.sa_anomaly_map(_ffi.ptr(x), _ffi.ptr(r), _ffi.ptr(m), None, _ffi.ptr(a_out), ctypes.byref(P), _ffi.ptr(res), _ffi.ptr(ws),
                                      _ffi.stream()), "sa_anomaly_map")

    def fused_one():
        _ffi.check(lib.sa_anomaly_map_ensemble(_ffi.ptr(x), _ffi.ptr(r), n, _ffi.ptr(m), m[0].numel(), None, _ffi.ptr(a_out), ctypes.byref(P), 1,
                                               _ffi.ptr(res), _ffi.ptr(ws), _ffi.stream()), "sa_anomaly_map_ensemble")

    runs = [_events(fn, args.iters, args.warmup) for fn in (single, fused_one, single, fused_one)]
    out["single_vs_one_member"] = {"sa_anomaly_map_us_median": [round(runs[0][0] * 1e3, 1), round(runs[2][0] * 1e3, 1)],
                                   "sa_anomaly_map_ensemble_K1_us_median": [round(runs[1][0] * 1e3, 1), round(runs[3][0] * 1e3, 1)],
                                   "sa_anomaly_map_us_min": [round(runs[0][1] * 1e3, 1), round(runs[2][1] * 1e3, 1)],
                                   "sa_anomaly_map_ensemble_K1_us_min": [round(runs[1][1] * 1e3, 1), round(runs[3][1] * 1e3, 1)]}
    assert math.isfinite(out["members"][str(args.members[0])]["no_label"]["fused"]["us_median"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
