"""Masked median filter of an anomaly map (csrc/median.hip) for one volume of the production size, 160 x 224 x 160.

    python tools/bench_median.py [--dims 160 224 160] [--iters 50] [--warmup 5] [--no_torch] [--no_scipy] [--out profiles/median_bench_line.json]

Prints one JSON line and writes it to ``--out``.  Per window side (3, 5), input and variant, on the same box in the same process (device events, median
and minimum of ``--iters``):
  dense    a uniform random map: every window needs the full selection
  sparse   the 2 % blob field of tools/bench_components.py multiplied into a random residual: zero almost everywhere, the mode's case
  zeros    all zeros: every block takes the constant-tile early-out
each ``plain`` (no mask, no labels) and ``masked`` (a ball mask, erosion 2, labels and a threshold).  ``sa_anomaly_median`` (all its launches) in us,
its share of the copy-rate floor (map in, map out, mask and label bytes at 6.29 TB/s) and of the VALU estimate of DESIGN 7.18 (32 bisection steps of
2 k^3 lane-operations per voxel at 39 T lane-ops/s).  For comparison on the dense map: the torch composition (pad + three unfolds + median, chunked
along D) on the same GPU, and ``scipy.ndimage.median_filter`` on the host where scipy imports (the copy to the host is not in it)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_components import _blobs, _events      # noqa: E402  (tools/bench_components.py: the same blob field and timer)

HBM_PEAK = 6.29e12      # bytes / s, the measured float4-copy rate of the MI355X
VALU_RATE = 39e12       # lane-operations / s, the estimate of DESIGN 7.18 (256 CUs x 64 lanes x 2.4 GHz)


def torch_median(a, k, chunk=8):
    """the composition torch offers: zero pad, three unfolds, median over the k^3 window, D planes `chunk` at a time"""
    import torch.nn.functional as F
    r = k // 2
    p = F.pad(a, (r, r, r, r, r, r))
    out = torch.empty_like(a)
    for d0 in range(0, a.shape[0], chunk):
        d1 = min(d0 + chunk, a.shape[0])
        win = p[d0:d1 + 2 * r].unfold(0, k, 1).unfold(1, k, 1).unfold(2, k, 1)
        out[d0:d1] = win.reshape(d1 - d0, a.shape[1], a.shape[2], k ** 3).median(dim=-1).values
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=[160, 224, 160])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no_torch", action="store_true")
    ap.add_argument("--no_scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "median_bench_line.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_median needs a HIP device"
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.metrics.median import TILE
    lib = _ffi.lib()
    dev = torch.device("cuda:0")
    D, H, W = args.dims
    n = D * H * W
    g = torch.Generator(device=dev).manual_seed(1)
    dense = torch.rand((D, H, W), device=dev, generator=g)
    inputs = {
        "dense": dense,
        "sparse": ((_blobs((D, H, W), 2, dev) >= 0.5).float() * torch.rand((D, H, W), device=dev, generator=g)).contiguous(),
        "zeros": torch.zeros((D, H, W), device=dev),
    }
    zz, yy, xx = torch.meshgrid(*[torch.linspace(-1, 1, s, device=dev) for s in (D, H, W)], indexing="ij")
    ball = (zz * zz + yy * yy + xx * xx <= 1.0).to(torch.uint8).contiguous()
    label = (_blobs((D, H, W), 3, dev) >= 0.5).to(torch.uint8)
    out = {"dims": [D, H, W], "tile": list(TILE), "iters": args.iters, "sizes": {}}
    res = torch.empty(1, _ffi.ANOMALY_RESULT_WORDS, dtype=torch.int64, device=dev)
    o = torch.empty((1, D, H, W), device=dev)
    for k in (3, 5):
        lines = {}
        for name, a in inputs.items():
            a = a.reshape(1, D, H, W).contiguous()
            for variant, (m, e, y) in (("plain", (None, 0, None)), ("masked", (ball, 2, label))):
                P = _ffi.MedianParams(B=1, D=D, H=H, W=W, size=k, erosion=e, has_mask=int(m is not None), has_labels=int(y is not None),
                                      has_threshold=int(y is not None), inv_bin=256.0, threshold=0.5)
                ws = torch.empty((lib.sa_anomaly_median_workspace_bytes(ctypes.byref(P)) + 7) // 8, dtype=torch.float64, device=dev)

                def run():
                    _ffi.check(lib.sa_anomaly_median(_ffi.ptr(a), _ffi.ptr(m), _ffi.ptr(y), _ffi.ptr(o), ctypes.byref(P), _ffi.ptr(res), _ffi.ptr(ws),
                                                     _ffi.stream()), "sa_anomaly_median")

                med, best = _events(run, args.iters, args.warmup)
                bpv = 8 + (1 + 2 * e if m is not None else 0) + (1 if y is not None else 0)      # an erosion step reads and writes a byte
                floor_us = bpv * n / HBM_PEAK * 1e6
                valu_us = 32 * 2 * k ** 3 * n / VALU_RATE * 1e6
                lines[f"{name}_{variant}"] = {"us_median": round(med * 1e3, 1), "us_min": round(best * 1e3, 1), "bytes_per_voxel": bpv,
                                              "copy_floor_us": round(floor_us, 1), "times_copy_floor": round(med * 1e3 / floor_us, 1),
                                              "valu_estimate_us": round(valu_us, 1), "share_of_valu_estimate": round(med * 1e3 / valu_us, 3),
                                              "nonzero_out": int((o != 0).sum())}
        if not args.no_torch:
            med, best = _events(lambda: torch_median(inputs["dense"], k), 3, 1)
            lines["torch_composition_dense_ms"] = round(med, 1)
            P = _ffi.MedianParams(B=1, D=D, H=H, W=W, size=k, erosion=0, has_mask=0, has_labels=0, has_threshold=0, inv_bin=256.0, threshold=0.0)
            ws = torch.empty((lib.sa_anomaly_median_workspace_bytes(ctypes.byref(P)) + 7) // 8, dtype=torch.float64, device=dev)
            _ffi.check(lib.sa_anomaly_median(_ffi.ptr(inputs["dense"]), None, None, _ffi.ptr(o), ctypes.byref(P), _ffi.ptr(res), _ffi.ptr(ws), _ffi.stream()))
            assert torch.equal(o[0], torch_median(inputs["dense"], k)), "the kernel and the torch composition disagree on a finite map"
        if not args.no_scipy:
            try:
                import scipy.ndimage as ndi
                host = inputs["dense"].cpu().numpy()
                t0 = time.perf_counter()
                ndi.median_filter(host, size=k, mode="constant", cval=0.0)
                lines["scipy_median_filter_dense_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            except ImportError:
                out["scipy"] = "not installed"
        out["sizes"][str(k)] = lines
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
