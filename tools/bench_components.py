"""Connected components (csrc/components.hip) for one volume of the production size, 160 x 224 x 160.

    python tools/bench_components.py [--dims 160 224 160] [--iters 50] [--warmup 5] [--no_scipy] [--out profiles/components_bench_line.json]

Prints one JSON line and writes it to ``--out``.  Per input, on the same box in the same process (device events, median and minimum of ``--iters``):
  blobs        a smoothed random field thresholded to about 2 % foreground (tens of blobs of thousands of voxels and specks), c = 26, min_size = 20, with
               a label volume made the same way: the mode's case
  percolation  a uniform random field at density 0.30 with c = 6, near the lattice's percolation threshold: sprawling components, the hard case for
               chain lengths
  full         every voxel foreground, c = 26: one component, every tile-local piece adds into ONE word
``sa_components`` (its five launches) in us, the bytes per voxel of the launches' traffic model and the share of the 6.29 TB/s copy rate.  Where scipy
imports, ``scipy.ndimage.label`` plus ``bincount`` on the host for the same input, for information only (the copy to the host is not in it)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
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


def bytes_per_voxel(tile, labelled):
    """The launches' traffic model, compulsory bytes only (the neighbour reads of the merge and the second hops of the filter hit in cache):
    local   reads the volume (4, the label volume 1) and writes parent and size (8);
    merge   reads parent on the tile's faces (4 x the share of face voxels);
    flatten reads size (4);
    filter  reads parent (4) and writes ids (4); with labels the label byte (1) and the label forest's parent (4).
    With labels the label volume goes through local, merge and flatten as well (1 + 8, 4 x faces, 4) and local reads its byte for the map's pieces."""
    td, th, tw = tile
    faces = 1.0 - (td - 1) * (th - 2) * (tw - 2) / (td * th * tw)
    one = 4 + 8 + 4 * faces + 4 + 8
    return one if not labelled else one + 1 + (1 + 8 + 4 * faces + 4) + 5


def _blobs(shape, seed, dev, share=0.02):
    import torch.nn.functional as F
    g = torch.Generator(device=dev).manual_seed(seed)
    v = torch.rand((1, 1) + tuple(shape), device=dev, generator=g)
    for _ in range(2):
        v = F.avg_pool3d(v, 9, stride=1, padding=4, count_include_pad=False)
    v = v[0, 0]
    t = torch.quantile(v.flatten()[::7], 1.0 - share)
    return ((v - t) * 50.0 + 0.5).clamp_(0.0, 1.0).contiguous()      # foreground [>= 0.5]: about `share` of the voxels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=[160, 224, 160])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no_scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_bench_line.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_components needs a HIP device"
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.metrics.components import NAMES, TILE
    lib = _ffi.lib()
    dev = torch.device("cuda:0")
    D, H, W = args.dims
    n = D * H * W
    g = torch.Generator(device=dev).manual_seed(1)
    inputs = {
        "blobs": (_blobs((D, H, W), 2, dev), 0.5, 26, 20, (_blobs((D, H, W), 3, dev) >= 0.5).to(torch.uint8)),
        "percolation": (torch.rand((D, H, W), device=dev, generator=g), 0.70, 6, 1, None),
        "full": (torch.ones((D, H, W), device=dev), 0.5, 26, 1, None),
    }
    out = {"dims": [D, H, W], "tile": list(TILE), "iters": args.iters, "inputs": {}}
    ndi = None
    if not args.no_scipy:
        try:
            import scipy.ndimage as ndi
        except ImportError:
            out["scipy"] = "not installed"
    for name, (a, t, c, m, y) in inputs.items():
        a = a.reshape(1, D, H, W).contiguous()
        P = _ffi.ComponentsParams(B=1, D=D, H=H, W=W, connectivity=c, min_size=m, has_labels=int(y is not None), threshold=t)
        ws = torch.empty((lib.sa_components_workspace_bytes(ctypes.byref(P)) + 7) // 8, dtype=torch.float64, device=dev)
        res = torch.empty(1, _ffi.COMPONENTS_RESULT_WORDS, dtype=torch.int64, device=dev)
        ids = torch.empty((1, D, H, W), dtype=torch.int32, device=dev)

        def run():
            _ffi.check(lib.sa_components(_ffi.ptr(a), _ffi.ptr(y), _ffi.ptr(ids), ctypes.byref(P), _ffi.ptr(res), _ffi.ptr(ws), _ffi.stream()), "sa_components")

        med, best = _events(run, args.iters, args.warmup)
        bpv = bytes_per_voxel(TILE, y is not None)
        line = {"connectivity": c, "min_size": m, "labels": y is not None, "us_median": round(med * 1e3, 1), "us_min": round(best * 1e3, 1),
                "bytes_per_voxel": round(bpv, 2), "GB_s": round(bpv * n / (med * 1e-3) / 1e9, 1),
                "share_of_hbm_peak": round(bpv * n / (med * 1e-3) / HBM_PEAK, 3)}
        line.update({k: int(v) for k, v in zip(NAMES, res[0, :5].tolist())})
        if ndi is not None:
            host = (a[0] >= t).cpu().numpy()
            t0 = time.perf_counter()
            lab, found = ndi.label(host, structure=ndi.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[c]))
            sizes = np.bincount(lab.ravel())
            line["scipy_label_bincount_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            assert found == line["components"] and int(sizes[1:].max(initial=0)) == line["largest_component"]
        out["inputs"][name] = line
    out["model_floor_us"] = round(bytes_per_voxel(TILE, False) * n / HBM_PEAK * 1e6, 1)
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
