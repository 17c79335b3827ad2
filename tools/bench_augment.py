"""``sa_augment`` (csrc/augment.hip) at the production batch: the two launches alone, records already on the device.

    python tools/bench_augment.py [--shape 8 1 160 224 160] [--iters 30] [--warmup 5]

Times each case with device events (median over iterations) and prints one JSON line: microseconds, GB/s over the bytes the case has to move (read the
input and write the output once = 8 bytes per voxel; a sample with the gamma bit is read and written once more by the second pass = 16) and that rate
as a fraction of 6.3 TB/s, the achievable HBM bandwidth.  ``schedule`` is a batch as ``--augmentation=True`` draws it at the default probability 0.2."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 6.3e12


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
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.utils import vqvae as uv

    assert torch.cuda.is_available(), "bench_augment needs a HIP device"
    dev = torch.device("cuda:0")
    B, _, D, H, W = args.shape
    dims = (D, H, W)
    x = torch.rand(args.shape, generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    y = torch.empty_like(x)
    lib = _ffi.lib()
    ws = torch.zeros(lib.sa_augment_workspace_bytes(B) // 8, dtype=torch.int64, device=dev)
    every = uv.AUG_GAMMA | uv.AUG_SHIFT | uv.AUG_NOISE | uv.AUG_CLAMP

    def rec(mode=uv.AUG_IDENTITY, flags=0):
        r = uv.identity_record(dims)
        r["mode"], r["flags"] = mode, flags
        r["perm"], r["sign"] = (0, 1, 2), (-1, 1, -1)
        r["M"] = uv.affine_matrix((0.04, -0.03, 0.02), (1.5, -0.5, 1.0), (1.03, 0.98, 1.01)).astype(np.float32).reshape(-1)
        r["gamma"], r["shift"], r["noise_std"] = 1.01, 0.02, 0.01
        return r

    cfg = dict(augmentation=True, augmentation_probability=0.2, augmentation_strength=0, patch_size=None)
    cases = {"identity": [rec()] * B, "flips": [rec(uv.AUG_SIGNED_PERM)] * B, "affine": [rec(uv.AUG_AFFINE)] * B,
             "shift_noise_clamp": [rec(flags=every & ~uv.AUG_GAMMA)] * B, "affine_all_intensity": [rec(uv.AUG_AFFINE, every)] * B,
             "schedule": [uv.draw_augmentation(cfg, "training", 4, 0, s, dims) for s in range(B)]}
    out = {"shape": args.shape}
    for name, recs in cases.items():
        recs = np.stack(recs)
        uv.check_records(recs, dims, dims)
        params = torch.from_numpy(recs.view(np.uint8).reshape(B, -1)).to(dev)

        def run():
            _ffi.check(lib.sa_augment(_ffi.ptr(x), _ffi.ptr(y), B, D, H, W, D, H, W, _ffi.ptr(params), 1234, _ffi.ptr(ws), _ffi.stream()), "sa_augment")

        med, best = _time(run, args.iters, args.warmup)
        moved = sum(16 if int(r["flags"]) & uv.AUG_GAMMA else 8 for r in recs) * D * H * W
        out[name] = {"us_median": round(med, 1), "us_min": round(best, 1), "bytes": moved, "GB_s": round(moved / (med * 1e-6) / 1e9, 1),
                     "frac_6p3TBs": round(moved / (med * 1e-6) / HBM_BYTES_PER_S, 3)}
        if name == "schedule":
            out[name]["modes"] = [int(r["mode"]) for r in recs]
            out[name]["flags"] = [int(r["flags"]) for r in recs]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
