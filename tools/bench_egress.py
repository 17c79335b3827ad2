"""The NIfTI output path (csrc/egress.hip) for one volume of the production size, 160 x 224 x 160.

    python tools/bench_egress.py [--dims 160 224 160] [--iters 20] [--warmup 3] [--volumes 12] [--rounds 2] [--no_cli]

Prints one JSON line with, all on the same box in the same process:
  kernel      ``sa_volume_egress`` alone (device events, median) from an fp32 volume: float32 and int16 with auto-scaling, for an orientation whose
              perm[2] == 0 (straight from registers) and one where it is not (the LDS transpose), each also with every axis reversed; us and GB/s over
              the algorithmic bytes (float32: 4 n read + 4 n written; int16 auto-scaled: 2 x 4 n read + 2 n written)
  ingest      ``sa_volume_ingest`` of the float32 block just written, same box and process: the kernel that moves the same bytes the other way
  decoding    wall time per volume of ``run_vqvae.py --mode=decoding`` on the default (production) network over ``--volumes`` code grids: ``.npy`` (the
              unchanged path, the baseline), ``.nii`` and ``.nii.gz`` with ``--num_workers`` 0 and 8, alternating for ``--rounds`` rounds; the network
              is built once and handed to every run, so a run is the loop plus the flag parsing"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
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


def _kernels(args, out):
    from synthanatomy_amd import _ffi
    lib = _ffi.lib()
    dev = torch.device("cuda:0")
    ext = list(args.dims)
    n = ext[0] * ext[1] * ext[2]
    x = torch.rand(ext, device=dev)
    ws = torch.zeros(8, dtype=torch.int64, device=dev)
    raw = torch.empty(n * 4, dtype=torch.uint8, device=dev)
    out["kernel"] = {}
    orientations = (("straight", (1, 2, 0), (1, 1, 1)), ("straight_reversed", (1, 2, 0), (-1, -1, -1)), ("transposed", (0, 1, 2), (1, 1, 1)),
                    ("transposed_lps", (0, 1, 2), (-1, -1, 1)))
    for name, perm, sign in orientations:
        for dtype, code, moved in (("float32", 16, 8 * n), ("int16", 4, 10 * n)):
            P = _ffi.EgressParams(x_dtype=0, dtype=code, flags=1, slope=1.0, inter=0.0)
            P.ext[:], P.perm[:], P.sign[:] = ext, perm, sign

            def run():
                _ffi.check(lib.sa_volume_egress(_ffi.ptr(x), _ffi.ptr(raw), raw.numel(), ctypes.byref(P), _ffi.ptr(ws), _ffi.stream()), "sa_volume_egress")

            med, best = _events(run, args.iters, args.warmup)
            out["kernel"][f"{name}_{dtype}"] = {"us_median": round(med * 1e3, 1), "us_min": round(best * 1e3, 1), "GB_s": round(moved / (med * 1e-3) / 1e9, 1)}
    # the other direction on the float32 block of the last orientation, no normalisation: n x 4 bytes in, n x 4 bytes out
    name, perm, sign = orientations[-1]
    P = _ffi.EgressParams(x_dtype=0, dtype=16, flags=0, slope=1.0, inter=0.0)
    P.ext[:], P.perm[:], P.sign[:] = ext, perm, sign
    _ffi.check(lib.sa_volume_egress(_ffi.ptr(x), _ffi.ptr(raw), raw.numel(), ctypes.byref(P), _ffi.ptr(ws), _ffi.stream()), "sa_volume_egress")
    y = torch.empty(ext, dtype=torch.float32, device=dev)
    ws_in = torch.zeros(8, dtype=torch.int64, device=dev)
    Q = _ffi.IngestParams(dtype=16, byteswap=0, flags=0, slope=1.0, inter=0.0)
    dims = [0, 0, 0]
    for a in range(3):
        dims[perm[a]] = ext[a]
    Q.n[:], Q.perm[:], Q.sign[:], Q.off[:], Q.ext[:] = dims, perm, sign, (0, 0, 0), ext

    def back():
        _ffi.check(lib.sa_volume_ingest(_ffi.ptr(raw), raw.numel(), _ffi.ptr(y), ctypes.byref(Q), _ffi.ptr(ws_in), _ffi.stream()), "sa_volume_ingest")

    med, best = _events(back, args.iters, args.warmup)
    out["ingest"] = {f"{name}_float32": {"us_median": round(med * 1e3, 1), "us_min": round(best * 1e3, 1), "GB_s": round(8 * n / (med * 1e-3) / 1e9, 1)}}
    out["round_trip_exact"] = bool(torch.equal(x, y))


def _decoding(args, out):
    import run_vqvae
    from synthanatomy_amd.utils.general import parse_flags
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        proj = tmp + "/"
        os.mkdir(proj + "codes")
        base = [f"--training_subjects={proj}codes", f"--validation_subjects={proj}codes", "--project_directory=" + proj, "--experiment_name=bench",
                "--mode=decoding"]
        cfg = parse_flags(base, run_vqvae.DEFAULTS)
        grid = [(b - a) // 2 ** cfg["no_levels"] for a, b in cfg["roi"]]
        rng = np.random.default_rng(0)
        for k in range(args.volumes):
            np.save(f"{proj}codes/v{k:03d}.npy", rng.integers(0, cfg["num_embeddings"][0], grid).astype(np.uint16))
        torch.manual_seed(0)
        net = run_vqvae.build_network(cfg, dev)
        build, run_vqvae.build_network = run_vqvae.build_network, lambda cfg, dev: net      # every run below decodes with this one network
        variants = [("npy", ".npy", 8), ("nii_w0", ".nii", 0), ("nii_w8", ".nii", 8), ("nii_gz_w0", ".nii.gz", 0), ("nii_gz_w8", ".nii.gz", 8)]
        times = {k: [] for k, _, _ in variants}
        try:
            for r in range(args.rounds + 1):      # round 0 warms up
                for key, ext, workers in variants:
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    with contextlib.redirect_stdout(io.StringIO()):
                        run_vqvae.run(base + [f"--output_ext={ext}", f"--num_workers={workers}"])
                    torch.cuda.synchronize()
                    if r:
                        times[key].append((time.perf_counter() - t) * 1e3 / args.volumes)
        finally:
            run_vqvae.build_network = build
        out["decoding_ms_per_volume"] = {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2)} for k, v in times.items()}
        outputs = proj + "bench/baseline_vqvae/outputs/v000/"
        out["file_bytes"] = {f: os.path.getsize(outputs + f) for f in sorted(os.listdir(outputs))}
        out["volumes"], out["rounds"] = args.volumes, args.rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=[160, 224, 160])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--volumes", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no_cli", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_egress needs a HIP device"
    out = {"dims": list(args.dims)}
    _kernels(args, out)
    if not args.no_cli:
        _decoding(args, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
