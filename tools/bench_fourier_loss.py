"""The spectral terms of ``--loss=spectral | hartley | wavegan`` (reference src/losses/vqvae/vqvae.py:188-323, 326-519, 641-771) at the production
reconstruction volume: this build's path (two unnormalised rocFFT rfftn, the fused ``sa_fourier_loss`` pass, one irfftn for d loss / d pred) against
the torch composition the reference writes (full complex ortho fftn of both volumes, elementwise ops, autograd backward), and the fused pass alone.

    python tools/bench_fourier_loss.py [--shape 8 1 160 224 160] [--iters 30] [--warmup 5]

Times with device events (median over iterations, each one loss + gradient) and prints one JSON line.  The fused pass's bandwidth counts the bytes it
must move per half-spectrum bin: read both spectra and write the gradient (24 B); wavegan reads both spectra twice (40 B).  Fraction of 6.3 TB/s,
the achievable HBM bandwidth.  The pixel term (hip_mse) is left out of both sides."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 6.3e12
DIMS = (1, 2, 3, 4)


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
    from synthanatomy_amd.losses.vqvae import _FOURIER_KIND, _FourierFn

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from fourier_ref import reference_way_fp32

    assert torch.cuda.is_available(), "bench_fourier_loss needs a HIP device"
    dev = torch.device("cuda:0")
    B, C, D, H, W = args.shape
    gen = torch.Generator(device=dev).manual_seed(1)
    y = torch.rand(args.shape, generator=gen, device=dev)
    pred = y + 0.05 * torch.randn(args.shape, generator=gen, device=dev)
    lib = _ffi.lib()
    xp, xy = torch.fft.rfftn(pred, dim=DIMS).contiguous(), torch.fft.rfftn(y, dim=DIMS).contiguous()
    grad_spec = torch.empty_like(xp)
    strides = list(torch.fft.rfftn(pred, dim=DIMS).stride())
    sums = torch.empty(3, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.sa_fourier_loss_workspace_bytes(B, C, D, H, W) // 8, dtype=torch.float64, device=dev)

    nbins = xp.numel()
    out = {"shape": args.shape, "bins": nbins, "rfftn_out_strides": strides}
    for name, fn in (("rfftn_x2_us", lambda: (torch.fft.rfftn(pred, dim=DIMS), torch.fft.rfftn(y, dim=DIMS))),
                     ("rfftn_x2_contiguous_us", lambda: (torch.fft.rfftn(pred, dim=DIMS).contiguous(), torch.fft.rfftn(y, dim=DIMS).contiguous())),
                     ("irfftn_us", lambda: torch.fft.irfftn(xp, s=(C, D, H, W), dim=DIMS, norm="forward"))):
        out[name] = round(_time(fn, args.iters, args.warmup)[0], 1)
    for kind in ("spectral", "hartley", "wavegan"):
        k = _FOURIER_KIND[kind]

        def fused_step():
            p = pred.detach().requires_grad_(True)
            spec, _, _ = _FourierFn.apply(p, y, kind, 1.0, True)
            spec.backward()
            return spec.detach(), p.grad

        def kernel_only():
            _ffi.check(lib.sa_fourier_loss(k, _ffi.ptr(xp), _ffi.ptr(xy), B, C, D, H, W, 1, 1.0, _ffi.ptr(sums), _ffi.ptr(grad_spec), _ffi.ptr(ws),
                                           _ffi.stream()), "sa_fourier_loss")

        bytes_moved = (40 if kind == "wavegan" else 24) * nbins
        row = {}
        for name, fn in (("fused_loss_grad", fused_step), ("torch_loss_grad", lambda: reference_way_fp32(kind, pred, y)),
                         ("kernel", kernel_only)):
            med, best = _time(fn, args.iters, args.warmup)
            row[name] = {"us_median": round(med, 1), "us_min": round(best, 1)}
        kmed = row["kernel"]["us_median"]
        row["kernel"].update({"bytes_per_bin": bytes_moved // nbins, "GB_s": round(bytes_moved / (kmed * 1e-6) / 1e9, 1),
                              "frac_6p3TBs": round(bytes_moved / (kmed * 1e-6) / HBM_BYTES_PER_S, 3)})
        row["speedup_vs_torch"] = round(row["torch_loss_grad"]["us_median"] / row["fused_loss_grad"]["us_median"], 2)
        f_loss, f_grad = fused_step()
        r_loss, r_grad = reference_way_fp32(kind, pred, y)
        row["loss_rel_diff"] = abs(float(f_loss) - float(r_loss)) / abs(float(r_loss))
        row["grad_rel_l2"] = float((f_grad.double() - r_grad.double()).norm() / r_grad.double().norm())
        del r_grad, f_grad
        out[kind] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
