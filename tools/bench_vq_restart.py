"""Dead-code restarts of the EMA quantizer: what the opt-in path costs, at the flagship codebook of ``bench.py``'s configuration.

    python tools/bench_vq_restart.py [--batch 8] [--calls 50] [--reps 9] [--step_reps 5] [--block 4] [--skip_step] [--out profiles/vq_restart_bench_line.json]

1. Device time (events around ``--calls`` back-to-back calls, median over ``--reps`` repetitions) of ``sa_vq_ema_update`` -- what the default path launches --
   against ``sa_vq_restart_donors`` + ``sa_vq_ema_update_restart`` with nothing dead and with R = 32 codes dead in every call.
2. The flagship training step (forward, MSE, backward, Adam; bf16) with ``set_codebook_restart`` on (patience so long that nothing dies) against off, the two
   alternating in ONE run in blocks of ``--block`` steps: off(a), on, off(b), off(a), ...  ``on_minus_off_ms`` is the difference of the medians,
   ``off_a_minus_off_b_ms`` the same difference between two labels of the SAME configuration: the spread below which a difference says nothing.

Prints (and with --out writes) one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _events(fn, calls, reps):
    """median and minimum over ``reps`` of the device time of ``calls`` back-to-back fn() (ms per call)"""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / calls)
    return statistics.median(times), min(times)


def kernel_times(K, D, M, R, calls, reps):
    from synthanatomy_amd import _ffi
    lib, st = _ffi.lib(), _ffi.stream()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(3)
    rows = torch.randn(M, D, device=dev, generator=g)
    N = torch.rand(K, device=dev, generator=g) + 0.5
    avg = torch.randn(K, D, device=dev, generator=g)
    cb = torch.empty(K, D, device=dev)
    stats = torch.zeros(K + K * D + R * D, device=dev)
    counts, dw, donors = stats[:K], stats[K:K + K * D], stats[K + K * D:]
    counts.fill_(float(M // K))
    dw.copy_(torch.randn(K * D, device=dev, generator=g))
    idle = torch.zeros(K, dtype=torch.int32, device=dev)
    info = torch.zeros(2 + R, dtype=torch.int32, device=dev)
    step = [0]

    def plain():
        _ffi.check(lib.sa_vq_ema_update(_ffi.ptr(N), _ffi.ptr(avg), _ffi.ptr(cb), _ffi.ptr(counts), _ffi.ptr(dw), K, D, 0.99, 1e-5, st), "sa_vq_ema_update")

    def restart():
        step[0] += 1
        _ffi.check(lib.sa_vq_restart_donors(_ffi.ptr(rows), M, D, 0, M, R, 4, step[0], _ffi.ptr(donors), st), "sa_vq_restart_donors")
        _ffi.check(lib.sa_vq_ema_update_restart(_ffi.ptr(N), _ffi.ptr(avg), _ffi.ptr(cb), _ffi.ptr(counts), _ffi.ptr(dw), K, D, 0.99, 1e-5, _ffi.ptr(idle), 1,
                                                _ffi.ptr(donors), R, _ffi.ptr(info), st), "sa_vq_ema_update_restart")

    out = {}
    med, best = _events(plain, calls, reps)
    out["sa_vq_ema_update_us"] = {"median": round(med * 1e3, 2), "min": round(best * 1e3, 2)}
    med, best = _events(restart, calls, reps)
    assert info.tolist()[:2] == [0, 0]
    out["donors_plus_update_restart_nothing_dead_us"] = {"median": round(med * 1e3, 2), "min": round(best * 1e3, 2)}
    counts[torch.arange(R, device=dev) * (K // R) + 7] = 0.0      # R codes without an assignment, patience 1: dead (and restarted) in EVERY call
    med, best = _events(restart, calls, reps)
    assert info.tolist()[:2] == [R, R]
    out[f"donors_plus_update_restart_{R}_dead_us"] = {"median": round(med * 1e3, 2), "min": round(best * 1e3, 2)}
    return out


def step_times(batch, block, reps):
    import bench
    from synthanatomy_amd.losses.vqvae import get_vqvae_loss
    from synthanatomy_amd.networks.vqvae.baseline import BaselineVQVAE
    from synthanatomy_amd.runtime.ddp import GradReducer
    from synthanatomy_amd.runtime.optim import FlatParams, FusedAdam
    dev = torch.device("cuda:0")
    x = torch.rand((batch, 1, 160, 224, 160), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    torch.manual_seed(4)
    net = BaselineVQVAE(**bench.NET, compute_dtype=torch.bfloat16).to(dev).train()
    flat = FlatParams(net.parameters())
    red = GradReducer(flat)
    net.set_grad_sink(red)
    opt = FusedAdam(flat, lr=1.65e-4)
    opt.on_step.append(net.invalidate_packed_weights)
    loss_fn = get_vqvae_loss({"loss": "mse"})
    it = [0]

    def step():
        if net.quantizer[0].impl._restart is not None:
            net.set_codebook_restart_step(it[0])
        it[0] += 1
        flat.zero_grad()
        loss_fn(net(x), x).backward()
        opt.step(grad_scale=red.finish())

    for _ in range(3):
        step()
    times = {"off_a": [], "on": [], "off_b": []}
    for _ in range(reps):
        for label in ("off_a", "on", "off_b"):
            net.set_codebook_restart(10 ** 9 if label == "on" else None, 32, 4)
            step()      # (the first step of a block allocates the packed buffer of its configuration: not timed)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(block):
                step()
            b.record()
            torch.cuda.synchronize()
            times[label].append(a.elapsed_time(b) / block)
    med = {k: statistics.median(v) for k, v in times.items()}
    off = statistics.median(times["off_a"] + times["off_b"])
    return {"batch": batch, "block_steps": block, "blocks_per_label": reps, "ms_median": {k: round(v, 3) for k, v in med.items()},
            "ms_all": {k: [round(t, 3) for t in v] for k, v in times.items()}, "on_minus_off_ms": round(med["on"] - off, 3),
            "off_a_minus_off_b_ms": round(med["off_a"] - med["off_b"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--step_reps", type=int, default=5)
    ap.add_argument("--block", type=int, default=4)
    ap.add_argument("--skip_step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vq_restart needs a HIP device"
    import bench
    K, D = bench.NET["n_embed"], bench.NET["embed_dim"]
    M = args.batch * 10 * 14 * 10      # latent rows of the 160 x 224 x 160 volume behind four stride-2 levels
    out = {"K": K, "D": D, "M": M, "R": 32, "kernels": kernel_times(K, D, M, 32, args.calls, args.reps)}
    if not args.skip_step:
        out["training_step"] = step_times(args.batch, args.block, args.step_reps)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
