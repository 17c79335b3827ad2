"""Throughput of ``Performer.heal`` against ``Performer.sample`` on the bench Performer (bench.py's PERF configuration: 24 layers, dim 512, 16 heads of
which 8 local, window 420, raster-ordered 10 x 14 x 10 latents = 1 400 tokens, ReZero, bf16; batch 6) in ONE process, so that both see the same box:

  sample        the stateful O(N) sampler (sa_sample_step closes each step)
  heal_score    heal(codes): every token scored, none replaced (sa_heal_step with log_threshold = -inf: the draw is skipped)
  heal_replace  heal(codes, threshold=1 / vocabulary): an untrained network is close to uniform, so about half of the tokens are redrawn

each with the captured per-token graph and with eager launches (``use_graph=False``).

    python tools/bench_healing.py [--batch 6] [--rounds 3] [--out profiles/healing_bench_line.json]

Device events around every run, one warm-up run of each kind (graph capture, weight packing, workspace sizing), the median over ``--rounds``.  Run it
under a time limit (``timeout -k 10 600 python tools/bench_healing.py``).  Prints one JSON line and writes it to ``--out`` when given."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn):
    """milliseconds of fn() between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from bench import PERF
    from synthanatomy_amd.networks.transformers.img2seq_ordering import Ordering
    from synthanatomy_amd.networks.transformers.performer import Performer

    dev = torch.device("cuda:0")
    spatial = PERF["spatial"]
    N = spatial[0] * spatial[1] * spatial[2]
    B = args.batch
    order = Ordering("raster_scan", 3, (1,) + spatial, (False, False, False), ((2, 0, 1),), ((0, 1),), ("rotate_90", "transpose"))
    torch.manual_seed(4)
    net = Performer(num_tokens=PERF["vocab"] + 1, max_seq_len=N + 1, dim=PERF["dim"], depth=PERF["depth"], heads=PERF["heads"], ordering=order,
                    local_attn_heads=PERF["local_heads"], local_window_size=PERF["window"], feature_redraw_interval=1, use_rezero=True,
                    spatial_position_emb="absolute", spatial_shape=spatial, compute_dtype=torch.bfloat16).to(dev).eval()
    prefix = torch.full((B, 1), PERF["vocab"], dtype=torch.long, device=dev)
    codes = torch.randint(0, PERF["vocab"], (B, *spatial), generator=torch.Generator().manual_seed(4)).to(dev)
    tau = 1.0 / PERF["vocab"]
    kinds = {}
    for tag, graph in (("graph", True), ("eager", False)):
        kinds[f"sample_{tag}"] = lambda g=graph: net.sample(prefix, sample=True, use_graph=g)
        kinds[f"heal_score_{tag}"] = lambda g=graph: net.heal(codes, sample=True, use_graph=g)
        kinds[f"heal_replace_{tag}"] = lambda g=graph: net.heal(codes, threshold=tau, sample=True, use_graph=g)
    ms = {k: [] for k in kinds}
    replaced = None
    with torch.no_grad():
        for name, fn in kinds.items():      # warm-up
            _, out = _timed(fn)
            if name == "heal_replace_graph":
                replaced = float(out[2].float().mean())
            print(f"warm-up {name} done", flush=True)
        for r in range(args.rounds):
            for name, fn in kinds.items():
                ms[name].append(_timed(fn)[0])
                print(f"round {r} {name}: {ms[name][-1]:.1f} ms", flush=True)
    tps = {k: B * N / (statistics.median(v) * 1e-3) for k, v in ms.items()}
    line = {"metric": "performer_healing_tokens_per_sec", "unit": "tokens/s", "tokens_per_s": {k: round(v, 1) for k, v in tps.items()},
            "heal_over_sample": {t: {k: round(tps[f"{k}_{t}"] / tps[f"sample_{t}"], 4) for k in ("heal_score", "heal_replace")} for t in ("graph", "eager")},
            "fraction_replaced_at_tau": round(replaced, 4), "tau": tau, "ms": {k: [round(x, 1) for x in v] for k, v in ms.items()}, "batch": B, "tokens": N,
            "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
