"""Cost of generalized (ReLU) attention on the bench Performer (bench.py's PERF configuration: 24 layers, dim 512, 16 heads of which 8 local, window 420,
raster-ordered 10 x 14 x 10 latents = 1 400 tokens, ReZero, bf16; batch 6) in ONE process, so that all three see the same box:

  generalized      generalized_attention=True: phi = relu(dd) + 1e-3 on the chunked route (csrc/favor_generalized.hip), sa_favor_generalized_step when decoding
  softmax_chunked  the softmax map on the SAME chunked route (SA_NO_FUSED_FAVOR=1: feature maps in HBM, local heads in launches of their own)
  softmax_fused    the default: the softmax map recomputed on chip (csrc/favor_fused.hip), local heads riding in the FAVOR+ launches

each timed for one training step (forward, cross entropy, backward; no optimizer) and for one stateful sample() with the captured per-token graph.

    python tools/bench_generalized_attention.py [--batch 6] [--rounds 5] [--out profiles/generalized_attention_bench_line.json]

Device events around every call, one warm-up call of each kind (weight packing, workspace sizing, graph capture), the kinds alternate inside a round, the
median over ``--rounds``.  Run it under a time limit (``timeout -k 10 600 python tools/bench_generalized_attention.py``).  Prints one JSON line and writes it
to ``--out`` when given."""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from bench import PERF
    from synthanatomy_amd import debug
    from synthanatomy_amd.losses.transformer import CELoss
    from synthanatomy_amd.networks.transformers.img2seq_ordering import Ordering
    from synthanatomy_amd.networks.transformers.performer import Performer

    dev = torch.device("cuda:0")
    spatial = PERF["spatial"]
    N = spatial[0] * spatial[1] * spatial[2]
    B = args.batch
    order = Ordering("raster_scan", 3, (1,) + spatial, (False, False, False), ((2, 0, 1),), ((0, 1),), ("rotate_90", "transpose"))

    def network(generalized):
        torch.manual_seed(4)
        return Performer(num_tokens=PERF["vocab"] + 1, max_seq_len=N + 1, dim=PERF["dim"], depth=PERF["depth"], heads=PERF["heads"], ordering=order,
                         local_attn_heads=PERF["local_heads"], local_window_size=PERF["window"], feature_redraw_interval=None, use_rezero=True,
                         spatial_position_emb="absolute", spatial_shape=spatial, compute_dtype=torch.bfloat16, generalized_attention=generalized).to(dev)

    nets = {True: network(True), False: network(False)}
    g = torch.Generator().manual_seed(4)
    tok = torch.randint(0, PERF["vocab"] + 1, (B, N), generator=g).to(dev)
    tgt = torch.randint(0, PERF["vocab"], (B, N), generator=g).to(dev)
    prefix = torch.full((B, 1), PERF["vocab"], dtype=torch.long, device=dev)
    loss_fn = CELoss()

    def train(net, chunked):
        net.train()
        net.zero_grad(set_to_none=True)
        with debug.override(no_fused_favor=chunked):
            loss = loss_fn(net(tok).transpose(1, 2), tgt)
            loss.backward()
        return float(loss.detach())

    def sample(net):
        with torch.no_grad():
            return net.sample(prefix, sample=True, use_graph=True)

    kinds = {"train_generalized": lambda: train(nets[True], False), "train_softmax_chunked": lambda: train(nets[False], True),
             "train_softmax_fused": lambda: train(nets[False], False), "sample_generalized": lambda: sample(nets[True]),
             "sample_softmax": lambda: sample(nets[False])}      # (the decode step has one softmax form: sa_attn_step)
    ms = {k: [] for k in kinds}
    losses = {}
    for name, fn in kinds.items():      # warm-up
        _, out = _timed(fn)
        if name.startswith("train"):
            losses[name] = round(out, 5)
        print(f"warm-up {name} done", flush=True)
    for r in range(args.rounds):
        for name, fn in kinds.items():
            ms[name].append(_timed(fn)[0])
            print(f"round {r} {name}: {ms[name][-1]:.1f} ms", flush=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    line = {"metric": "performer_generalized_attention", "unit": "ms (median)", "median_ms": {k: round(v, 2) for k, v in med.items()},
            "train_tokens_per_s": {k[len("train_"):]: round(B * N / (v * 1e-3), 1) for k, v in med.items() if k.startswith("train_")},
            "sample_tokens_per_s": {k[len("sample_"):]: round(B * N / (v * 1e-3), 1) for k, v in med.items() if k.startswith("sample_")},
            "generalized_over_softmax_chunked_train": round(med["train_generalized"] / med["train_softmax_chunked"], 4),
            "generalized_over_softmax_fused_train": round(med["train_generalized"] / med["train_softmax_fused"], 4),
            "generalized_over_softmax_sample": round(med["sample_generalized"] / med["sample_softmax"], 4),
            "first_loss": losses, "ms": {k: [round(x, 1) for x in v] for k, v in ms.items()}, "batch": B, "tokens": N, "layers": PERF["depth"],
            "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
