"""Cost of ff_dropout / attn_dropout on the production Performer training step (bench.py's PERF configuration: batch 6, raster-ordered 10 x 14 x 10 latents
= 1 400 tokens, 24 layers, 16 heads of which 8 local, window 420, ReZero, bf16): the same network at p = 0 and at ff_dropout = attn_dropout = P, timed in
alternating rounds in one process.

    python tools/bench_dropout.py [--p 0.1] [--rounds 4] [--steps 10] [--warmup 3]

Prints one JSON line: tokens/s of each setting (median over rounds) and their ratio."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from bench import PERF
    from synthanatomy_amd.losses.transformer import CELoss
    from synthanatomy_amd.networks.transformers.img2seq_ordering import Ordering
    from synthanatomy_amd.networks.transformers.performer import Performer
    from synthanatomy_amd.runtime.optim import FlatParams, FusedAdam

    dev = torch.device("cuda:0")
    spatial = PERF["spatial"]
    N = spatial[0] * spatial[1] * spatial[2]
    B = args.batch
    order = Ordering("raster_scan", 3, (1,) + spatial, (False, False, False), ((2, 0, 1),), ((0, 1),), ("rotate_90", "transpose"))
    gen = torch.Generator(device=dev).manual_seed(4)
    codes = torch.randint(0, PERF["vocab"], (B, N), generator=gen, device=dev)
    seq = codes[:, torch.as_tensor(order.get_sequence_ordering(), device=dev)]
    seq = torch.nn.functional.pad(seq, (1, 0), value=PERF["vocab"])
    x_in, x_tgt = seq[:, :-1].contiguous(), seq[:, 1:].contiguous()
    loss_fn = CELoss()
    runs = {}
    for p in (0.0, args.p):
        torch.manual_seed(4)
        net = Performer(num_tokens=PERF["vocab"] + 1, max_seq_len=N + 1, dim=PERF["dim"], depth=PERF["depth"], heads=PERF["heads"], ordering=order,
                        local_attn_heads=PERF["local_heads"], local_window_size=PERF["window"], feature_redraw_interval=1, use_rezero=True,
                        spatial_position_emb="absolute", spatial_shape=spatial, compute_dtype=torch.bfloat16, ff_dropout=p, attn_dropout=p).to(dev).train()
        flat = FlatParams(net.parameters())
        opt = FusedAdam(flat, lr=1e-3)
        opt.on_step.append(net.invalidate_packed_weights)

        def step(net=net, flat=flat, opt=opt):
            flat.zero_grad()
            loss = loss_fn(net(x_in).transpose(1, 2), x_tgt)
            loss.backward()
            opt.step()

        for _ in range(args.warmup):
            step()
        runs[p] = step
    torch.cuda.synchronize()
    tps = {p: [] for p in runs}
    for _ in range(args.rounds):
        for p, step in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            tps[p].append(B * N * args.steps / (time.perf_counter() - t0))
    med = {p: statistics.median(v) for p, v in tps.items()}
    print(json.dumps({"tokens_per_s_p0": round(med[0.0], 1), f"tokens_per_s_p{args.p}": round(med[args.p], 1), "ratio": round(med[args.p] / med[0.0], 4),
                      "rounds": {str(p): [round(x, 1) for x in v] for p, v in tps.items()}, "batch": B, "tokens": N}))


if __name__ == "__main__":
    main()
