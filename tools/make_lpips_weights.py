#!/usr/bin/env python3
"""Merge the two upstream weight files of LPIPS-alex into the one file ``run_vqvae.py --perceptual_weights=<file>`` reads:

    python tools/make_lpips_weights.py --alexnet alexnet-owt-7be5be79.pth --lpips weights/v0.1/alex.pth --out lpips_alex.pth

* ``--alexnet``: torchvision's AlexNet checkpoint (keys ``features.{0,3,6,8,10}.weight|bias``; the classifier is ignored);
* ``--lpips``: the lpips package's ``weights/v0.1/alex.pth`` (keys ``lin{0..4}.model.1.weight``).

The output is a ``torch.save``d dict in the key layout of ``lpips.LPIPS(net='alex').state_dict()``: ``net.slice{1..5}.{0,3,6,8,10}.weight|bias``,
``lin{0..4}.model.1.weight`` and the scaling layer's constants.  Host only; it runs wherever the two files already are and never fetches anything."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synthanatomy_amd.losses import lpips  # noqa: E402

FEATURES = (0, 3, 6, 8, 10)


def merge(alexnet: dict, lins: dict) -> dict:
    out = {}
    for idx, key in zip(FEATURES, lpips.CONV_KEYS):
        for p in ("weight", "bias"):
            src = f"features.{idx}.{p}"
            if src not in alexnet:
                raise ValueError(f"--alexnet: key {src!r} is missing (expected torchvision's alexnet state dict)")
            out[f"{key}.{p}"] = alexnet[src]
    for key in lpips.LIN_KEYS:
        if key not in lins:
            raise ValueError(f"--lpips: key {key!r} is missing (expected lpips' weights/v0.1/alex.pth)")
        out[key] = lins[key]
    out["scaling_layer.shift"] = torch.tensor(lpips.SHIFT).view(1, 3, 1, 1)
    out["scaling_layer.scale"] = torch.tensor(lpips.SCALE).view(1, 3, 1, 1)
    checked = lpips.validate_state_dict(out, "(merged)")      # names and shapes, as the loader will check them
    out.update({k: checked[k] for k in lpips.expected_shapes()})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--alexnet", required=True)
    ap.add_argument("--lpips", required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args(argv)
    try:
        merged = merge(torch.load(a.alexnet, map_location="cpu", weights_only=True), torch.load(a.lpips, map_location="cpu", weights_only=True))
    except ValueError as e:
        print(f"make_lpips_weights: {e}", file=sys.stderr)
        return 1
    torch.save(merged, a.out)
    print(f"wrote {a.out}: {len(merged)} tensors")
    return 0


if __name__ == "__main__":
    sys.exit(main())
