#!/usr/bin/env python3
"""Merge the two upstream weight files of LPIPS-alex into the one file ``run_vqvae.py --perceptual_weights=<file>`` reads:

    python tools/make_lpips_weights.py --alexnet alexnet-owt-7be5be79.pth --lpips weights/v0.1/alex.pth --out lpips_alex.pth

* ``--alexnet``: torchvision's AlexNet checkpoint (keys ``features.{0,3,6,8,10}.weight|bias``; the classifier is ignored);
* ``--lpips``: the lpips package's ``weights/v0.1/alex.pth`` (keys ``lin{0..4}.model.1.weight``).

With ``--net=squeeze`` the same for LPIPS-squeeze (``--loss=baseline``, ``lpips_kwargs net='squeeze'``):

    python tools/make_lpips_weights.py --net=squeeze --backbone squeezenet1_1-b8a52dc0.pth --lpips weights/v0.1/squeeze.pth --out lpips_squeeze.pth

* ``--backbone`` (an alias of ``--alexnet``): torchvision's SqueezeNet-1.1 checkpoint (keys ``features.0.weight|bias`` and
  ``features.{3,4,6,7,9,10,11,12}.{squeeze,expand1x1,expand3x3}.weight|bias``; the classifier is ignored);
* ``--lpips``: the lpips package's ``weights/v0.1/squeeze.pth`` (keys ``lin{0..6}.model.1.weight``).

The output is a ``torch.save``d dict in the key layout of ``lpips.LPIPS(net='alex').state_dict()``: ``net.slice{1..5}.{0,3,6,8,10}.weight|bias``,
``lin{0..4}.model.1.weight`` and the scaling layer's constants.  Host only; it runs wherever the two files already are and never fetches anything."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synthanatomy_amd.losses import lpips, lpips_squeeze  # noqa: E402

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


def merge_squeeze(backbone: dict, lins: dict) -> dict:
    out = {}
    pairs = [("features.0", lpips_squeeze.CONV1_KEY)]
    pairs += [(f"features.{feat}.{part}", f"{key}.{part}") for feat, key, *_ in lpips_squeeze.FIRES for part in ("squeeze", "expand1x1", "expand3x3")]
    for src_key, dst_key in pairs:
        for p in ("weight", "bias"):
            src = f"{src_key}.{p}"
            if src not in backbone:
                raise ValueError(f"--backbone: key {src!r} is missing (expected torchvision's squeezenet1_1 state dict)")
            out[f"{dst_key}.{p}"] = backbone[src]
    for key in lpips_squeeze.LIN_KEYS:
        if key not in lins:
            raise ValueError(f"--lpips: key {key!r} is missing (expected lpips' weights/v0.1/squeeze.pth)")
        out[key] = lins[key]
    out["scaling_layer.shift"] = torch.tensor(lpips.SHIFT).view(1, 3, 1, 1)
    out["scaling_layer.scale"] = torch.tensor(lpips.SCALE).view(1, 3, 1, 1)
    checked = lpips_squeeze.validate_state_dict(out, "(merged)")      # names and shapes, as the loader will check them
    out.update({k: checked[k] for k in lpips_squeeze.expected_shapes()})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--net", choices=("alex", "squeeze"), default="alex")
    ap.add_argument("--alexnet", "--backbone", dest="alexnet", required=True)
    ap.add_argument("--lpips", required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args(argv)
    try:
        merged = (merge_squeeze if a.net == "squeeze" else merge)(torch.load(a.alexnet, map_location="cpu", weights_only=True), torch.load(a.lpips, map_location="cpu", weights_only=True))
    except ValueError as e:
        print(f"make_lpips_weights: {e}", file=sys.stderr)
        return 1
    torch.save(merged, a.out)
    print(f"wrote {a.out}: {len(merged)} tensors")
    return 0


if __name__ == "__main__":
    sys.exit(main())
