"""Launch geometries of a convolution / transposed convolution from its (kernel, stride, padding, output_padding, dilation) tuple.

Pure integer arithmetic: no torch, no library (tests/test_sampling_geometry_cpu.py walks it on the CPU).  ``engine.ConvOp`` turns every class
returned here into one ``sa_conv_geom``: grid index m and tap j read input ``m * in_mult + j * tap_step + in_off`` (zero outside) and write
output ``m * out_mult + out_off``; tap j is the layer's weight tap ``taps[j]``.

Both layer kinds relate a FINE axis (conv input / convT output, extent F) to a COARSE one (conv output / convT input, extent C) through
``f = c * s - p + t * d``, and every launch is one of two forms:

* window  -- rows are coarse voxels, each gathers its k taps from the fine side: conv forward / weight gradient, convT data gradient.
* residue -- rows are the fine voxels ``f = s * m + r`` of one class r in [0, s), each gathers from the coarse side the taps with
  ``(r + p - t * d) = 0 (mod s)``: t = t0 + j * s / gcd(s, d), which read ``c = m + (r + p - t0 * d) / s - j * d / gcd(s, d)``:
  conv data gradient, convT forward / weight gradient.  Every fine voxel belongs to exactly one class, so voxels no window reads (or the
  ``output_padding`` planes of a transposed convolution) come out as zero (+ bias) without a separate fill.
"""
from __future__ import annotations

from math import gcd
from typing import Dict, List, Optional, Tuple

MAX_KERNEL = 4      # SA_MAX_TAPS = 64 bounds k^3


def _name(kind, k, s, p, op, d):
    return f"{kind} (kernel {k}, stride {s}, padding {p}, " + (f"output_padding {op}, " if kind == "convT" else "") + f"dilation {d})"


def check_tuple(kind: str, k: int, s: int, p: int, op: int = 0, d: int = 1, flag: Optional[str] = None) -> None:
    """ValueError for tuples torch itself rejects (naming `flag`), NotImplementedError for legal ones outside the planner's rule."""
    assert kind in ("conv", "convT")
    what = (flag + " " if flag else "") + str((k, s, p, op, d) if kind == "convT" else (k, s, p, d)) + ": " + _name(kind, k, s, p, op, d)
    if k < 1 or s < 1 or d < 1 or p < 0 or op < 0:
        raise ValueError(f"{what}: kernel, stride and dilation must be positive, padding and output_padding non-negative")
    if kind == "convT" and op >= max(s, d):
        raise ValueError(f"{what}: output_padding must be smaller than either stride or dilation")
    if kind == "conv" and op != 0:
        raise ValueError(f"{what}: a convolution has no output_padding")
    if k > MAX_KERNEL:
        raise NotImplementedError(f"{what}: kernels of 1 .. {MAX_KERNEL} taps per axis ({MAX_KERNEL ** 3} taps per launch)")
    if s > 2:
        raise NotImplementedError(f"{what}: stride 1 or 2")
    for r in range(s):
        if not any((r + p - t * d) % s == 0 for t in range(k)):
            raise NotImplementedError(f"{what}: residue class {r} of the stride owns no tap (stride 2 needs kernel >= 2 and an odd dilation)")


def out_size(kind: str, k: int, s: int, p: int, op: int, d: int, I: int) -> int:
    if kind == "conv":
        return (I + 2 * p - d * (k - 1) - 1) // s + 1
    return (I - 1) * s - 2 * p + d * (k - 1) + op + 1


def window_axis(k: int, s: int, p: int, d: int, C: int) -> List[Dict]:
    """rows = coarse voxels (one class)"""
    return [dict(grid=C, in_mult=s, tap_step=d, in_off=-p, out_mult=1, out_off=0, taps=list(range(k)))]


def residue_axis(k: int, s: int, p: int, d: int, F: int) -> List[Dict]:
    """rows = fine voxels, one class per residue r of the stride (classes without voxels are left out)"""
    g = gcd(s, d)
    out = []
    for r in range(s):
        grid = (F - r + s - 1) // s
        if grid <= 0:
            continue
        t0 = next((t for t in range(k) if (r + p - t * d) % s == 0), None)
        if t0 is None:
            raise NotImplementedError(f"residue class {r} of stride {s} owns no tap of kernel {k}, padding {p}, dilation {d}")
        out.append(dict(grid=grid, in_mult=1, tap_step=-(d // g), in_off=(r + p - t0 * d) // s, out_mult=s, out_off=r, taps=list(range(t0, k, s // g))))
    return out


def _product(axes: List[List[Dict]], k: int, in_dims, out_dims) -> List[Dict]:
    res = []
    for a in axes[0]:
        for b in axes[1]:
            for c in axes[2]:
                abc = (a, b, c)
                lut = [(td * k + th) * k + tw for td in a["taps"] for th in b["taps"] for tw in c["taps"]]
                cls = {key: tuple(x[key] for x in abc) for key in ("grid", "in_mult", "tap_step", "in_off", "out_mult", "out_off")}
                cls["KT"] = tuple(len(x["taps"]) for x in abc)
                cls["lut"] = None if lut == list(range(k ** 3)) else lut
                cls["in_dims"], cls["out_dims"] = tuple(in_dims), tuple(out_dims)
                res.append(cls)
    return res


def plan(kind: str, k: int, s: int, p: int, op: int, d: int, idims: Tuple[int, int, int]) -> Dict:
    """{"odims", "fwd", "dgrad", "wgrad"}: lists of classes.  fwd / wgrad read the layer's input and are laid over its output; dgrad reads the
    output gradient and is laid over the input."""
    check_tuple(kind, k, s, p, op, d)
    idims = tuple(int(i) for i in idims)
    odims = tuple(out_size(kind, k, s, p, op, d, i) for i in idims)
    if min(odims) < 1 or min(idims) < 1:
        raise ValueError(f"{_name(kind, k, s, p, op, d)} on extents {idims}: output size {odims} is too small")
    if kind == "conv":
        fwd = _product([window_axis(k, s, p, d, o) for o in odims], k, idims, odims)
        dgr = _product([residue_axis(k, s, p, d, i) for i in idims], k, odims, idims)
    else:
        fwd = _product([residue_axis(k, s, p, d, o) for o in odims], k, idims, odims)
        dgr = _product([window_axis(k, s, p, d, i) for i in idims], k, odims, idims)
    return {"odims": odims, "fwd": fwd, "dgrad": dgr, "wgrad": fwd}


def triples(classes: List[Dict]):
    """every (row voxel written, weight tap, voxel read) the classes generate, as ((o_d, o_h, o_w), tap, (i_d, i_h, i_w)) -- reads outside
    `in_dims` contribute nothing and are left out; rows outside `out_dims` are a planner error"""
    for c in classes:
        k3 = c["lut"]
        KT = c["KT"]
        for md in range(c["grid"][0]):
            for mh in range(c["grid"][1]):
                for mw in range(c["grid"][2]):
                    m = (md, mh, mw)
                    o = tuple(m[a] * c["out_mult"][a] + c["out_off"][a] for a in range(3))
                    assert all(0 <= o[a] < c["out_dims"][a] for a in range(3)), (c, m)
                    j = 0
                    for td in range(KT[0]):
                        for th in range(KT[1]):
                            for tw in range(KT[2]):
                                t = (td, th, tw)
                                i = tuple(m[a] * c["in_mult"][a] + t[a] * c["tap_step"][a] + c["in_off"][a] for a in range(3))
                                tap = k3[j] if k3 is not None else j
                                j += 1
                                if all(0 <= i[a] < c["in_dims"][a] for a in range(3)):
                                    yield o, tap, i
