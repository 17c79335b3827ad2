"""The 2.5D LPIPS-alex perceptual term of ``PerceptualLoss`` / ``JukeboxPerceptualLoss`` / ``HartleyPerceptualLoss`` (reference
src/losses/vqvae/vqvae.py:931-988) on HIP: weights, the slice draw, the launch chain and its ``autograd.Function``.  DESIGN.md section 7.12.

The arithmetic restates ``lpips.LPIPS(net='alex', version='0.1', lpips=True, spatial=False)`` in ``eval()`` mode from its published description
(the package is not a dependency): it is UNPINNED against upstream, like the Performer.  Two deliberate choices, both in csrc/lpips.hip:

* the padding rule -- the scaling layer's shift is folded into conv1, and the border classes of ``sa_lpips_unfold`` keep the fold exact where
  conv1's zero padding (applied AFTER scaling upstream) is read;
* the subgradient at zero -- where the prediction's feature vector is all zero, the normalisation's projection term is dropped (upstream: NaN).
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _ffi
from ..engine import ConvOp, make_geom

# (cin, cout, kernel, stride, padding) of torchvision's AlexNet features and their state-dict prefixes in lpips.LPIPS(net='alex')
ALEX_CONVS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
CONV_KEYS = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")
LIN_KEYS = tuple(f"lin{i}.model.1.weight" for i in range(5))
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
MIN_SIDE = 31                       # the smallest slice side for which the second pool still has an output
UNFOLD_LD = 136                     # 121 taps + 9 border classes, rounded up to 16 bytes in bf16
WORKSPACE_CAP = 1 << 30             # bytes of activations + gradients one chunk of slices may hold
DEFAULT_LPIPS_KWARGS = {"pretrained": True, "net": "alex", "version": "0.1", "lpips": True, "spatial": False, "pnet_rand": False, "pnet_tune": False,
                        "use_dropout": True, "model_path": None, "eval_mode": True, "verbose": False}


def expected_shapes() -> Dict[str, Tuple[int, ...]]:
    shapes = {}
    for key, (ci, co, k, _, _) in zip(CONV_KEYS, ALEX_CONVS):
        shapes[key + ".weight"] = (co, ci, k, k)
        shapes[key + ".bias"] = (co,)
    for key, (_, co, _, _, _) in zip(LIN_KEYS, ALEX_CONVS):
        shapes[key] = (1, co, 1, 1)
    return shapes


def _draw_state_dict(seed: int, shapes: Dict[str, Tuple[int, ...]]) -> Dict[str, torch.Tensor]:
    """one seeded draw in the order of ``shapes``: He-scaled convolutions, small biases, NON-NEGATIVE lin weights (as the trained ones are)"""
    gen = torch.Generator().manual_seed(int(seed))
    sd = {}
    for key, shape in shapes.items():
        if key.startswith("lin"):
            sd[key] = torch.rand(shape, generator=gen, dtype=torch.float64).float()
        elif key.endswith(".weight"):
            fan = shape[1] * shape[2] * shape[3]
            sd[key] = torch.randn(shape, generator=gen, dtype=torch.float64).mul_((2.0 / fan) ** 0.5).float()
        else:
            sd[key] = torch.randn(shape, generator=gen, dtype=torch.float64).mul_(0.1).float()
    return sd


def _validate_layout(sd, source: str, shapes: Dict[str, Tuple[int, ...]], net: str, tool: str, foreign_keys: Sequence[str], foreign: str):
    """The tensors of ``shapes`` from a state dict, checked by name and shape (``ValueError`` naming the key), + the scaling layer (the published constants
    when the file has none).  A file that holds one of ``foreign_keys`` belongs to the other network and is refused with ``foreign``."""
    if not isinstance(sd, dict):
        raise ValueError(f"--perceptual_weights {source}: expected a torch.save'd dict of tensors, got {type(sd).__name__}")
    if any(key in sd for key in foreign_keys):
        raise ValueError(f"--perceptual_weights {source}: {foreign}")
    out = {}
    for key, shape in shapes.items():
        if key not in sd:
            raise ValueError(f"--perceptual_weights {source}: key {key!r} is missing (expected the layout of lpips.LPIPS(net={net!r}).state_dict(); "
                             f"{tool} builds it from the two upstream files)")
        t = sd[key]
        if not torch.is_tensor(t) or tuple(t.shape) != shape:
            raise ValueError(f"--perceptual_weights {source}: {key!r} has shape {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}, expected {shape}")
        out[key] = t.detach().float().cpu().contiguous()
    for key, default in (("scaling_layer.shift", SHIFT), ("scaling_layer.scale", SCALE)):
        if key in sd:
            t = sd[key]
            if not torch.is_tensor(t) or t.numel() != 3:
                raise ValueError(f"--perceptual_weights {source}: {key!r} must hold 3 values")
            out[key] = t.detach().double().reshape(3).cpu()
        else:
            out[key] = torch.tensor(default, dtype=torch.float64)
    return out


def random_state_dict(seed: int) -> Dict[str, torch.Tensor]:
    """Seeded stand-in weights in the key layout of ``lpips.LPIPS(net='alex').state_dict()``.  For tests, smoke runs and benchmarks only -- the distances
    mean nothing."""
    return _draw_state_dict(seed, expected_shapes())


def validate_state_dict(sd, source: str) -> Dict[str, torch.Tensor]:
    """The tensors this build needs from an LPIPS-alex state dict; an LPIPS-squeeze file is refused as such."""
    return _validate_layout(sd, source, expected_shapes(), "alex", "tools/make_lpips_weights.py", ("net.slice2.3.squeeze.weight",),
                            "this is an LPIPS-squeeze file (it holds 'net.slice2.3.squeeze.weight'); it serves --loss=baseline "
                            "and lpips_kwargs net='squeeze', not the LPIPS-alex losses")


def load_weights(spec: str, net: str = "alex") -> Dict[str, torch.Tensor]:
    """``random:<seed>`` or the path of a ``torch.save``d state dict in the layout of ``net`` ("alex" | "squeeze", the latter in losses/lpips_squeeze.py).
    Host only: nothing touches the device."""
    if net == "squeeze":
        from . import lpips_squeeze
        validate, draw = lpips_squeeze.validate_state_dict, lpips_squeeze.random_state_dict
    elif net == "alex":
        validate, draw = validate_state_dict, random_state_dict
    else:
        raise ValueError(f"--perceptual_weights: no LPIPS network {net!r} in this build (alex, squeeze)")
    if not isinstance(spec, str) or not spec:
        raise ValueError(f"--perceptual_weights must be a file or random:<seed>; got {spec!r}")
    if spec.startswith("random:"):
        try:
            seed = int(spec[len("random:"):])
        except ValueError:
            raise ValueError(f"--perceptual_weights {spec!r}: the seed after 'random:' must be an integer") from None
        return validate(draw(seed), spec)
    if not os.path.isfile(spec):
        raise ValueError(f"--perceptual_weights {spec!r}: no such file")
    try:
        sd = torch.load(spec, map_location="cpu", weights_only=True)
    except Exception as e:      # noqa: BLE001 -- whatever the unpickler raises, the flag is named
        raise ValueError(f"--perceptual_weights {spec!r}: cannot be read as a torch.save'd state dict ({type(e).__name__}: {e})") from e
    return validate(sd, spec)


def draw_slices(seed: int, step: int, view: int, n_slices: int, n_keep: int) -> np.ndarray:
    """The kept slice ids of one 2.5D view, int32 and sorted: ``n_keep`` of ``n_slices`` without replacement, keyed on (seed, step, view) -- the
    project's own draw (upstream: ``torch.randperm`` on the device), drawn on the host so that a resumed run reproduces it."""
    if n_keep >= n_slices:
        return np.arange(n_slices, dtype=np.int32)
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF, int(view)])))
    return np.sort(rng.permutation(n_slices)[:n_keep]).astype(np.int32)


def conv1_extent(e: int) -> int:
    return (e + 2 * 2 - 11) // 4 + 1


def pool_extent(e: int) -> int:
    return (e - 3) // 2 + 1


def ceil_pool_extent(e: int) -> int:
    """MaxPool2d(3, 2, ceil_mode=True): ceil((e - 3) / 2) + 1, minus one if the last window would start outside the input"""
    o = -(-(e - 3) // 2) + 1
    return o - 1 if (o - 1) * 2 >= e else o


def slice_sides(shape, view: int) -> Tuple[int, int]:
    """(h, w) of the slices of one 2.5D view of a volume [B, 1, D, H, W]"""
    _, _, D, H, W = shape
    return ((H, W), (D, W), (D, H))[view]


def folded_conv1(w: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, h: int, w_: int) -> torch.Tensor:
    """conv1 of the scaled 3-channel image as ONE [64, UNFOLD_LD] matrix over the columns of ``sa_lpips_unfold`` (float64).  Columns 0 .. 120:
    ``sum_c W[o, c, t] / scale_c``.  Columns 121 + 3 cH + cW: ``- sum over the taps INSIDE the image for that border class of sum_c W[o, c, t]
    shift_c / scale_c`` -- upstream pads the SCALED image with zeros, so a padded tap must not contribute ``-shift / scale`` (the padding rule)."""
    w = w.double()
    m = torch.zeros(w.shape[0], UNFOLD_LD, dtype=torch.float64)
    m[:, :121] = (w / scale.view(1, 3, 1, 1)).sum(1).reshape(-1, 121)
    b = (w * (shift / scale).view(1, 3, 1, 1)).sum(1)                  # [64, 11, 11]

    def inside(cls, extent):       # taps of a window that starts at -2 (class 1), ends after the image (class 2), or lies inside (class 0)
        t = torch.arange(11)
        if cls == 1:
            return t >= 2
        if cls == 2:
            last = (conv1_extent(extent) - 1) * 4 - 2
            return last + t < extent
        return torch.ones(11, dtype=torch.bool)

    for ch in range(3):
        for cw in range(3):
            keep = (inside(ch, h)[:, None] & inside(cw, w_)[None, :]).double()
            m[:, 121 + 3 * ch + cw] = -(b * keep).sum((1, 2))
    return m


class Conv2dOp:
    """A stride-1 "same" 2-D convolution ([Cout, Cin, k, k], padding (k - 1) / 2) over channels-last slices [N, h, w, C] on ``sa_conv_fprop``: the 2-D
    geometry is a 3-D one with Di = Dm = Do = 1 and KT = {1, k, k}.  Forward with bias + ReLU, data gradient with addend + ReLU mask.  Frozen weights:
    both operands are packed once per device and dtype."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor], dtype: torch.dtype):
        co, ci, k, k2 = weight.shape
        assert k == k2 and k % 2 == 1 and k * k <= _ffi.MAX_TAPS
        self.weight, self.bias, self.dtype = weight.contiguous(), bias, dtype
        self.cin, self.cout, self.k, self.pad = ci, co, k, (k - 1) // 2
        self._wpk = {}
        self._bias_pad = None
        if bias is not None:
            self._bias_pad = torch.zeros(-(-co // 128) * 128, dtype=torch.float32, device=weight.device)
            self._bias_pad[:co] = bias

    def _geom(self, N, h, w, dgrad):
        k, p, T = self.k, self.pad, self.k * self.k
        if dgrad:
            g = make_geom(self.dtype, N, (1, h, w), (1, h, w), self.cout, (1, h, w), self.cin, self.cout, self.cin, (1, k, k), (1, 1, 1), (1, -1, -1),
                          (0, p, p), (1, 1, 1), (0, 0, 0))
            rows, red, s_row, s_red = self.cin, self.cout, T, self.cin * T
        else:
            g = make_geom(self.dtype, N, (1, h, w), (1, h, w), self.cin, (1, h, w), self.cout, self.cin, self.cout, (1, k, k), (1, 1, 1), (1, 1, 1),
                          (0, -p, -p), (1, 1, 1), (0, 0, 0))
            rows, red, s_row, s_red = self.cout, self.cin, self.cin * T, T
        key = (dgrad, g.CoutPad, g.Kpad)
        if key not in self._wpk:
            wpk = torch.empty(g.CoutPad * g.Kpad, dtype=self.dtype, device=self.weight.device)
            _ffi.check(_ffi.lib().sa_pack_weights(_ffi.ptr(self.weight), _ffi.ptr(wpk), _ffi.dtype_id(self.dtype), rows, red, T, None, s_row, s_red,
                                                  g.CoutPad, g.Cin, g.Kpad, _ffi.stream()), "sa_pack_weights")
            self._wpk[key] = wpk
        return g, self._wpk[key]

    def fprop(self, x: torch.Tensor, relu: bool = True) -> torch.Tensor:
        N, h, w, C = x.shape
        assert x.dtype == self.dtype and x.is_contiguous() and C == self.cin, (x.dtype, x.shape, self.cin)
        g, wpk = self._geom(N, h, w, False)
        out = torch.empty((N, h, w, self.cout), dtype=self.dtype, device=x.device)
        ep = ConvOp._epilogue(self._bias_pad, None, None, None, _ffi.ACT_RELU if relu else _ffi.ACT_NONE, _ffi.MASK_NONE, False, self.dtype, 0.0)
        _ffi.check(_ffi.lib().sa_conv_fprop(ctypes.byref(g), _ffi.dtype_id(self.dtype), _ffi.ptr(x), _ffi.ptr(wpk), _ffi.ptr(out), ctypes.byref(ep),
                                            _ffi.stream()), "sa_conv_fprop (2-D)")
        return out

    def dgrad(self, gy: torch.Tensor, addend: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, out_dtype=None) -> torch.Tensor:
        """d / d input from the gradient at the PRE-activation output; (+ addend) * (mask > 0) in the epilogue."""
        N, h, w, C = gy.shape
        assert gy.dtype == self.dtype and gy.is_contiguous() and C == self.cout, (gy.dtype, gy.shape, self.cout)
        out_dtype = out_dtype or self.dtype
        g, wpk = self._geom(N, h, w, True)
        out = torch.empty((N, h, w, self.cin), dtype=out_dtype, device=gy.device)
        ep = ConvOp._epilogue(None, addend, mask, None, _ffi.ACT_NONE, _ffi.MASK_POS, False, out_dtype, 0.0)
        _ffi.check(_ffi.lib().sa_conv_fprop(ctypes.byref(g), _ffi.dtype_id(self.dtype), _ffi.ptr(gy), _ffi.ptr(wpk), _ffi.ptr(out), ctypes.byref(ep),
                                            _ffi.stream()), "sa_conv_fprop (2-D data gradient)")
        return out


class LpipsNet(torch.nn.Module):
    """What the LPIPS networks of this build share: the compute dtype, the workspace cap, the operator cache, the two pool launches and the frame of
    ``view_term`` -- chunking, the distance accumulator and the head launches.  A network adds its frozen weights as NON-PERSISTENT buffers (no Parameter:
    nothing reaches an optimiser, a gradient reducer or a checkpoint) with ``lin0 .. lin{T-1}`` for its T taps, and

    * ``bytes_per_slice(h, w, esize)``: activations of both images + gradients of one, per kept slice (the chunk size follows from the workspace cap);
    * ``_features(y, y_pred, view, cid, normalize) -> (taps, saved)``: the tap feature maps [2 S, h, w, C] of one chunk -- target slices in the first
      half, the prediction's in the second -- and whatever ``_input_grad`` needs besides them;
    * ``_input_grad(gh, taps, saved, grad, view, cid, scale)``: grad += scale * (the heads' gradients ``gh`` at the prediction's taps, carried back to
      the kept slices ``cid`` of the volume)."""

    def __init__(self, compute_dtype: torch.dtype, workspace_cap: int):
        super().__init__()
        if compute_dtype not in (torch.float32, torch.bfloat16):
            raise NotImplementedError(f"LPIPS compute dtype must be float32 (parity) or bfloat16 (throughput); got {compute_dtype}")
        self.compute_dtype = compute_dtype
        self.workspace_cap = int(workspace_cap)
        self._ops = {}

    def _pool(self, x: torch.Tensor, ceil: bool):
        """MaxPool2d(3, 2, ceil_mode=ceil) of channels-last [N, hi, wi, C] and its argmax (uint8)"""
        N, hi, wi, C = x.shape
        extent, fn = (ceil_pool_extent, "sa_lpips_maxpool_ceil_fwd") if ceil else (pool_extent, "sa_lpips_maxpool_fwd")
        p = torch.empty((N, extent(hi), extent(wi), C), dtype=x.dtype, device=x.device)
        idx = torch.empty(p.shape, dtype=torch.uint8, device=x.device)
        _ffi.check(getattr(_ffi.lib(), fn)(_ffi.ptr(x), _ffi.dtype_id(x.dtype), _ffi.ptr(p), _ffi.ptr(idx), N, hi, wi, C, _ffi.stream()), fn)
        return p, idx

    def _unpool(self, gp: torch.Tensor, idx: torch.Tensor, addend: Optional[torch.Tensor], mask: Optional[torch.Tensor], shape, ceil: bool) -> torch.Tensor:
        """gradient at a pool's input [S, hi, wi, C] from the gradient at its output: (addend + the routed gp) * (mask > 0)"""
        _, hi, wi, C = shape
        fn = "sa_lpips_maxpool_ceil_bwd" if ceil else "sa_lpips_maxpool_bwd"
        gx = torch.empty((gp.shape[0], hi, wi, C), dtype=gp.dtype, device=gp.device)
        _ffi.check(getattr(_ffi.lib(), fn)(_ffi.ptr(gp), ctypes.c_void_p(idx.data_ptr()), _ffi.ptr(addend),
                                           ctypes.c_void_p(mask.data_ptr()) if mask is not None else None, _ffi.dtype_id(gp.dtype), _ffi.ptr(gx),
                                           gp.shape[0], hi, wi, C, _ffi.stream()), fn)
        return gx

    def view_term(self, y: torch.Tensor, y_pred: torch.Tensor, view: int, ids: torch.Tensor, grad: Optional[torch.Tensor], scale: float,
                  normalize: bool, chunk: Optional[int] = None) -> torch.Tensor:
        """d [S] fp32 = LPIPS(y slice, y_pred slice) for the kept slices ``ids`` (device int32) of ``view``; when ``grad`` (fp32 volume) is given,
        grad += scale * d sum(d) / d y_pred.  Per chunk: the network's forward launches, one head per tap and, with a gradient, its backward launches
        (the networks' ``_features`` give the counts)."""
        h, w = slice_sides(y.shape, view)
        d = torch.zeros(ids.numel(), dtype=torch.float32, device=y.device)
        if chunk is None:
            chunk = max(1, self.workspace_cap // self.bytes_per_slice(h, w, 2 if self.compute_dtype == torch.bfloat16 else 4))
        for lo in range(0, ids.numel(), chunk):      # (a call per chunk: its workspace is released before the next chunk allocates)
            self._chunk_term(y, y_pred, view, ids[lo:lo + chunk], d[lo:lo + chunk], grad, float(scale) * (2.0 if normalize else 1.0), normalize)
        return d

    def _chunk_term(self, y, y_pred, view, cid, dc, grad, scale, normalize):
        S, dt = cid.numel(), self.compute_dtype
        taps, saved = self._features(y, y_pred, view, cid, normalize)
        gh = []
        for l, f in enumerate(taps):
            _, hl, wl, C = f.shape
            g1 = torch.empty((S, hl, wl, C), dtype=dt, device=y.device) if grad is not None else None
            _ffi.check(_ffi.lib().sa_lpips_head(_ffi.ptr(f), ctypes.c_void_p(f[S:].data_ptr()), _ffi.dtype_id(dt), _ffi.ptr(getattr(self, f"lin{l}")), S, hl * wl,
                                                C, _ffi.ptr(dc), _ffi.ptr(g1), int(l == len(taps) - 1), _ffi.stream()), "sa_lpips_head")
            gh.append(g1)
        if grad is not None:
            self._input_grad(gh, taps, saved, grad, view, cid, scale)


class LpipsAlex(LpipsNet):
    """Frozen LPIPS-alex weights and the launch chain of the perceptual term over the kept slices of one view."""

    def __init__(self, weights: Dict[str, torch.Tensor], compute_dtype: torch.dtype = torch.float32, workspace_cap: int = WORKSPACE_CAP):
        super().__init__(compute_dtype, workspace_cap)
        for i, key in enumerate(CONV_KEYS):
            self.register_buffer(f"w{i}", weights[key + ".weight"].float().clone(), persistent=False)
            self.register_buffer(f"b{i}", weights[key + ".bias"].float().clone(), persistent=False)
        for i, key in enumerate(LIN_KEYS):
            self.register_buffer(f"lin{i}", weights[key].float().reshape(-1).clone(), persistent=False)
        self.register_buffer("shift", weights["scaling_layer.shift"].double().clone(), persistent=False)
        self.register_buffer("scale", weights["scaling_layer.scale"].double().clone(), persistent=False)

    def _conv(self, i: int, h: int = 0, w: int = 0) -> Conv2dOp:
        """layer i's operator on the buffers' device; conv1 (i = 0) is the folded 1-tap matrix of a slice shape"""
        dev = self.w0.device
        key = (i, h, w, dev, self.compute_dtype) if i == 0 else (i, dev, self.compute_dtype)
        op = self._ops.get(key)
        if op is None:
            if i == 0:
                m = folded_conv1(self.w0.cpu(), self.shift.cpu(), self.scale.cpu(), h, w).float().to(dev)
                op = Conv2dOp(m.reshape(64, UNFOLD_LD, 1, 1), self.b0, self.compute_dtype)
            else:
                op = Conv2dOp(getattr(self, f"w{i}"), getattr(self, f"b{i}"), self.compute_dtype)
            self._ops[key] = op
        return op

    def _convs(self, shape, view: int) -> List[Conv2dOp]:
        return [self._conv(0, *slice_sides(shape, view))] + [self._conv(i) for i in range(1, 5)]

    @staticmethod
    def bytes_per_slice(h: int, w: int, esize: int) -> int:
        h1, w1 = conv1_extent(h), conv1_extent(w)
        h2, w2 = pool_extent(h1), pool_extent(w1)
        h3, w3 = pool_extent(h2), pool_extent(w2)
        act = h1 * w1 * (UNFOLD_LD + 64) + h2 * w2 * (64 + 192) + h3 * w3 * (192 + 384 + 256 + 256)
        return 3 * act * esize + h1 * w1 * UNFOLD_LD * 4 + h2 * w2 * 64 + h3 * w3 * 192

    def _features(self, y, y_pred, view, cid, normalize):
        """Launches: 1 unfold per image (2), 5 GEMM forwards, 2 pools.  saved = the two pools' argmax maps."""
        B, _, D, H, W = y.shape
        S, dt = cid.numel(), self.compute_dtype
        h, w = slice_sides(y.shape, view)
        convs = self._convs(y.shape, view)
        cols = torch.empty((2 * S, conv1_extent(h), conv1_extent(w), UNFOLD_LD), dtype=dt, device=y.device)
        for half, vol in enumerate((y, y_pred)):
            _ffi.check(_ffi.lib().sa_lpips_unfold(_ffi.ptr(vol), _ffi.dtype_id(dt), ctypes.c_void_p(cols[half * S:].data_ptr()), _ffi.ptr(cid), S, view, B, D, H, W,
                                                  int(normalize), UNFOLD_LD, _ffi.stream()), "sa_lpips_unfold")
        f = [convs[0].fprop(cols)]
        del cols
        pools = []
        for i in (1, 2):
            p, idx = self._pool(f[-1], ceil=False)
            pools.append(idx)
            f.append(convs[i].fprop(p))
        f.append(convs[3].fprop(f[-1]))
        f.append(convs[4].fprop(f[-1]))
        return f, pools

    def _input_grad(self, gh, f, pools, grad, view, cid, scale):
        """Launches: 5 data-gradient GEMMs, 2 pool backwards, 1 fold.  Data gradients of the prediction's half: each launch adds the head's own gradient at
        that tap and applies the tap's ReLU mask."""
        B, _, D, H, W = grad.shape
        S = cid.numel()
        convs = self._convs(grad.shape, view)
        gz = convs[4].dgrad(gh[4], addend=gh[3], mask=f[3][S:])
        gz = convs[3].dgrad(gz, addend=gh[2], mask=f[2][S:])
        for i in (2, 1):
            gz = self._unpool(convs[i].dgrad(gz), pools[i - 1][S:], gh[i - 1], f[i - 1][S:], f[i - 1].shape, ceil=False)
        dcols = convs[0].dgrad(gz, out_dtype=torch.float32)
        _ffi.check(_ffi.lib().sa_lpips_fold(_ffi.ptr(dcols), _ffi.ptr(grad), _ffi.ptr(cid), S, view, B, D, H, W, scale, UNFOLD_LD, _ffi.stream()), "sa_lpips_fold")


def view_sums(pred: torch.Tensor, target: torch.Tensor, net: LpipsNet, views: Sequence[int], ids: List[torch.Tensor], factor: float, normalize: bool, chunk):
    """The common part of the loss-and-gradient-in-forward Functions: per view the fp64 sum of the LPIPS distances over its kept slices ``ids`` and, when
    ``pred`` requires a gradient, grad = d (factor * sum over the views of the mean distance) / d pred (else None).  Returns (grad, sums)."""
    _ffi.require_gpu()
    a = pred.contiguous()
    b = target.contiguous().to(a.device)
    grad = torch.zeros_like(a) if pred.requires_grad else None
    sums = []
    for view, vid in zip(views, ids):
        d = net.view_term(b, a, view, vid, grad, factor / vid.numel(), normalize, chunk)
        sums.append(d.double().sum())       # (one fixed-order reduction of <= a few thousand values)
    return grad, sums


class PerceptualFn(torch.autograd.Function):
    """sum over the views of ``perceptual_factor * mean(LPIPS over the kept slices)`` and its gradient to the prediction, computed in the forward
    pass; returns the differentiable sum and the per-view terms as non-differentiable side outputs (the summaries)."""

    @staticmethod
    def forward(ctx, pred, target, net: LpipsNet, views: Sequence[int], ids: List[torch.Tensor], factor: float, normalize: bool, chunk):
        ctx.grad, sums = view_sums(pred, target, net, views, ids, factor, normalize, chunk)
        terms = [s.div(vid.numel()).mul(factor).float() for s, vid in zip(sums, ids)]
        total = terms[0].clone()
        for t in terms[1:]:
            total = total + t
        ctx.mark_non_differentiable(*terms)
        return (total, *terms)

    @staticmethod
    def backward(ctx, g, *_):
        # re-entrant like _MSEFn: the stored d loss / d pred is neither consumed nor scaled in place
        grad = ctx.grad
        return (grad * g if grad is not None else None), None, None, None, None, None, None, None
