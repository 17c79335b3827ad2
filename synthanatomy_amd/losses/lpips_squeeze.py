"""The 2.5D LPIPS-squeeze perceptual term -- ``lpips.LPIPS(net="squeeze")`` of the reference's ``BaselineLoss`` (src/losses/vqvae/vqvae.py:1648-1780) and
of ``lpips_kwargs={"net": "squeeze"}`` for the three perceptual classes -- on HIP: weights, extents, the launch chain.  DESIGN.md section 7.13.

The arithmetic restates ``lpips.LPIPS(net='squeeze', version='0.1', lpips=True, spatial=False)`` in ``eval()`` mode over torchvision's SqueezeNet-1.1
``features`` from their published sources: RESTATED, UNPINNED (neither package is a dependency nor present where this project is built).  The network:
Conv(3 -> 64, k3, s2, p0) + ReLU [tap 1], three MaxPool(3, 2, ceil_mode=True), eight Fire modules (squeeze 1x1 + ReLU, expand 1x1 and expand 3x3 p1,
concatenated, + ReLU) with taps after features 4, 7, 9, 10, 11, 12; seven ``lin`` rows; the head and its zero subgradient are those of losses/lpips.py.

Runs on the ``view_term`` frame of :class:`~synthanatomy_amd.losses.lpips.LpipsNet`, as ``LpipsAlex`` does, so ``PerceptualFn`` and the loss classes take
either network; weight validation, the seeded draw and the pools are the shared ones of losses/lpips.py.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Tuple

import torch

from .. import _ffi
from .lpips import WORKSPACE_CAP, Conv2dOp, LpipsNet, _draw_state_dict, _validate_layout, ceil_pool_extent, slice_sides  # noqa: F401

# (features index, state-dict prefix, cin, squeeze, expand1x1, expand3x3) of torchvision's squeezenet1_1 inside lpips.LPIPS(net='squeeze')
FIRES = ((3, "net.slice2.3", 64, 16, 64, 64), (4, "net.slice2.4", 128, 16, 64, 64), (6, "net.slice3.6", 128, 32, 128, 128),
         (7, "net.slice3.7", 256, 32, 128, 128), (9, "net.slice4.9", 256, 48, 192, 192), (10, "net.slice5.10", 384, 48, 192, 192),
         (11, "net.slice6.11", 384, 64, 256, 256), (12, "net.slice7.12", 512, 64, 256, 256))
CONV1_KEY = "net.slice1.0"
TAP_CHANNELS = (64, 128, 256, 384, 384, 512, 512)
TAP_FIRES = (None, 1, 3, 4, 5, 6, 7)       # the Fire module (index into FIRES) whose output is tap l; tap 0 is conv1
LIN_KEYS = tuple(f"lin{i}.model.1.weight" for i in range(7))
MIN_SIDE = 17                       # the smallest slice side for which the third ceil-mode pool still has an output (17 -> 8, 4, 2, 1)


def expected_shapes() -> Dict[str, Tuple[int, ...]]:
    shapes = {CONV1_KEY + ".weight": (64, 3, 3, 3), CONV1_KEY + ".bias": (64,)}
    for _, key, ci, s, e1, e3 in FIRES:
        shapes[f"{key}.squeeze.weight"], shapes[f"{key}.squeeze.bias"] = (s, ci, 1, 1), (s,)
        shapes[f"{key}.expand1x1.weight"], shapes[f"{key}.expand1x1.bias"] = (e1, s, 1, 1), (e1,)
        shapes[f"{key}.expand3x3.weight"], shapes[f"{key}.expand3x3.bias"] = (e3, s, 3, 3), (e3,)
    for key, c in zip(LIN_KEYS, TAP_CHANNELS):
        shapes[key] = (1, c, 1, 1)
    return shapes


def random_state_dict(seed: int) -> Dict[str, torch.Tensor]:
    """Seeded stand-in weights in the key layout of ``lpips.LPIPS(net='squeeze').state_dict()``.  For tests, smoke runs and benchmarks only -- the
    distances mean nothing."""
    return _draw_state_dict(seed, expected_shapes())


def validate_state_dict(sd, source: str) -> Dict[str, torch.Tensor]:
    """The tensors this build needs from an LPIPS-squeeze state dict; an LPIPS-alex file is refused as such."""
    return _validate_layout(sd, source, expected_shapes(), "squeeze", "tools/make_lpips_weights.py --net=squeeze", ("net.slice4.8.weight", "net.slice2.3.weight"),
                            "this is an LPIPS-alex file (it holds 'net.slice2.3.weight'); --loss=baseline and lpips_kwargs net='squeeze' need the "
                            "layout of lpips.LPIPS(net='squeeze').state_dict() (tools/make_lpips_weights.py --net=squeeze)")


def is_squeeze_layout(weights) -> bool:
    return isinstance(weights, dict) and f"{FIRES[0][1]}.squeeze.weight" in weights


def conv1_extent(e: int) -> int:
    return (e - 3) // 2 + 1


def extents(e: int, what: str = "slice side") -> Tuple[int, int, int, int]:
    """(conv1, pool1, pool2, pool3) output extents of one slice side; sides below MIN_SIDE are refused by name"""
    if e < MIN_SIDE:
        raise ValueError(f"{what} {e}: every slice side must be >= {MIN_SIDE} (the smallest for which SqueezeNet's third ceil-mode pool still has an output)")
    e1 = conv1_extent(e)
    e2 = ceil_pool_extent(e1)
    e3 = ceil_pool_extent(e2)
    return e1, e2, e3, ceil_pool_extent(e3)


def folded_conv1(w: torch.Tensor, b: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """features.0 of the scaled, channel-broadcast slice as one single-channel convolution (float64): ``W'[o, t] = sum_c W[o, c, t] / scale_c`` [64, 9] and
    ``b'[o] = b[o] - sum_{c, t} W[o, c, t] shift_c / scale_c``.  Exact: the layer has no padding, so no window reads outside the image."""
    w, shift, scale = w.double(), shift.double().view(1, 3, 1, 1), scale.double().view(1, 3, 1, 1)
    return (w / scale).sum(1).reshape(w.shape[0], 9), b.double() - (w * shift / scale).sum((1, 2, 3))


def merged_expand(w1: torch.Tensor, b1: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """the two expand convolutions of a Fire module as ONE 3 x 3 / pad 1 convolution with Cout = e1 + e3: the 1 x 1 weights sit on the centre tap, the other
    taps of those rows are zero (the same sums up to added zeros); its output is ``cat[expand1x1, expand3x3]``"""
    wm = torch.zeros(w1.shape[0] + w3.shape[0], w3.shape[1], 3, 3, dtype=w3.dtype, device=w3.device)
    wm[:w1.shape[0], :, 1, 1] = w1[:, :, 0, 0]
    wm[w1.shape[0]:] = w3
    return wm, torch.cat([b1, b3])


class LpipsSqueeze(LpipsNet):
    """Frozen LPIPS-squeeze weights and the launch chain of the perceptual term over the kept slices of one view."""

    def __init__(self, weights: Dict[str, torch.Tensor], compute_dtype: torch.dtype = torch.float32, workspace_cap: int = WORKSPACE_CAP):
        super().__init__(compute_dtype, workspace_cap)
        w1, b1 = folded_conv1(weights[CONV1_KEY + ".weight"], weights[CONV1_KEY + ".bias"], weights["scaling_layer.shift"], weights["scaling_layer.scale"])
        self.register_buffer("w0", w1.t().contiguous().float(), persistent=False)        # [9][64], tap-major
        self.register_buffer("b0", b1.float(), persistent=False)
        for i, (_, key, _, _, _, _) in enumerate(FIRES):
            self.register_buffer(f"sw{i}", weights[f"{key}.squeeze.weight"].float().clone(), persistent=False)
            self.register_buffer(f"sb{i}", weights[f"{key}.squeeze.bias"].float().clone(), persistent=False)
            wm, bm = merged_expand(weights[f"{key}.expand1x1.weight"].float(), weights[f"{key}.expand1x1.bias"].float(),
                                   weights[f"{key}.expand3x3.weight"].float(), weights[f"{key}.expand3x3.bias"].float())
            self.register_buffer(f"ew{i}", wm, persistent=False)
            self.register_buffer(f"eb{i}", bm, persistent=False)
        for i, key in enumerate(LIN_KEYS):
            self.register_buffer(f"lin{i}", weights[key].float().reshape(-1).clone(), persistent=False)

    def _fire(self, i: int) -> Tuple[Conv2dOp, Conv2dOp]:
        """(squeeze, merged expand) operators of Fire module i on the buffers' device"""
        key = (i, self.w0.device, self.compute_dtype)
        ops = self._ops.get(key)
        if ops is None:
            ops = (Conv2dOp(getattr(self, f"sw{i}"), getattr(self, f"sb{i}"), self.compute_dtype),
                   Conv2dOp(getattr(self, f"ew{i}"), getattr(self, f"eb{i}"), self.compute_dtype))
            self._ops[key] = ops
        return ops

    @staticmethod
    def bytes_per_slice(h: int, w: int, esize: int) -> int:
        (h1, h2, h3, h4), (w1, w2, w3, w4) = extents(h), extents(w)
        act = h1 * w1 * 64 + h2 * w2 * (64 + 2 * (16 + 128)) + h3 * w3 * (128 + 2 * (32 + 256)) + h4 * w4 * (256 + 2 * (48 + 384) + 2 * (64 + 512))
        return 3 * act * esize + 2 * (h2 * w2 * 64 + h3 * w3 * 128 + h4 * w4 * 256)

    def _features(self, y, y_pred, view, cid, normalize):
        """Launches: 2 first layers (one per image), 3 pools, 16 GEMM forwards.  saved = (the squeeze outputs, the module outputs, the pools' argmax maps by
        the index of the module behind each pool)."""
        B, _, D, H, W = y.shape
        S, dt = cid.numel(), self.compute_dtype
        h, w = slice_sides(y.shape, view)
        fires = [self._fire(i) for i in range(len(FIRES))]
        t1 = torch.empty((2 * S, extents(h)[0], extents(w)[0], 64), dtype=dt, device=y.device)
        for half, vol in enumerate((y, y_pred)):
            _ffi.check(_ffi.lib().sa_lpips_squeeze_conv1_fwd(_ffi.ptr(vol), _ffi.dtype_id(dt), _ffi.ptr(self.w0), _ffi.ptr(self.b0),
                                                             ctypes.c_void_p(t1[half * S:].data_ptr()), _ffi.ptr(cid), S, view, B, D, H, W, int(normalize),
                                                             _ffi.stream()), "sa_lpips_squeeze_conv1_fwd")
        taps, zs, outs, idxs = [t1], [], [], {}
        x = t1
        for i, (feat, *_rest) in enumerate(FIRES):
            if feat in (3, 6, 9):                          # features 2, 5, 8: the ceil-mode pools in front of these modules
                x, idxs[i] = self._pool(x, ceil=True)
            z = fires[i][0].fprop(x)
            x = fires[i][1].fprop(z)
            zs.append(z)
            outs.append(x)
            if i in TAP_FIRES:
                taps.append(x)
        return taps, (zs, outs, idxs)

    def _input_grad(self, gh, taps, saved, grad, view, cid, scale):
        """Launches: 16 data-gradient GEMMs, 3 pool backwards, 1 first-layer adjoint.  Data gradients of the prediction's half, module by module from the
        last: g is the gradient at the PRE-activation output of module i's merged expand.  Its data gradient takes the squeeze's ReLU output as mask; the
        squeeze's data gradient then adds the head's own gradient at the tap in front of it (if that input is a tap) and takes that input as mask; where a
        pool lies in front, the pool backward takes addend and mask instead.  The first tap's ReLU mask is applied by the first layer's adjoint."""
        B, _, D, H, W = grad.shape
        S, t1, (zs, outs, idxs) = cid.numel(), taps[0], saved
        fires = [self._fire(i) for i in range(len(FIRES))]
        head_of = {fi: l for l, fi in enumerate(TAP_FIRES) if fi is not None}        # Fire index -> tap index of its output
        g = gh[6]
        for i in range(len(FIRES) - 1, -1, -1):
            g = fires[i][1].dgrad(g, mask=zs[i][S:])
            src = outs[i - 1] if i else t1                 # what feeds module i, through a pool where one lies in front: [2 S, ...]
            l_src = head_of.get(i - 1) if i else 0
            add = gh[l_src] if l_src is not None else None
            if i in idxs:
                g = self._unpool(fires[i][0].dgrad(g), idxs[i][S:], add, src[S:] if i else None, src.shape, ceil=True)
            else:
                g = fires[i][0].dgrad(g, addend=add, mask=src[S:])
        _ffi.check(_ffi.lib().sa_lpips_squeeze_conv1_bwd(_ffi.ptr(g), ctypes.c_void_p(t1[S:].data_ptr()), _ffi.dtype_id(self.compute_dtype), _ffi.ptr(self.w0),
                                                         _ffi.ptr(grad), _ffi.ptr(cid), S, view, B, D, H, W, scale, _ffi.stream()), "sa_lpips_squeeze_conv1_bwd")
