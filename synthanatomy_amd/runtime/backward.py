"""Host machinery the hand-scheduled backward passes of the VQ-VAE, the Performer and the discriminator share: where weight gradients accumulate and when
a bucket is reported to the reducer (``GradCtx``), weight-gradient launches on a second HIP stream with their operand-lifetime window (``SideWgrad``,
DESIGN §5a) and the one decision whether a pass uses that stream (``side_wgrad``)."""
from __future__ import annotations

import collections
import os

import torch

from .. import debug


class SideWgrad:
    """Weight gradients on a second HIP stream.  They are leaves of the backward pass: nothing on the main chain reads a dW before the optimizer, and the dense
    data-gradient launches they sit between run one block per CU (§4.4 (iii)) -- the weight-gradient blocks of the other queue share those CUs.  Every launch is
    ordered behind an event of the main stream (its operands are complete) and the main stream joins once at the end of the backward pass.

    Operand lifetime (round 6): the operands of the last ``LAG`` side launches are kept alive HERE, and before the launch that pushes one out of that window
    the main stream waits for its completion event -- so an operand returns to the main stream's allocator pool only behind a stream-ordered wait, and the next
    main-stream kernel that is handed the same block cannot overtake the side launch still reading it.  Rounds 3-5 used ``Tensor.record_stream`` instead: the
    caching allocator then parks every freed operand until an event recorded AT FREE TIME on the side stream has completed, and with the host a whole iteration
    ahead of the device no block ever became reusable -- the pool of the adversarial iteration grew to 113 GB for 29 GB of live tensors, with GB-sized
    ``hipMalloc``s inside the first dozen iterations (the 1 431 ms "adversarial" record of round 5: one warm-up + three timed iterations, all of them allocating)."""

    try:
        LAG = max(1, int(os.environ.get("SA_SIDE_WGRAD_LAG", "3")))
    except ValueError:
        raise ValueError(f"SA_SIDE_WGRAD_LAG={os.environ.get('SA_SIDE_WGRAD_LAG')!r}: expected the number of side-stream launches whose operands stay alive (an integer >= 1)") from None
    _streams = {}        # the weight-gradient stream of each device, shared by every pass

    def __init__(self, dev):
        self.main = torch.cuda.current_stream(dev)
        key = dev.index if dev.index is not None else torch.cuda.current_device()
        if key not in self._streams:
            self._streams[key] = torch.cuda.Stream(device=dev)
        self.side = self._streams[key]
        self.inflight = collections.deque()

    def run(self, fn, *operands):
        ev = torch.cuda.Event()
        ev.record(self.main)
        self.side.wait_event(ev)
        with torch.cuda.stream(self.side):
            fn()                                  # (workspaces allocated in here come from the side stream's own pool: stream-ordered reuse)
            done = torch.cuda.Event()
            done.record(self.side)
        self.inflight.append((done, operands))
        while len(self.inflight) > self.LAG:
            old, ops = self.inflight.popleft()
            self.main.wait_event(old)
            del ops

    def join(self):
        self.main.wait_stream(self.side)
        self.inflight.clear()


def side_wgrad(dtype, device, *host_switches):
    """The ``SideWgrad`` of one backward pass, or None for one stream: exact-f32 mode, any of the named ``debug.host`` switches, ``--deterministic``, tensors
    off the device, or a current stream that is being captured into a graph (the window's cross-stream waits are not part of a capture)."""
    if dtype == torch.float32 or device.type != "cuda" or any(debug.host(s) for s in host_switches):
        return None
    if debug.deterministic() or torch.cuda.is_current_stream_capturing():
        return None
    return SideWgrad(device)


class GradCtx:
    """Where the weight-gradient kernels accumulate.  Without a sink: fresh zeroed tensors handed back to autograd.  With a
    sink (runtime.ddp.GradReducer): views of the flat gradient buffer, and the sink is told as soon as a parameter's
    gradient kernels are queued so that its bucket's all-reduce can start while backward continues."""

    def __init__(self, sink=None, side=None):
        self.sink, self.grads, self.side = sink, {}, side

    def wgrad(self, op, x, g, dw, db):
        """op.wgrad(x, g, dw, db); on the second stream when there is one (SideWgrad: weight gradients are leaves of the pass)"""
        if self.side is None:
            op.wgrad(x, g, dw, db)
        else:
            self.side.run(lambda: op.wgrad(x, g, dw, db), x, g, dw, db)

    def buf(self, p):
        """the accumulator of parameter p (None for None): the same tensor however often a pass asks"""
        if p is None:
            return None
        if self.sink is not None:
            b = self.sink.buffer(p)
            if b is not None:
                return b
        t = self.grads.get(p)
        if t is None:
            t = torch.zeros_like(p)
            self.grads[p] = t
        return t

    def done(self, *params):
        if self.sink is None:
            return
        if self.side is not None and getattr(self.sink, "active", True):
            # DDP: a bucket's all-reduce is ordered behind an event of the CURRENT stream (runtime/ddp.GradReducer._launch); the gradients of these parameters
            # were queued on the main stream (bias / gate gradients) and on the weight-gradient stream, so report them from the latter after it has caught up
            self.side.side.wait_stream(self.side.main)
            with torch.cuda.stream(self.side.side):
                self._report(params)
            return
        self._report(params)

    def _report(self, params):
        params = [p for p in params if p is not None]
        if hasattr(self.sink, "flush"):
            tok = self.sink.flush()       # optimizer slices deferred by EARLIER reports: everything that reads their parameters is queued (runtime/ddp.GradReducer.flush)
            for p in params:
                self.sink.ready(p, tok)
        else:
            for p in params:
                self.sink.ready(p)
