"""CPU: the host machinery the three backward passes share (synthanatomy_amd/runtime/backward.py) -- where weight gradients accumulate, what a report to the
sink looks like, and the cases in which a pass stays on one stream.  No device."""
import torch

from synthanatomy_amd.runtime.backward import GradCtx, side_wgrad


def _params():
    return torch.nn.Parameter(torch.randn(3, 5)), torch.nn.Parameter(torch.randn(7).double())


def test_grad_ctx_without_a_sink():
    w, b = _params()
    gc = GradCtx()
    for p in (w, b):
        t = gc.buf(p)
        assert t.shape == p.shape and t.dtype == p.dtype and not t.any()
        assert gc.buf(p) is t                  # asked twice in one pass (the residual stage's fallback route): the same accumulator
        assert gc.grads[p] is t
    assert gc.buf(None) is None
    assert len(gc.grads) == 2
    gc.done(w, None, b)                        # nothing to report to
    assert len(gc.grads) == 2 and not gc.buf(w).any()


class _Sink:
    """knows ONE parameter; records the calls of the sink protocol"""

    def __init__(self, known):
        self.known, self.t, self.calls = known, torch.full(known.shape, 2.0), []

    def buffer(self, p):
        return self.t if p is self.known else None

    def ready(self, p, *tok):
        self.calls.append(("ready", p, *tok))


class _FlushSink(_Sink):
    def flush(self):
        self.calls.append(("flush",))
        return 42


def test_grad_ctx_with_a_sink_that_flushes():
    a, b = _params()
    sink = _FlushSink(a)
    gc = GradCtx(sink)
    assert gc.buf(a) is sink.t and a not in gc.grads
    tb = gc.buf(b)                              # unknown to the sink: a private zero tensor
    assert tb is not sink.t and not tb.any() and tb.shape == b.shape and gc.grads[b] is tb and gc.buf(b) is tb
    gc.done(a, None, b)
    assert len(sink.calls) == 3 and sink.calls[0] == ("flush",)
    assert sink.calls[1][0] == "ready" and sink.calls[1][1] is a and sink.calls[1][2] == 42
    assert sink.calls[2][0] == "ready" and sink.calls[2][1] is b and sink.calls[2][2] == 42


def test_grad_ctx_with_a_sink_without_flush():
    a, b = _params()
    sink = _Sink(a)
    GradCtx(sink).done(a, None, b)
    assert [len(c) for c in sink.calls] == [2, 2]      # ready(p), no token
    assert sink.calls[0][1] is a and sink.calls[1][1] is b


def test_grad_ctx_reports_to_a_grad_reducer_with_the_token():
    from synthanatomy_amd.runtime.ddp import GradReducer
    from synthanatomy_amd.runtime.optim import FlatParams
    torch.manual_seed(0)
    w, b = torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(5))
    flat = FlatParams([w, b])
    red = GradReducer(flat)
    assert len(red.buckets) == 1
    gc = GradCtx(red)
    assert gc.buf(w).data_ptr() == flat.grad_view(w).data_ptr() and not gc.grads
    gc.done(w, b)
    assert red._pending == [0] and not red._tainted           # complete, every report behind the flush that opened it
    red.reset()
    red.ready(w)                                              # a bare report (autograd hook, third-party user of the sink)
    assert red._pending == [1] and red._tainted == {0}


def test_one_stream_off_the_device_and_in_exact_f32_mode():
    assert side_wgrad(torch.bfloat16, torch.device("cpu")) is None
    assert side_wgrad(torch.bfloat16, torch.device("cpu"), "no_side_wgrad") is None
    assert side_wgrad(torch.float32, torch.device("cpu")) is None
    assert side_wgrad(torch.float32, torch.device("cuda", 0), "no_side_wgrad", "no_side_wgrad_vqvae") is None
