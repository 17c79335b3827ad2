"""GPU: the parts of synthanatomy_amd/runtime/backward.py that need streams -- the operand-lifetime window of the weight-gradient stream and the
stream a bucket is reported from -- and the discriminator's ``invalidate_packed_weights``.  Everything here waits on events and compares values."""
import weakref

import pytest
import torch

pytestmark = pytest.mark.gpu

NUMEL = 65536


def _launch(side, out, a, b):
    """one side-stream launch reading a and b; nothing but ``side`` holds them once this returns"""
    side.run(lambda: out.copy_(a + b), a, b)


def test_side_stream_keeps_the_operands_of_the_last_lag_launches_alive():
    from synthanatomy_amd.runtime.backward import SideWgrad
    dev = torch.device("cuda", torch.cuda.current_device())
    side = SideWgrad(dev)
    LAG, n = side.LAG, 5
    assert LAG == 3 and side.side != side.main
    gen = torch.Generator(device=dev).manual_seed(7)
    outs = [torch.zeros(NUMEL, device=dev) for _ in range(n)]
    want, refs = [], []
    for i in range(n):
        a, b = torch.randn(NUMEL, device=dev, generator=gen), torch.randn(NUMEL, device=dev, generator=gen)
        want.append(a + b)                     # on the main stream, beforehand
        refs.append((weakref.ref(a), weakref.ref(b)))
        _launch(side, outs[i], a, b)
        del a, b
        assert len(side.inflight) <= LAG
        for j, (ra, rb) in enumerate(refs):
            alive = j > i - LAG                # the last LAG launches; the main stream has been made to wait for every earlier one
            assert (ra() is not None) == alive and (rb() is not None) == alive, (i, j)
    side.join()
    assert not side.inflight and all(ra() is None and rb() is None for ra, rb in refs)
    torch.cuda.synchronize()
    for i in range(n):
        assert torch.equal(outs[i], want[i]), i


class _Sink:
    """records the stream every report arrives on"""

    def __init__(self):
        self.streams = []

    def buffer(self, p):
        return None

    def ready(self, p):
        self.streams.append(torch.cuda.current_stream())


def test_a_bucket_is_reported_from_the_weight_gradient_stream_when_the_sink_is_active():
    from synthanatomy_amd.runtime.backward import GradCtx, SideWgrad
    dev = torch.device("cuda", torch.cuda.current_device())
    main = torch.cuda.current_stream(dev)
    side = SideWgrad(dev)
    p, q = torch.nn.Parameter(torch.zeros(4, device=dev)), torch.nn.Parameter(torch.zeros(2, device=dev))

    def streams(sink, side_):
        GradCtx(sink, side_).done(p, None, q)
        assert len(sink.streams) == 2 and torch.cuda.current_stream(dev) == main
        return sink.streams

    active, idle, plain = _Sink(), _Sink(), _Sink()
    active.active, idle.active = True, False
    assert streams(active, side) == [side.side, side.side]
    assert streams(idle, side) == [main, main]
    assert streams(plain, side) == [side.side, side.side]        # a sink that does not say counts as active
    for sink in (_Sink(), active):
        sink.streams = []
        assert streams(sink, None) == [main, main]               # one-stream pass
    side.join()
    torch.cuda.synchronize()


def test_discriminator_invalidate_packed_weights():
    from synthanatomy_amd.networks.discriminator.baseline import BaselineDiscriminator
    torch.manual_seed(3)
    disc = BaselineDiscriminator(input_nc=1, ndf=8, n_layers=1).cuda().eval()
    x = torch.randn(1, 1, 8, 8, 8, device="cuda")
    with torch.no_grad():
        y0 = disc(x).clone()
        for p in disc.parameters():
            p.data.mul_(1.25)                  # behind autograd's version counter, as the fused Adam kernel writes
        before = [s.op._pack_version() for s in disc._stages]
        disc.invalidate_packed_weights()
        assert all(s.op._pack_version() != v for s, v in zip(disc._stages, before))
        y1 = disc(x)
        fresh = BaselineDiscriminator(input_nc=1, ndf=8, n_layers=1).cuda().eval()
        fresh.load_state_dict(disc.state_dict())
        y2 = fresh(x)
    torch.cuda.synchronize()
    assert torch.equal(y1, y2) and not torch.equal(y0, y1)
