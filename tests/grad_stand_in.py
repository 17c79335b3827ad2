"""Stand-in for ``synthanatomy_amd.runtime.backward.GradCtx`` in tests that drive ONE stage's ``bwd`` by hand: accumulators the test owns (so that it can
start them from something other than zero) and no sink."""
import torch


class Grads:
    def __init__(self, params, init=None):
        """``init``: the accumulators' starting contents, one CPU tensor per parameter (default: zeros).  ``self.init`` keeps CPU copies of them."""
        if init is None:
            init = [torch.zeros(p.shape) for p in params]
        self.init = {id(p): t.clone() for p, t in zip(params, init)}
        self.b = {id(p): t.to(p.device) for p, t in zip(params, init)}

    def buf(self, p):
        return self.b[id(p)]

    def done(self, *ps):
        pass
