"""Generalized (ReLU) attention, restated: performer-pytorch 1.0.11 ``generalized_kernel`` as ``FastAttention`` calls it with
``generalized_attention=True, kernel_fn=nn.ReLU()`` (reference run_transformer.py:81, src/networks/transformers/performer.py:97-98,207-208).  The package
is absent offline and not pinned by the reference, so -- like oracle/performer_ref.py -- this is OUR restatement, parity with upstream is UNPINNED:

    data_dash = (dim_head^-1/4 * data) @ projection^T          phi(data) = relu(data_dash) + 1e-3

the same map for queries and keys: no m^-1/2 ratio, no -|x|^2 / 2 term, no maximum.  Causal linear attention over phi(q), phi(k), v is
``oracle.performer_ref.causal_linear_attention`` unchanged (eps = 1e-6 in the normaliser).

Whole-network comparisons swap ``oracle.performer_ref.softmax_kernel`` for ``as_softmax_kernel`` (pytest's monkeypatch): ``self_attention`` there calls it
for q and k, and the generalized map ignores ``is_query``."""
import torch

from oracle import performer_ref as P

KERNEL_EPS = 1e-3


def generalized_kernel(data, proj, eps=KERNEL_EPS):
    """data [..., n, d], proj [m, d] -> [..., n, m], in the dtype of ``data`` (the tests hand in fp64)"""
    c = data.shape[-1] ** -0.25
    return torch.relu(torch.einsum("...id,jd->...ij", c * data, proj.to(data.dtype))) + eps


def as_softmax_kernel(data, proj, is_query, eps=None):
    """drop-in for oracle.performer_ref.softmax_kernel"""
    return generalized_kernel(data, proj)


def attention(q, k, v, proj):
    """causal generalized attention of heads q, k, v [..., n, d]"""
    return P.causal_linear_attention(generalized_kernel(q, proj), generalized_kernel(k, proj), v)
