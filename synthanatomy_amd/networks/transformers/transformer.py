"""Autoregressive sampling surface of the transformers (plugin surface of reference ``src/networks/transformers/transformer.py:8-104``:
``TransformerBase.sample_next_index`` / ``sample``).

Two pieces are shared by every decoding path of this build -- the reference-faithful prefix-growing loop below and the stateful O(N) decoder of
``performer.Performer`` -- so that they cannot drift apart:

* ``choose_next``: the decision rule for ONE position (temperature, optional top-k cut, categorical draw or arg-max), with the reference's
  random-number consumption (one ``torch.multinomial`` per generated token) -- ``tests/golden/sample.npz`` pins it against the reference class;
* ``sequence_to_grid``: what happens to a finished token sequence (drop the prefix, undo the sequence ordering, reshape to the latent grid).
"""
from __future__ import annotations

import math
from typing import Any, Optional

import numpy as np
import torch


def choose_next(last_logits: torch.Tensor, temperature: float = 1.0, sample: bool = True, top_k: Optional[int] = None) -> torch.Tensor:
    """[B, V] logits of the newest position -> [B, 1] token ids."""
    scaled = last_logits / temperature
    if top_k is not None:      # everything below the k-th largest logit of a row is cut off
        kth = torch.topk(scaled, top_k, dim=-1).values[:, -1:]
        scaled = scaled.masked_fill(scaled < kth, float("-inf"))
    probs = torch.softmax(scaled, dim=-1)
    if sample:
        return torch.multinomial(probs, num_samples=1)
    return torch.topk(probs, k=1, dim=-1).indices


def sequence_to_grid(tokens: torch.Tensor, prefix_len: int, ordering) -> torch.Tensor:
    """[B, prefix + prod(dims)] generated sequence -> [B, *dims] code grid in image order (the channel axis of ``ordering.dimensions`` squeezed, so the
    result goes straight into an embedding-style lookup / ``decode_samples``)."""
    body = tokens[:, prefix_len:]
    body = body[:, ordering.get_revert_sequence_ordering()]
    return torch.squeeze(body.reshape(body.shape[0], *ordering.dimensions), 1)


def heal_log_threshold(threshold: Optional[float]) -> float:
    """the probability threshold of ``heal`` as the log-probability the decision compares with: ``None`` (score only) is -inf, which nothing lies below"""
    if threshold is None:
        return float("-inf")
    if not float(threshold) > 0.0:
        raise ValueError(f"threshold must be None or a probability > 0, but got {threshold}")
    return math.log(float(threshold))


class TransformerBase(torch.nn.Module):
    """Abstract class for transformers."""

    @torch.no_grad()
    def heal(self, codes: torch.Tensor, conditioning: torch.Tensor = None, threshold: Optional[float] = None, temperature: float = 1.0, sample: bool = True,
             top_k: Optional[int] = None):
        """Score an existing code grid ``[B, *spatial]`` token by token with p(x_t | x_<t) and resample ("heal") the tokens whose probability lies below
        ``threshold`` from the model, in sequence order, every later token conditioned on the already-healed prefix.  Returns ``(healed int64, nll float32
        in nats, replaced bool)`` in the latent grid's layout.  ``threshold=None`` scores only.  The score is the log-softmax of the RAW last-row logits
        (temperature and top-k steer the replacement draw alone, through ``choose_next``).  This is the procedure in its reference form -- one full forward
        over the growing prefix per position, as ``sample`` -- and the comparator of the O(N) decoder of ``performer.Performer``."""
        self.eval()
        log_threshold = heal_log_threshold(threshold)
        n_new = int(np.prod(self.ordering.dimensions))
        dev = next(self.parameters()).device
        body = codes.reshape(codes.shape[0], -1)[:, self.ordering.get_sequence_ordering()].long().to(dev)
        assert body.shape[1] == n_new, f"codes of {body.shape[1]} entries, but the ordering covers {n_new}"
        seq = torch.cat((torch.full_like(body[:, :1], self.bos_token()), body), 1)
        nll = torch.zeros(seq.shape, dtype=torch.float32, device=dev)
        replaced = torch.zeros(seq.shape, dtype=torch.bool, device=dev)
        for t in range(1, 1 + n_new):
            logits = self(seq[:, :t], conditioning)[:, -1, :].float()
            x = seq[:, t]
            inside = (x >= 0) & (x < logits.shape[1])
            logp = torch.log_softmax(logits, dim=-1).gather(1, x.clamp(0, logits.shape[1] - 1)[:, None]).squeeze(1)
            nll[:, t] = torch.where(inside, -logp, torch.full_like(logp, float("inf")))
            repl = (-nll[:, t] < log_threshold) | (log_threshold > 0)
            if bool(repl.any()):
                seq[:, t] = torch.where(repl, choose_next(logits, temperature, sample, top_k).squeeze(1), x)
            replaced[:, t] = repl
        return tuple(sequence_to_grid(a, 1, self.ordering) for a in (seq, nll, replaced))

    def bos_token(self) -> int:
        """the begin-of-sentence id: the entry behind the codebook in the token table (``prepare_batch`` pads the sequence with ``vocab_size``)"""
        return self.token_emb.num_embeddings - 1

    @torch.no_grad()
    def sample_next_index(self, x: torch.Tensor, conditioning: torch.Tensor = None, temperature: float = 1.0, sample: bool = True,
                          top_k: Optional[int] = None) -> torch.Tensor:
        self.eval()
        return choose_next(self(x, conditioning)[:, -1, :], temperature, sample, top_k)

    @torch.no_grad()
    def sample(self, prefix: torch.Tensor, conditioning: torch.Tensor = None, temperature: float = 1.0, sample: bool = True,
               top_k: Optional[int] = None) -> torch.Tensor:
        """The reference procedure: every new token costs one full forward over everything generated so far (O(N^2) token-forwards)."""
        n_prefix, n_new = prefix.shape[1], int(np.prod(self.ordering.dimensions))
        seq = torch.empty(prefix.shape[0], n_prefix + n_new, dtype=prefix.dtype, device=prefix.device)
        seq[:, :n_prefix] = prefix
        for t in range(n_prefix, n_prefix + n_new):
            seq[:, t:t + 1] = self.sample_next_index(seq[:, :t], conditioning=conditioning, temperature=temperature, sample=sample, top_k=top_k)
        return sequence_to_grid(seq, n_prefix, self.ordering)

    def forward(self, x: torch.Tensor) -> Any:
        return self(x)
