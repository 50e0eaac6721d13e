"""Self-supervised pretraining of the encoder, wav2vec 2.0 style (INTEGRATION.md "Self-supervised pretraining"): span masking,
negative sampling, the Gumbel vector quantizer and the contrastive loss.  The two samplers are device torch ops without a host
read-back; the quantizer and the loss are the gfx950 kernels of csrc/pretrain.hip (autograd.GumbelQuantizeFn,
autograd.ContrastiveLossFn) and have no CPU fallback."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from . import autograd as ag


def span_mask(lengths: torch.Tensor, T: int, p: float = 0.065, span: int = 10,
              generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """(B,T) bool, True = masked.  Every valid frame t <= lengths[b] - span starts a span of `span` frames with probability p,
    and the frame with the smallest draw of each row always starts one: an utterance of at least `span` frames has at least
    `span` masked frames (a shorter one has none).  Frames at or beyond lengths[b] are never masked.  One torch.rand block on the
    device of `lengths`; nothing is read back."""
    if not isinstance(T, int) or T < 1 or not isinstance(span, int) or span < 1 or not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"span_mask: T and span must be positive ints and p in [0, 1], got T={T!r}, span={span!r}, p={p!r}")
    lengths = torch.as_tensor(lengths)
    dev = lengths.device
    r = torch.rand((lengths.shape[0], T), generator=generator, device=dev)
    t = torch.arange(T, device=dev)
    n = lengths.to(torch.int64).clamp(0, T)[:, None]
    can_start = t[None, :] <= n - span
    r = r.masked_fill(~can_start, 2.0)
    forced = (t[None, :] == r.argmin(dim=1)[:, None]) & can_start
    starts = ((r < float(p)) | forced).to(torch.int32).cumsum(dim=1)
    before = torch.nn.functional.pad(starts, (span, 0))[:, :T]           # the count of starts up to t - span
    return ((starts - before) > 0) & (t[None, :] < n)


def sample_negatives(mask: torch.Tensor, K: int = 100, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """(B,T,K) int32: for every masked frame K draws, uniform with replacement, over the OTHER masked frames of its utterance:
    a rank in [0, m_b - 1) skips the frame's own rank and maps through the sorted table of the masked positions.  -1 at
    unmasked frames and in utterances with fewer than two masked frames.  Nothing is read back."""
    if mask.dim() != 2 or mask.dtype != torch.bool or not isinstance(K, int) or K < 1:
        raise ValueError(f"sample_negatives: mask must be (B,T) bool and K a positive int, got {tuple(mask.shape)} {mask.dtype}, "
                         f"K={K!r}")
    B, T = mask.shape
    m = mask.sum(dim=1)                                                   # (B)
    own = mask.to(torch.int64).cumsum(dim=1) - 1                          # the rank of a masked frame among the masked
    table = torch.sort((~mask).to(torch.uint8), dim=1, stable=True).indices   # the masked positions first, ascending
    u = torch.rand((B, T, K), generator=generator, device=mask.device)
    span = (m - 1).clamp_min(1)[:, None, None]
    rank = (u * span).long().clamp_max_(span - 1)
    rank = rank + (rank >= own[:, :, None]).long()
    neg = table.gather(1, rank.clamp_(0, T - 1).view(B, T * K)).view(B, T, K)
    keep = mask[:, :, None] & (m >= 2)[:, None, None]
    return torch.where(keep, neg, torch.full_like(neg, -1)).to(torch.int32)


def _on_device(t, name: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.ConformerHipError(f"{name}: expected a tensor on a HIP device, got {getattr(t, 'device', type(t))}; the "
                                     "pretraining objective only exists as gfx950 kernels (no CPU fallback)")


def gumbel_quantize(logits: torch.Tensor, codevectors: torch.Tensor, tau: float, noise: Optional[torch.Tensor] = None,
                    row_mask: Optional[torch.Tensor] = None, hard_eval: bool = False
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(out (N,G*dg), codes (N,G) int32, perplexity ()): logits (N,G,V) fp32, codevectors (G*V,dg) (a leading 1 is dropped).
    codes = argmax(logits + noise), out the chosen rows of codevectors side by side, perplexity = sum_g exp(entropy of the mean
    over the rows of row_mask (N) of softmax(logits))).  Differentiable in logits (straight through softmax((logits + noise) /
    tau), plus the perplexity) and in codevectors.  noise=None draws Gumbel values as F.gumbel_softmax does; a given noise is
    used as is.  hard_eval: plain argmax, the marginal of the one-hot codes, nothing differentiable."""
    _on_device(logits, "logits")
    _on_device(codevectors, "codevectors")
    if codevectors.dim() == 3 and codevectors.shape[0] == 1:
        codevectors = codevectors[0]
    if hard_eval:
        noise = None
        logits, codevectors = logits.detach(), codevectors.detach()
    elif noise is None:
        noise = -torch.empty_like(logits, memory_format=torch.legacy_contiguous_format).exponential_().log()
    return ag.GumbelQuantizeFn.apply(logits, codevectors, float(tau), noise, row_mask)


def contrastive_loss(context: torch.Tensor, targets: torch.Tensor, mask: torch.Tensor, negatives: torch.Tensor,
                     ids: Optional[torch.Tensor] = None, temperature: float = 0.1
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(loss (), frame_loss (B,T), n_correct () int32): context, targets (B,T,D) fp32, mask (B,T) bool, negatives (B,T,K) int32
    as sample_negatives returns them (an index outside [0,T) is an absent candidate), ids (B,T) int64 or None (a negative whose
    id equals the positive's is excluded: pass the quantizer's codes folded into one id per frame).  frame_loss is
    -log softmax(cos(context, candidates) / temperature)[positive] at masked frames and 0 elsewhere; loss its sum.
    Differentiable in context and targets."""
    _on_device(context, "context")
    _on_device(targets, "targets")
    return ag.ContrastiveLossFn.apply(context, targets, mask, negatives, ids, float(temperature))
