"""Quantization (surface of model/modules/quantization.py:7-75): the Gumbel vector quantizer over the stem's output, on the
gfx950 kernels of csrc/pretrain.hip.  Constructor, parameters (`codevectors` (1, G*V, dg), `weight_proj`) and
`forward(hidden_states, mask_time_indices) -> (codevectors, perplexity)` are the reference's, and so is the train / eval split:
training draws Gumbel noise and counts the perplexity over the noise-free softmax, eval takes the plain argmax and counts it over
the one-hot codes.  `codevectors` is initialised uniform_() (the reference leaves it uninitialised).  `temperature` stays a plain
attribute the caller may decay."""
from typing import Optional, Tuple

import torch
import torch.nn as nn

from ... import autograd as ag
from ... import ops
from ...pretrain import gumbel_quantize


class Quantization(nn.Module):
    def __init__(self, d_model: int, n_mel_channels: int, num_codevector_groups: int, num_codevectors_per_group: int,
                 codevector_dim: int) -> None:
        super().__init__()
        self.num_groups = num_codevector_groups
        self.num_vars = num_codevectors_per_group
        if codevector_dim % self.num_groups != 0:
            raise ValueError(f"`codevector_dim {codevector_dim} must be divisible by `num_codevector_groups` {self.num_groups} "
                             "for concatenation")
        self.codevectors = nn.Parameter(torch.empty(1, self.num_groups * self.num_vars,
                                                    codevector_dim // self.num_groups).uniform_())
        self.weight_proj = nn.Linear(d_model * (((n_mel_channels - 1) // 2 - 1) // 2), self.num_groups * self.num_vars)
        self.temperature = 2            # can be decayed for training
        self.last_codes = None          # (B, T, G) int32 of the last forward: ids for the contrastive loss

    def forward(self, hidden_states: torch.Tensor, mask_time_indices: Optional[torch.Tensor] = None,
                noise: Optional[torch.Tensor] = None, weight: Optional[torch.Tensor] = None
                ) -> Tuple[torch.Tensor, torch.Tensor]:
        """hidden_states (B,T,F) fp32 on the HIP device; mask_time_indices (B,T) bool: the frames the perplexity counts (None:
        all).  noise (B*T, G, V): the Gumbel values to use in training instead of drawing them.  weight: weight_proj.weight
        re-laid for hidden_states in another feature order (Wav2Vec2 hands in the stem's channel-last output)."""
        B, T, _ = hidden_states.shape
        x = hidden_states.reshape(B * T, -1)
        w = self.weight_proj.weight if weight is None else weight
        if ag.needs_grad(self.weight_proj, x):
            logits = ag.LinearFn.apply(x, w, self.weight_proj.bias)
        else:
            logits = ops.linear(x, w, self.weight_proj.bias)
        logits = logits.float().view(B * T, self.num_groups, self.num_vars)
        rows = None if mask_time_indices is None else mask_time_indices.reshape(-1)
        out, codes, perplexity = gumbel_quantize(logits, self.codevectors, self.temperature, noise=noise, row_mask=rows,
                                                 hard_eval=not self.training)
        self.last_codes = codes.view(B, T, self.num_groups)
        return out.view(B, T, -1), perplexity
