"""Wav2Vec2 (surface of model/wav2vec2.py:15-54): a wav2vec 2.0-style pretrainer over the Conformer's own stem and blocks -- a
masked context network, a Gumbel quantizer over the stem's output and two projections.  The reference's file cannot be imported
(it needs torchaudio, a generate_mask that does not exist and a wrong heads= keyword); its constructor and state_dict keys are
kept, its forward is written out as it was meant (INTEGRATION.md "Self-supervised pretraining"):

    stem -> targets = quantization_projector(quantization(stem output, mask))       from the UNMASKED stem output
         -> masked frames of the stem output zeroed -> input Linear -> blocks -> hidden_projector = context

`forward(x (B,n_mel,T), lengths (B) int64) -> (context (B,T',P), target (B,T',P), perplexity (), mask_indexes (B,T') bool)`.
mask_indexes is True at MASKED frames (the reference's `!= 0` marks the unmasked ones and counts the perplexity over them: a bug
not copied).  Masking is pretrain.span_mask: `time_augment` is the span, `time_mask_ratio` the start probability."""
from typing import Optional, Tuple

import torch
import torch.nn as nn

from .. import autograd as ag
from .. import ops
from ..pretrain import span_mask
from .modules.quantization import Quantization
from .utils._guard import STRICT, refuse_dropout
from .utils.block import ConformerBlock
from .utils.convolution import ConvolutionSubsampling
from .utils.position import RelativePositionalEncoding


class Wav2Vec2(nn.Module):
    def __init__(self, n_blocks: int, n_mel_channels: int, d_model: int, heads: int, kernel_size: int, proj_dim: int,
                 num_groups: int = 2, num_vars: int = 320, time_augment: int = 30, time_mask_ratio: float = 0.065,
                 dropout_rate: float = 0.0) -> None:
        super().__init__()
        self.n_freq_out = ((n_mel_channels - 1) // 2 - 1) // 2
        self.downsampling_conv = ConvolutionSubsampling(channels=d_model)
        self.linear = nn.Linear(in_features=d_model * self.n_freq_out, out_features=d_model)
        self.rel_pe = RelativePositionalEncoding(d_model=d_model)
        self.blocks = nn.ModuleList([ConformerBlock(d_model=d_model, n_heads=heads, kernel_size=kernel_size,
                                                    dropout_rate=dropout_rate) for _ in range(n_blocks)])
        self.span = int(time_augment)
        self.mask_prob = float(time_mask_ratio)
        self.quantization = Quantization(d_model=d_model, n_mel_channels=n_mel_channels, num_codevector_groups=num_groups,
                                         num_codevectors_per_group=num_vars, codevector_dim=proj_dim)
        self.hidden_projector = nn.Linear(in_features=d_model, out_features=proj_dim)
        self.quantization_projector = nn.Linear(in_features=proj_dim, out_features=proj_dim)

    @staticmethod
    def _linear(layer: nn.Linear, x: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        w = layer.weight if weight is None else weight
        if ag.needs_grad(layer, x):
            return ag.LinearFn.apply(x, w, layer.bias)
        return ops.linear(x, w, layer.bias)

    def forward(self, x: torch.Tensor, lengths: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
                mask_indexes: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """generator seeds the span mask; mask_indexes (B,T') bool and noise (B*T', G, V) fix the mask and the quantizer's Gumbel
        values instead of drawing them (a fixed batch for a test or a probe)."""
        refuse_dropout(self, "Wav2Vec2")
        d = self.linear.out_features
        h = self.downsampling_conv.channel_last(x)                                   # (B, T', F'*C)
        if h.dtype != torch.float32:
            h = h.float()
        B, n_frames, _ = h.shape
        out_len = ConvolutionSubsampling.out_lengths(lengths)
        if out_len is None:
            out_len = torch.full((B,), n_frames, dtype=torch.int64, device=h.device)
        elif out_len.device != h.device:
            out_len = out_len.to(h.device)
        if STRICT and int(out_len.max()) != n_frames:
            raise RuntimeError(f"lengths.max() after subsampling must equal T'={n_frames}")
        if mask_indexes is None:
            mask_indexes = span_mask(out_len, n_frames, self.mask_prob, self.span, generator)
        # the quantizer reads the stem output in the reference's feature order (c*F' + f): its weight re-laid, not the activation
        wq = self.quantization.weight_proj.weight
        wq = wq.view(wq.shape[0], d, self.n_freq_out).transpose(1, 2).reshape(wq.shape[0], -1)
        target, perplexity = self.quantization(h, mask_indexes, noise=noise, weight=wq)
        target = self._linear(self.quantization_projector, target)
        h = h * (~mask_indexes)[:, :, None].to(h.dtype)                              # the reference's masking value: zero
        wlp = self.linear.weight.view(d, d, self.n_freq_out).transpose(1, 2).reshape(d, -1)
        h = self._linear(self.linear, h, wlp)
        table = self.rel_pe.table(n_frames)
        for layer in self.blocks:
            h, _ = layer.fused_chain(h, table, out_len, None)
        return self._linear(self.hidden_projector, h), target, perplexity, mask_indexes

    def export_encoder_state_dict(self) -> dict:
        """The stem, input Linear, positional encoding and blocks under the Encoder's keys (`blocks.*` -> `layers.*`):
        `conformer.encoder.load_state_dict(w2v.export_encoder_state_dict(), strict=False)` picks up the pretrained weights."""
        out = {}
        for k, v in self.state_dict().items():
            head = k.split(".", 1)[0]
            if head in ("downsampling_conv", "linear", "rel_pe"):
                out[k] = v
            elif head == "blocks":
                out["layers." + k.split(".", 1)[1]] = v
        return out
