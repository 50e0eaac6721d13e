"""The transducer's two heads (INTEGRATION.md "Transducer (RNN-T)"): the label predictor and the joint network.

Predictor: an embedding of [blank, y_0 .. y_{U-1}] (blank stands for start-of-sequence), then `n_layers` LSTM layers over the
lengths target_lengths + 1 from zero state.  Joiner: logits = out(tanh(enc_proj(enc)[:, :, None] + pred_proj(pred)[:, None])).
The embedding lookup is an index gather (F.embedding); everything that does arithmetic runs on the gfx950 kernels: the LSTM
(autograd.LstmFn in training, ops.lstm_forward with a carried state in `step`), the fp32 GEMMs (autograd.LinearFn /
ops.linear) and the combine (autograd.RnntJointFn / ops.rnnt_joint_forward).  There is no CPU path.

The reference carries a model/modules/transducer.py too, a stub around nn.Transformer that nothing uses; it is not reproduced.
"""
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import autograd as ag
from ... import ops


def _linear(layer: nn.Linear, x: torch.Tensor) -> torch.Tensor:
    if ag.needs_grad(layer, x):
        return ag.LinearFn.apply(x, layer.weight, layer.bias)
    return ops.linear(x, layer.weight.detach(), layer.bias.detach())


class Predictor(nn.Module):
    def __init__(self, vocab_size: int, hidden_dim: int, n_layers: int = 1, blank_id: int = 0) -> None:
        super().__init__()
        if hidden_dim % 4 != 0:
            raise NotImplementedError(f"Predictor: the LSTM kernels take a hidden size that is a multiple of 4, got {hidden_dim}")
        if not 0 <= blank_id < vocab_size:
            raise ValueError(f"Predictor: blank_id {blank_id} outside the vocabulary of {vocab_size}")
        self.vocab_size, self.blank_id = int(vocab_size), int(blank_id)
        self.embedding = nn.Embedding(vocab_size, hidden_dim)
        self.lstm = nn.LSTM(input_size=hidden_dim, hidden_size=hidden_dim, num_layers=n_layers, batch_first=True)

    def _layer(self, k: int):
        return tuple(getattr(self.lstm, f"{name}_l{k}") for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))

    def forward(self, targets: Optional[torch.Tensor], target_lengths: torch.Tensor) -> torch.Tensor:
        """targets (B,U) int64 padded (None or U = 0: only the start position), target_lengths (B) -> (B,U+1,H); rows at or
        behind target_lengths + 1 are zero."""
        dev = self.embedding.weight.device
        lens = torch.as_tensor(target_lengths).to(device=dev, dtype=torch.int64)
        B = lens.shape[0]
        start = torch.full((B, 1), self.blank_id, dtype=torch.int64, device=dev)
        if targets is None:
            tokens = start
        else:
            tokens = torch.cat([start, targets.to(device=dev, dtype=torch.int64).clamp(0, self.vocab_size - 1)], dim=1)
        lens = lens.clamp(0, tokens.shape[1] - 1) + 1
        h = F.embedding(tokens, self.embedding.weight)
        for k in range(self.lstm.num_layers):
            w_ih, w_hh, b_ih, b_hh = self._layer(k)
            if ag.needs_grad(self, h):
                h = ag.LstmFn.apply(h, w_ih, w_hh, b_ih, b_hh, lens)
            else:
                h = ops.lstm_forward(h.detach(), w_ih.detach(), w_hh.detach(), (b_ih + b_hh).detach(), lens)
        return h

    def init_state(self, batch: int) -> torch.Tensor:
        """Zero state, planes (2 * n_layers, B, H): plane 2k is layer k's hidden state, plane 2k + 1 its cell state."""
        return torch.zeros(2 * self.lstm.num_layers, batch, self.lstm.hidden_size, dtype=torch.float32,
                           device=self.embedding.weight.device)

    @torch.no_grad()
    def fused_biases(self):
        """b_ih + b_hh per layer, as the LSTM kernels take them: computed once for a loop of `step` calls"""
        return [(self._layer(k)[2] + self._layer(k)[3]).contiguous() for k in range(self.lstm.num_layers)]

    @torch.no_grad()
    def step(self, last: torch.Tensor, state: torch.Tensor, biases=None) -> torch.Tensor:
        """Consume one token per utterance: last (B) int64, state as init_state lays it out, advanced IN PLACE.  Returns the top
        layer's output (B,H) (the top hidden plane after the step).  biases: what fused_biases returned."""
        biases = self.fused_biases() if biases is None else biases
        x = F.embedding(last.clamp(0, self.vocab_size - 1), self.embedding.weight)[:, None, :]
        for k in range(self.lstm.num_layers):
            w_ih, w_hh, _, _ = self._layer(k)
            x = ops.lstm_forward(x, w_ih, w_hh, biases[k], None, state=(state[2 * k], state[2 * k + 1]))
        return x[:, 0, :]


class Joiner(nn.Module):
    def __init__(self, d_model: int, hidden_dim: int, joint_dim: int, vocab_size: int) -> None:
        super().__init__()
        self.enc_proj = nn.Linear(d_model, joint_dim)
        self.pred_proj = nn.Linear(hidden_dim, joint_dim)
        self.out = nn.Linear(joint_dim, vocab_size)

    def project(self, enc: torch.Tensor, pred: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return _linear(self.enc_proj, enc), _linear(self.pred_proj, pred)

    def combine(self, e: torch.Tensor, p: torch.Tensor, frames: Optional[torch.Tensor] = None) -> torch.Tensor:
        """logits (B,T,U1,V) from the projections e (B,T,J) and p (B,U1,J); with frames (B) int64 (no gradient), (B,1,U1,V) from
        the one frame e[b, frames[b]] of every utterance."""
        if frames is None and ag.needs_grad(self, e, p):
            h = ag.RnntJointFn.apply(e, p)
        else:
            h = ops.rnnt_joint_forward(e.detach(), p.detach(), frames)
        return _linear(self.out, h)

    def forward(self, enc: torch.Tensor, pred: torch.Tensor) -> torch.Tensor:
        """enc (B,T,d_model), pred (B,U1,hidden_dim) -> logits (B,T,U1,V)"""
        e, p = self.project(enc.float(), pred.float())
        return self.combine(e, p)
