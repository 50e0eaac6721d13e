"""ConformerTransducer: the Conformer encoder under a transducer (RNN-T) head, the form the architecture was published in
(INTEGRATION.md "Transducer (RNN-T)").  `encoder.*` state_dict keys are exactly Conformer's, so a CTC or pretraining checkpoint
loads into it (`load_state_dict(..., strict=False)`, Wav2Vec2.export_encoder_state_dict into `.encoder`).

    forward(x (B,n_mel,T), lengths (B), targets (B,U) padded, target_lengths (B)) -> (logits (B,T',U+1,V), out_len (B))
    greedy(x, lengths, max_symbols=10) -> (tokens (B, T' * max_symbols), counts (B), frames (B, T' * max_symbols))

The logits go to ConformerCriterion.rnnt_loss with out_len and target_lengths."""
from typing import Optional, Tuple

import torch
import torch.nn as nn

from .modules.encoder import Encoder
from .modules.transducer import Joiner, Predictor


class ConformerTransducer(nn.Module):
    def __init__(self, vocab_size: int, n_mel_channels: int = 80, n_conformer_blocks: int = 16, d_model: int = 256,
                 n_heads: int = 4, kernel_size: int = 31, pred_hidden_dim: int = 640, n_pred_layers: int = 1,
                 joint_dim: int = 640, blank_id: int = 0, dropout_rate: float = 0.0) -> None:
        super().__init__()
        self.blank_id = int(blank_id)
        self.encoder = Encoder(n_mel_channels=n_mel_channels, n_blocks=n_conformer_blocks, d_model=d_model,
                               n_heads=n_heads, kernel_size=kernel_size, dropout_rate=dropout_rate)
        self.predictor = Predictor(vocab_size=vocab_size, hidden_dim=pred_hidden_dim, n_layers=n_pred_layers,
                                   blank_id=blank_id)
        self.joiner = Joiner(d_model=d_model, hidden_dim=pred_hidden_dim, joint_dim=joint_dim, vocab_size=vocab_size)

    def _encode(self, x: torch.Tensor, lengths: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        h, out_len = self.encoder(x, lengths)
        if out_len is None:
            out_len = torch.full((h.shape[0],), h.shape[1], dtype=torch.int64, device=h.device)
        return h, out_len

    def forward(self, x: torch.Tensor, lengths: Optional[torch.Tensor], targets: Optional[torch.Tensor],
                target_lengths: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        h, out_len = self._encode(x, lengths)
        pred = self.predictor(targets, target_lengths)
        return self.joiner(h, pred), out_len

    @torch.no_grad()
    def greedy(self, x: torch.Tensor, lengths: Optional[torch.Tensor] = None, max_symbols: int = 10):
        from ..decode import rnnt_greedy_decode
        h, out_len = self._encode(x, lengths)
        return rnnt_greedy_decode(self.predictor, self.joiner, h, out_len, max_symbols)
