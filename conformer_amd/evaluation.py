"""Surface of the reference's evaluation.py: ConformerCriterion (CTC loss, evaluation.py:8-16) on the gfx950 lattice
kernels, ConformerMetric (WER / CER, evaluation.py:18-27) as a plain host-side edit distance (the reference delegates to
torchmetrics' WordErrorRate / CharErrorRate: total edit distance / total reference length over the batch).  wer_tokens /
cer_tokens take token ids on the device instead of strings and score them there (conformer_amd.error_rate)."""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import torch

from . import autograd as ag


class ConformerCriterion:
    def __init__(self, blank_id: int = 0) -> None:
        self.blank_id = int(blank_id)

    def ctc_loss(self, outputs: torch.Tensor, targets: torch.Tensor, input_lengths: torch.Tensor,
                 target_lengths: torch.Tensor) -> torch.Tensor:
        """outputs: logits (B,T',V) as Conformer.forward returns them (any float dtype; computed in fp32 as
        evaluation.py:13); targets (B,Lmax) padded or 1-D concatenated (float targets are accepted as the reference
        passes them, evaluation.py:14); lengths (B,).  Mean over utterances of nll / target_length, infinite terms zeroed."""
        if not outputs.is_cuda:
            raise RuntimeError("ConformerCriterion.ctc_loss: logits must be on the HIP device (no CPU fallback)")
        return ag.CtcLossFn.apply(outputs.float(), targets.long(), input_lengths, target_lengths, self.blank_id)

    def mwer_loss(self, outputs: torch.Tensor, targets: torch.Tensor, input_lengths: torch.Tensor,
                  target_lengths: torch.Tensor, tables, *, unit: str = "word", n_best: int = 4, beam_width: int = 100,
                  hyp_tokens: Optional[torch.Tensor] = None, hyp_counts: Optional[torch.Tensor] = None,
                  num_hyps: Optional[torch.Tensor] = None, add_reference: bool = False, ctc_weight: float = 0.0,
                  decoder=None) -> torch.Tensor:
        """Minimum-word-error-rate loss over the n-best list (INTEGRATION.md "MWER training and n-best scores"): the mean over
        the batch of sum_n P_n W_n - mean_n W_n, where W_n is the edit distance of hypothesis n to the reference in `unit`s
        ("word", "char" or "token", error_rate.error_counts with `tables`, an ErrorRateTables) and P_n the softmax, over the
        list, of the exact CTC log-likelihoods of the hypotheses given `outputs` (autograd.CtcNbestScoreFn).  The subtracted
        mean centres the number and has no gradient.  An utterance with fewer than two live hypotheses contributes 0.

        outputs: logits (B,T',V) on the HIP device (no CPU fallback); targets (B,Lr) padded int64; lengths (B).  The list is
        hyp_tokens (B,N,L), hyp_counts (B,N) and optionally num_hyps (B), as the beam search returns them; when none is handed
        in, the device beam search runs on outputs.detach() with n_best and beam_width -- or `decoder` (a BeamCTCDecoder) runs
        its own, with its beam, language model and hotwords.  add_reference appends the reference as one more row unless a
        hypothesis already equals it (token distance 0).  ctc_weight adds ctc_weight * ctc_loss(...), the usual interpolation.
        One host read: the longest hypothesis (and, with add_reference, reference) sets the lattice width."""
        from . import decode, error_rate
        if not isinstance(outputs, torch.Tensor) or not outputs.is_cuda:
            raise RuntimeError("ConformerCriterion.mwer_loss: logits must be on the HIP device (no CPU fallback)")
        if targets.dim() != 2:
            raise ValueError(f"ConformerCriterion.mwer_loss: targets must be (B,Lr) padded, got {tuple(targets.shape)}")
        x = outputs.float()
        B, dev = x.shape[0], x.device
        refs = targets.long().to(dev).contiguous()
        in_len = torch.as_tensor(input_lengths).to(dev).long().contiguous()
        ref_len = torch.as_tensor(target_lengths).to(dev).long().contiguous()
        if hyp_tokens is None:
            if hyp_counts is not None or num_hyps is not None:
                raise ValueError("ConformerCriterion.mwer_loss: hyp_counts / num_hyps without hyp_tokens")
            if decoder is None:
                hyp_tokens, hyp_counts, _, num_hyps = decode.beam_ctc_decode(x.detach(), self.blank_id, in_len, beam_width,
                                                                             n_best)
            else:
                out = decode._beam_search(x.detach(), decoder.blank_id, in_len, n_best, decoder.beam_width,
                                          decoder.token_min_logp, decoder.beam_prune_logp, decoder.max_candidates, decoder.vocab,
                                          decoder._call_fusion(B, None, None))
                hyp_tokens, hyp_counts, num_hyps = out[0], out[1], out[-1]
        elif hyp_counts is None:
            raise ValueError("ConformerCriterion.mwer_loss: hyp_tokens without hyp_counts")
        hyp_tokens, hyp_counts = hyp_tokens.to(dev), hyp_counts.to(dev)
        hyp_len, _ = decode.nbest_rows(hyp_tokens, hyp_counts, num_hyps, 0, "ConformerCriterion.mwer_loss")
        if add_reference:
            N, width = hyp_tokens.shape[1], max(hyp_tokens.shape[2], refs.shape[1])
            rows = torch.full((B, N + 1, width), -1, dtype=torch.int64, device=dev)
            rows[:, :N, :hyp_tokens.shape[2]] = hyp_tokens
            rows[:, N, :refs.shape[1]] = refs
            same, _, _ = error_rate.error_counts(hyp_tokens.contiguous(), hyp_len.clamp_min(0), refs, ref_len, tables, "token")
            found = ((same == 0) & (hyp_len >= 0)).any(dim=1)
            last = ref_len.clamp(0, refs.shape[1]).masked_fill(found, -1)
            hyp_tokens, hyp_len = rows, torch.cat([hyp_len, last[:, None]], dim=1)
        max_len = int(hyp_len.max())                                   # the one host read
        errors, _, _ = error_rate.error_counts(hyp_tokens.contiguous(), hyp_len.clamp_min(0), refs, ref_len, tables, unit)
        ll = ag.CtcNbestScoreFn.apply(x, hyp_tokens, hyp_len, in_len, self.blank_id, max_len)
        loss = ag.MwerRiskFn.apply(ll, errors, hyp_len)
        if ctc_weight:
            loss = loss + float(ctc_weight) * self.ctc_loss(outputs, targets, input_lengths, target_lengths)
        return loss

    def rnnt_loss(self, outputs: torch.Tensor, targets: Optional[torch.Tensor], input_lengths: torch.Tensor,
                  target_lengths: torch.Tensor, reduction: str = "mean") -> torch.Tensor:
        """The transducer loss (INTEGRATION.md "Transducer (RNN-T)"): outputs are the joint's logits (B,T',U1,V) as
        ConformerTransducer.forward returns them (any float dtype; computed in fp32) on the HIP device (no CPU fallback); targets
        (B,U1-1) padded (None when U1 == 1); lengths (B).  blank_id is the blank.  "none": nll (B) float64, +inf for an utterance
        without a frame; "sum": the sum of the finite nll; "mean": that sum divided by B."""
        if not isinstance(outputs, torch.Tensor) or not outputs.is_cuda:
            raise RuntimeError("ConformerCriterion.rnnt_loss: logits must be on the HIP device (no CPU fallback)")
        if reduction not in ("mean", "sum", "none"):
            raise ValueError(f"ConformerCriterion.rnnt_loss: reduction must be 'mean', 'sum' or 'none', got {reduction!r}")
        tg = None if targets is None else targets.long().to(outputs.device)
        nll = ag.RnntLossFn.apply(outputs.float(), tg, input_lengths, target_lengths, self.blank_id)
        if reduction == "none":
            return nll
        total = nll.masked_fill(~torch.isfinite(nll), 0.0).sum()
        return total / nll.shape[0] if reduction == "mean" else total

    def pretrain_loss(self, context: torch.Tensor, target: torch.Tensor, perplexity: torch.Tensor, mask_indexes: torch.Tensor,
                      codes: Optional[torch.Tensor] = None, num_negatives: int = 100, temperature: float = 0.1,
                      diversity_weight: float = 0.1, generator: Optional[torch.Generator] = None, *,
                      num_codevectors: int = 640, negatives: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The wav2vec 2.0 objective on what Wav2Vec2.forward returns (INTEGRATION.md "Self-supervised pretraining"):

            contrastive + diversity_weight * (G V - perplexity) / (G V) * n_masked

        contrastive: pretrain.contrastive_loss of context against target (both (B,T',P)) over the frames of mask_indexes (B,T')
        with num_negatives draws per frame from the other masked frames of the same utterance (pretrain.sample_negatives with
        `generator`, or `negatives` (B,T',K) handed in).  codes (B,T',G), the quantizer's (Quantization.last_codes): a negative
        with the positive's codes is excluded.  num_codevectors is G V (640: the reference's 2 x 320).  Everything stays on the
        device; the parts are left in self.last_pretrain: contrastive, perplexity, n_masked and accuracy = n_correct / n_masked."""
        from . import pretrain
        if not isinstance(context, torch.Tensor) or not context.is_cuda:
            raise RuntimeError("ConformerCriterion.pretrain_loss: context must be on the HIP device (no CPU fallback)")
        mask = mask_indexes.to(context.device)
        if negatives is None:
            negatives = pretrain.sample_negatives(mask, int(num_negatives), generator)
        ids = None
        if codes is not None:
            c = codes.to(torch.int64)
            if c.shape[-1] <= 6:              # fold the G codes (each below 2^10) into one id: no collision, no host read
                ids = (c << (10 * torch.arange(c.shape[-1], device=c.device))).sum(dim=-1)
            else:                             # a dense id per distinct row (torch.unique synchronises)
                ids = torch.unique(c.reshape(-1, c.shape[-1]), dim=0, return_inverse=True)[1].view(c.shape[:-1])
        loss, _, n_correct = pretrain.contrastive_loss(context.float(), target.float(), mask, negatives, ids, temperature)
        n_masked = mask.sum()
        gv = float(num_codevectors)
        total = loss + float(diversity_weight) * (gv - perplexity) / gv * n_masked
        self.last_pretrain = {"contrastive": loss.detach(), "perplexity": perplexity.detach(), "n_masked": n_masked,
                              "accuracy": n_correct / n_masked.clamp_min(1)}
        return total


def _edit_distance(ref: Sequence, hyp: Sequence) -> int:
    prev = list(range(len(hyp) + 1))
    for i, r in enumerate(ref, 1):
        cur = [i] + [0] * len(hyp)
        for j, h in enumerate(hyp, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (r != h))
        prev = cur
    return prev[-1]


def _error_rate(prediction: Union[str, List[str]], target: Union[str, List[str]], split) -> torch.Tensor:
    preds = [prediction] if isinstance(prediction, str) else list(prediction)
    refs = [target] if isinstance(target, str) else list(target)
    errors = total = 0
    for p, r in zip(preds, refs):
        rt = split(r)
        errors += _edit_distance(rt, split(p))
        total += len(rt)
    return torch.tensor(errors / total if total else float("nan"))


class ConformerMetric:
    def wer_score(self, prediction: Union[str, List[str]], target: Union[str, List[str]]) -> torch.Tensor:
        return _error_rate(prediction, target, str.split)

    def cer_score(self, prediction: Union[str, List[str]], target: Union[str, List[str]]) -> torch.Tensor:
        return _error_rate(prediction, target, list)

    def wer_tokens(self, hyp_tokens: torch.Tensor, hyp_counts: torch.Tensor, ref_tokens: torch.Tensor,
                   ref_counts: torch.Tensor, tables) -> torch.Tensor:
        """wer_score of the texts these token rows spell, computed on the device from the ids (error_rate.error_counts takes the
        same arguments; `tables` is an error_rate.ErrorRateTables).  A 0-dim float64 device tensor; nothing synchronises."""
        from .error_rate import rate_tokens
        return rate_tokens(hyp_tokens, hyp_counts, ref_tokens, ref_counts, tables, "word")

    def cer_tokens(self, hyp_tokens: torch.Tensor, hyp_counts: torch.Tensor, ref_tokens: torch.Tensor,
                   ref_counts: torch.Tensor, tables) -> torch.Tensor:
        """cer_score of the texts these token rows spell, computed on the device from the ids, as wer_tokens."""
        from .error_rate import rate_tokens
        return rate_tokens(hyp_tokens, hyp_counts, ref_tokens, ref_counts, tables, "char")
