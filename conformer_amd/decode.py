"""CTC decoding on the device.

Greedy (reference: ConformerProcessor.greedy_decode / batch_greedy_decode, processing/processor.py:301-334):
one kernel does the per-frame argmax ("CTC alignment indices") and the pad/unk filtering + repeat collapse, replacing the
reference's per-frame `.item()` host loop (train.py:61).

Prefix beam search (reference: KenLanguageModel, processing/lm.py:6-75, without the language model): `beam_ctc_decode` and
`BeamCTCDecoder`, semantics in INTEGRATION.md "CTC prefix beam search".  Unlike the greedy decoder it collapses by the
standard CTC rule: a blank separates repeats.

The same search fused with a word n-gram model (`conformer_amd.lm`, an ARPA file): `beam_ctc_lm_decode` and
`BeamCTCDecoder(lm=...)`, semantics in INTEGRATION.md "Language-model fusion".

Hotword boosting, with or without the language model (`conformer_amd.hotwords`): `beam_ctc_hotword_decode` and
`BeamCTCDecoder(hotwords=...)`, semantics in INTEGRATION.md "Hotword boosting".  A list and a weight per utterance
(`hotwords=[...]` per call, `BeamCTCStream.set_hotwords`): INTEGRATION.md "Per-request hotwords".

The same search resumed chunk by chunk over a stream, in every mode: `beam_ctc_stream_init/step/finish` and
`BeamCTCDecoder.stream`, semantics in INTEGRATION.md "Streaming (resumable) search".  With `max_pending` the stream has no end:
after every step the prefix no live hypothesis can change is committed and the prefix tree re-rooted there, INTEGRATION.md
"Committed-prefix streaming (max_pending)".

Token and word timestamps from the search itself, in every mode above (`return_times=`, `times=True`, `BeamCTCDecoder.words`,
`BeamCTCStream.pop_committed_words`): INTEGRATION.md "Beam-search timestamps"."""
from __future__ import annotations

import math
from typing import Callable, Iterable, List, Optional, Sequence, Tuple, Union

import torch

from . import _lib, ops
from ._slot_state import positive_seconds
from .align import Word, group_words
from . import hotwords as _hw
from .hotwords import HotwordRows, Hotwords, as_hotwords
from .lm import NgramLanguageModel, as_language_model


def greedy_ctc_decode(logits: torch.Tensor, pad_id: int, unk_id: int, lengths: Optional[torch.Tensor] = None
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """logits (B,T,V) fp32 on the HIP device -> (frame_ids (B,T) int64, tokens (B,T) int64 padded with -1, counts (B)).
    `lengths=None` decodes every frame, as the reference does."""
    x = ops._req(logits, "logits")
    B, T, V = x.shape
    frame_ids = torch.empty(B, T, dtype=torch.int64, device=x.device)
    tokens = torch.empty(B, T, dtype=torch.int64, device=x.device)
    counts = torch.empty(B, dtype=torch.int64, device=x.device)
    if lengths is not None:
        lengths = ops._req(lengths, "lengths", torch.int64)
    _lib.call("cfm_greedy_ctc_decode_f32", x.data_ptr(), ops._p(lengths), frame_ids.data_ptr(), tokens.data_ptr(),
              counts.data_ptr(), B, T, V, int(pad_id), int(unk_id), ops._stream())
    return frame_ids, tokens, counts


def tokens_to_text(tokens: torch.Tensor, counts: torch.Tensor, vocab: Sequence[str], delim_token: str = "|") -> List[str]:
    """Host-side join of the decoded ids (processor.py:319): ''.join(vocab[id]).replace(delim, ' ')."""
    tk, ct = tokens.cpu().tolist(), counts.cpu().tolist()
    return ["".join(vocab[i] for i in row[:n]).replace(delim_token, " ") for row, n in zip(tk, ct)]


RNNT_SYNC_EVERY = 64      # iterations between two host reads of the device's `active` counter: the fastest of 4 / 16 / 64 in
                          # profiles/rnnt_bench.json


@torch.no_grad()
def rnnt_greedy_decode(predictor, joiner, enc: torch.Tensor, enc_len: Optional[torch.Tensor] = None, max_symbols: int = 10,
                       sync_every: int = RNNT_SYNC_EVERY) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Time-synchronous greedy transducer decode (INTEGRATION.md "Transducer (RNN-T)") of the encoder output enc (B,T,d) with
    lengths enc_len (B) through a Predictor and a Joiner (model/modules/transducer.py).  Returns (tokens (B, T * max_symbols)
    int64 padded with -1, counts (B) int64, frames (B, T * max_symbols) int64: the frame each token was emitted at).

    At most max_symbols tokens are emitted per frame.  The loop runs on the device: per iteration one decision per utterance
    (joint at the utterance's frame, argmax, emit or advance) and one predictor step whose state is kept where a token was
    emitted.  The host reads the device's count of unfinished utterances once per sync_every iterations and stops
    unconditionally after T * (max_symbols + 1), the most any utterance can need."""
    if int(max_symbols) < 1 or int(sync_every) < 1:
        raise ValueError(f"rnnt_greedy_decode: max_symbols and sync_every must be at least 1, got {max_symbols}, {sync_every}")
    enc = ops._req(enc if enc.dtype == torch.float32 else enc.float(), "enc")
    B, T, _ = enc.shape
    dev = enc.device
    if enc_len is None:
        in_len = torch.full((B,), T, dtype=torch.int64, device=dev)
    else:
        in_len = ops._req(torch.as_tensor(enc_len).to(dev), "enc_len", torch.int64)
    blank, cap = predictor.blank_id, T * int(max_symbols)
    tokens = torch.full((B, cap), -1, dtype=torch.int64, device=dev)
    frames = torch.full((B, cap), -1, dtype=torch.int64, device=dev)
    count = torch.zeros((B,), dtype=torch.int64, device=dev)
    t = torch.zeros((B,), dtype=torch.int64, device=dev)
    nsym = torch.zeros((B,), dtype=torch.int64, device=dev)
    last = torch.full((B,), blank, dtype=torch.int64, device=dev)
    emit = torch.zeros((B,), dtype=torch.int32, device=dev)
    active = torch.zeros((1,), dtype=torch.int32, device=dev)
    e = ops.linear(enc, joiner.enc_proj.weight.detach(), joiner.enc_proj.bias.detach())       # once, before the loop
    w_p, b_p = joiner.pred_proj.weight.detach(), joiner.pred_proj.bias.detach()
    biases = predictor.fused_biases()
    state = predictor.init_state(B)
    predictor.step(last, state, biases)                                     # the state after consuming blank
    cand = torch.empty(tuple(state.shape), dtype=torch.float32, device=dev)
    top = state[state.shape[0] - 2]                                         # the top layer's hidden plane (B,H), a view
    for it in range(T * (int(max_symbols) + 1)):
        p = ops.linear(top[:, None, :], w_p, b_p)                           # (B,1,J)
        logits = joiner.combine(e, p, frames=t)                             # (B,1,1,V) at each utterance's own frame
        ops.rnnt_greedy_decide(logits.view(B, -1), in_len, T, blank, max_symbols, tokens, frames, count, last, t, nsym, emit)
        cand.copy_(state)
        predictor.step(last, cand, biases)                                  # the candidate: one step on `last`
        ops.rnnt_greedy_commit(cand, state, emit, t, in_len, T, active)     # kept where a token was emitted
        if (it + 1) % int(sync_every) == 0 and int(active) == 0:
            break
    return tokens, count, frames


class _Fusion:
    """The fusion group of a search: the device tables of the language model and of the hotwords (None: not used) and the
    knobs.  `args` is the group as the C entries take it (lm_tables, alpha, beta, unk_score_offset, score_boundary, hw_tables,
    hotword_weight); `fused`: the search has LM or hotword terms (and returns am_scores).
    `rows`: per-request hotwords, (buffer, pointers (B) int64, weights (B) float64) on the device (HotwordRows.to_device, or a
    stream's reserved regions).  The search is then the hotword search through the entries of conformer_hip3_hotword_rows.h,
    which take the same group with the two arrays in the place of (hw_tables, hotword_weight); `hw_tables` is the buffer, which
    the init, reset and commit entries read as the mode flag only."""

    def __init__(self, lm_tables: Optional[torch.Tensor], hw_tables: Optional[torch.Tensor], alpha: float, beta: float,
                 unk_score_offset: float, score_boundary: bool, hotword_weight: float = 0.0, rows=None) -> None:
        self.rows = rows
        if rows is not None:
            hw_tables = rows[0]
        self.lm_tables, self.hw_tables = lm_tables, hw_tables
        self.score_boundary = 1 if score_boundary else 0
        self.fused = lm_tables is not None or hw_tables is not None
        self.args = (ops._p(lm_tables), float(alpha), float(beta), float(unk_score_offset), self.score_boundary,
                     ops._p(hw_tables), float(hotword_weight))
        if rows is not None:
            self.args = self.args[:5] + (rows[1].data_ptr(), rows[2].data_ptr())


_PLAIN = _Fusion(None, None, 0.0, 0.0, 0.0, False)
_NO_TIMES = (None, 0, None, None)          # the absent times group of the per-row stream entries


def _logits(logits: torch.Tensor) -> torch.Tensor:
    """fp32 logits on the device (bf16 / fp16 cast to fp32)"""
    if isinstance(logits, torch.Tensor) and logits.dtype in (torch.bfloat16, torch.float16):
        logits = logits.float()
    return ops._req(logits, "logits")


def _beam_outputs(B: int, N: int, T: int, device, fused: bool):
    tokens = torch.empty(B, N, T, dtype=torch.int64, device=device)
    counts = torch.empty(B, N, dtype=torch.int64, device=device)
    scores = torch.empty(B, N, dtype=torch.float32, device=device)
    am_scores = torch.empty(B, N, dtype=torch.float32, device=device) if fused else None
    num_hyps = torch.empty(B, dtype=torch.int64, device=device)
    return tokens, counts, scores, am_scores, num_hyps


def _flag(who: str, name: str, value) -> bool:
    """A boolean option, checked on the host (a tensor or a count passed by position lands here)."""
    if not isinstance(value, bool):
        raise ValueError(f"{who}: {name} must be True or False, got {value!r}")
    return value


def _is_rows(hotwords) -> bool:
    """`hotwords` is one entry per utterance (not one list of phrases): a list or tuple with an element that is no str."""
    return isinstance(hotwords, (list, tuple)) and any(not isinstance(e, str) for e in hotwords)


def _per_row(hotwords, hotword_weight) -> bool:
    return _is_rows(hotwords) or isinstance(hotword_weight, (list, tuple))


def token_words(decoder: "BeamCTCDecoder", ids: Sequence[int], frames: Sequence[int], logps: Sequence[float],
                frame_seconds: float) -> List[Word]:
    """Words of one hypothesis from the search's own timestamps (INTEGRATION.md "Beam-search timestamps"): token i spans
    [frames[i], frames[i] + 1), a Word's score is the mean of its tokens' log-probabilities."""
    v = decoder.vocab
    delim = v.index(decoder.delim_token) if decoder.delim_token in v else None
    return group_words(ids, frames, [f + 1 for f in frames], logps, v, delim, frame_seconds, decoder.skip_ids)


def _beam_search(logits: torch.Tensor, blank_id: int, lengths: Optional[torch.Tensor], n_best: int, beam_width: int,
                 token_min_logp: float, beam_prune_logp: float, max_candidates: int, vocab: Optional[Sequence[str]] = None,
                 fusion: Optional[Callable[[torch.device], _Fusion]] = None, return_times: bool = False):
    """The one-shot search behind beam_ctc_decode / beam_ctc_lm_decode / beam_ctc_hotword_decode and BeamCTCDecoder.
    `fusion(device)` builds the fusion group on the logits' device (None: the plain search); `vocab` must then have V tokens.
    Returns (tokens, counts, scores, num_hyps), with am_scores before num_hyps when fused.  return_times: the same search as
    init / step / finish on a temporary stream state (bit for bit the one-shot result), with the trailing pair (token_frames
    (B,N,T) int64 padded with -1, token_logp (B,N,T) fp32 padded with -inf)."""
    _flag("beam search", "return_times", return_times)
    x = _logits(logits)
    if x.dim() != 3:
        raise ValueError(f"logits: expected (B,T,V), got {tuple(x.shape)}")
    B, T, V = x.shape
    if fusion is not None and len(vocab) != V:
        raise ValueError(f"vocab has {len(vocab)} tokens, the logits {V}")
    if lengths is not None:
        lengths = ops._req(lengths, "lengths", torch.int64)
    f = _PLAIN if fusion is None else fusion(x.device)
    if return_times:
        st = _stream_alloc("beam search", B, T, x.device, int(beam_width), int(max_candidates), f, None, 0, True)
        beam_ctc_stream_step(st, x, blank_id, lengths, n_best=n_best, token_min_logp=token_min_logp,
                             beam_prune_logp=beam_prune_logp)
        tokens, counts, scores, am_scores, num_hyps, times = beam_ctc_stream_finish(st, n_best)
        if f.fused:
            return tokens, counts, scores, am_scores, num_hyps, times
        return tokens, counts, scores, num_hyps, times
    ws_bytes =_lib.load().cfm_ctc_beam_workspace_bytes(B, T, int(beam_width), int(max_candidates))
    workspace = torch.empty(max(int(ws_bytes), 1), dtype=torch.uint8, device=x.device)
    tokens, counts, scores, am_scores, num_hyps = _beam_outputs(B, int(n_best), T, x.device, f.fused)
    search = (x.data_ptr(), ops._p(lengths), B, T, V, int(blank_id), int(beam_width), int(max_candidates),
              float(token_min_logp), float(beam_prune_logp), int(n_best))
    out = (workspace.data_ptr(), int(ws_bytes), tokens.data_ptr(), counts.data_ptr(), scores.data_ptr())
    if f.rows is not None:
        if f.rows[1].numel() != B:
            raise ValueError(f"hotwords: {f.rows[1].numel()} per-utterance tables, the logits have {B} utterances")
        name, args = "cfm3_ctc_beam_hw_rows_decode_f32", search + f.args + out + (am_scores.data_ptr(),)
    elif f.hw_tables is not None:
        name, args = "cfm_ctc_beam_hw_decode_f32", search + f.args + out + (am_scores.data_ptr(),)
    elif f.lm_tables is not None:      # the LM entry takes the group without the hotword pair
        name, args = "cfm_ctc_beam_lm_decode_f32", search + f.args[:5] + out + (am_scores.data_ptr(),)
    else:
        name, args = "cfm_ctc_beam_decode_f32", search + out
    _lib.call(name, *args, num_hyps.data_ptr(), ops._stream())
    if f.fused:
        return tokens, counts, scores, am_scores, num_hyps
    return tokens, counts, scores, num_hyps


def beam_ctc_decode(logits: torch.Tensor, blank_id: int, lengths: Optional[torch.Tensor] = None, beam_width: int = 100,
                    n_best: int = 1, token_min_logp: float = -5.0, beam_prune_logp: float = -10.0, max_candidates: int = 16,
                    return_times: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """CTC prefix beam search over logits (B,T,V) on the HIP device (fp32, or bf16 / fp16 cast to fp32).
    Returns (tokens (B,N,T) int64 padded with -1, counts (B,N) int64, scores (B,N) fp32, num_hyps (B) int64), N = n_best,
    hypotheses best first; unused rows hold count 0, tokens -1 and score -inf.  `lengths` (B) int64 on the device: frames
    to consume per utterance (clamped to [0,T]; None = all).  Nothing synchronises with the host.
    return_times: the result gains a trailing pair (token_frames (B,N,T) int64 padded with -1, token_logp (B,N,T) fp32 padded
    with -inf), INTEGRATION.md "Beam-search timestamps"."""
    return _beam_search(logits, blank_id, lengths, n_best, beam_width, token_min_logp, beam_prune_logp, max_candidates,
                        return_times=return_times)


def beam_ctc_lm_decode(logits: torch.Tensor, blank_id: int, lm: Union[NgramLanguageModel, str],
                       lengths: Optional[torch.Tensor] = None, *, vocab: Sequence[str], delim_token: str = "|",
                       skip_ids: Sequence[int] = (), alpha: float = 2.1, beta: float = 9.2, unk_score_offset: float = -10.0,
                       score_boundary: bool = True, beam_width: int = 100, n_best: int = 1, token_min_logp: float = -5.0,
                       beam_prune_logp: float = -10.0, max_candidates: int = 16, return_times: bool = False
                       ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """CTC prefix beam search fused with the word n-gram model `lm` (an NgramLanguageModel or an ARPA path), on the HIP
    device.  `vocab` (V strings) spells the tokens: a token equal to `delim_token` (or " ") ends a word, tokens in
    `skip_ids` have no characters.  Hypotheses rank by the fused score (INTEGRATION.md "Language-model fusion").
    Returns (tokens (B,N,T) int64 padded with -1, counts (B,N) int64, scores (B,N) fp32 fused, am_scores (B,N) fp32
    acoustic, num_hyps (B) int64), best first by the final fused score; unused rows hold count 0, tokens -1 and scores
    -inf.  The device tables are packed and copied once per (lm, vocab, delim_token, skip_ids); after that nothing
    synchronises with the host.  return_times: as beam_ctc_decode, a trailing (token_frames, token_logp)."""
    def fusion(device):
        return _Fusion(as_language_model(lm).device_tables(vocab, delim_token, skip_ids, device), None, alpha, beta,
                       unk_score_offset, score_boundary)
    return _beam_search(logits, blank_id, lengths, n_best, beam_width, token_min_logp, beam_prune_logp, max_candidates,
                        vocab, fusion, return_times)


def beam_ctc_hotword_decode(logits: torch.Tensor, blank_id: int, hotwords: Union[Hotwords, Iterable[str]],
                            lengths: Optional[torch.Tensor] = None, *, vocab: Sequence[str], delim_token: str = "|",
                            skip_ids: Sequence[int] = (), hotword_weight: float = 9.0,
                            lm: Union[NgramLanguageModel, str, None] = None, alpha: float = 2.1, beta: float = 9.2,
                            unk_score_offset: float = -10.0, score_boundary: bool = True, beam_width: int = 100,
                            n_best: int = 1, token_min_logp: float = -5.0, beam_prune_logp: float = -10.0,
                            max_candidates: int = 16, return_times: bool = False
                            ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """CTC prefix beam search with hotword boosting on the HIP device, fused with the word n-gram model `lm` when one is
    given (an NgramLanguageModel or an ARPA path; alpha, beta, unk_score_offset, score_boundary as in beam_ctc_lm_decode).
    `hotwords`: a Hotwords or a sequence of phrases (str); `hotword_weight` any finite float.  Words are formed from `vocab`
    as in beam_ctc_lm_decode.  Hypotheses rank by the boosted score (INTEGRATION.md "Hotword boosting").  Returns (tokens
    (B,N,T) int64 padded with -1, counts (B,N) int64, scores (B,N) fp32 final boosted score, am_scores (B,N) fp32 acoustic,
    num_hyps (B) int64), best first by the final score; unused rows hold count 0, tokens -1 and scores -inf.  The device
    tables are packed and copied once per (hotwords, vocab, delim_token, skip_ids); after that nothing synchronises with the
    host.  return_times: as beam_ctc_decode, a trailing (token_frames, token_logp).
    Per-request hotwords (INTEGRATION.md "Per-request hotwords"): `hotwords` may be a list or tuple of B entries, one per
    utterance -- None, () or []: no hotwords for that utterance; a Hotwords; or a sequence of phrases -- and `hotword_weight` a
    list or tuple of B floats.  Row b of every output then equals this call on utterance b alone with its list and weight."""
    if _per_row(hotwords, hotword_weight):
        # per-request hotwords: `hotwords` is one entry per utterance (None or (): no hotwords, a Hotwords, or phrases) and / or
        # `hotword_weight` one float per utterance; row b is the single-list call on utterance b alone
        B = logits.shape[0] if isinstance(logits, torch.Tensor) and logits.dim() == 3 else 0
        entries = hotwords if _is_rows(hotwords) else [hotwords] * B
        rows = HotwordRows(entries, hotword_weight, vocab, delim_token, skip_ids, batch=B)

        def fusion_rows(device):
            lm_tables = None if lm is None else as_language_model(lm).device_tables(vocab, delim_token, skip_ids, device)
            return _Fusion(lm_tables, None, alpha, beta, unk_score_offset, score_boundary, rows=rows.to_device(device))
        return _beam_search(logits, blank_id, lengths, n_best, beam_width, token_min_logp, beam_prune_logp, max_candidates,
                            vocab, fusion_rows, return_times)
    if not math.isfinite(float(hotword_weight)):
        raise ValueError(f"hotword_weight must be finite, got {hotword_weight}")

    def fusion(device):
        hw = hotwords if isinstance(hotwords, Hotwords) else Hotwords(hotwords)
        hw_tables = hw.device_tables(vocab, delim_token, skip_ids, device)
        lm_tables = None if lm is None else as_language_model(lm).device_tables(vocab, delim_token, skip_ids, device)
        return _Fusion(lm_tables, hw_tables, alpha, beta, unk_score_offset, score_boundary, hotword_weight)
    return _beam_search(logits, blank_id, lengths, n_best, beam_width, token_min_logp, beam_prune_logp, max_candidates,
                        vocab, fusion, return_times)


class BeamCTCDecoder:
    """Drop-in for the reference's KenLanguageModel (processing/lm.py:6-75) without the language model: the same
    `__call__(logits, lengths=None, decode_func=None)`, a str for (T,V) logits and a list of str for (B,T,V).
    The best hypothesis is joined as ''.join(vocab[id]) with `delim_token` read as a space (processor.py:319); ids in
    `skip_ids` (the unk id, for example) are dropped from the text, not from the search.
    With `lm` (an NgramLanguageModel or the path of an ARPA file) the search is fused with that word n-gram model, as
    KenLanguageModel(lm_path, ..., alpha, beta) does: beam_ctc_lm_decode.  Without it the decoder is acoustic only.
    With `hotwords` (phrases, or a Hotwords) the search boosts them by `hotword_weight`, with or without `lm`, as
    KenLanguageModel(..., hotwords, hotword_weight) does: beam_ctc_hotword_decode.  None or an empty list leaves the
    decoder as it is without them."""

    def __init__(self, vocab: Sequence[str], blank_id: int, skip_ids: Sequence[int] = (), delim_token: str = "|",
                 beam_width: int = 190, beam_prune_logp: float = -20.0, token_min_logp: float = -5.0,
                 max_candidates: int = 16, *, lm: Union[NgramLanguageModel, str, None] = None, alpha: float = 2.1,
                 beta: float = 9.2, unk_score_offset: float = -10.0, score_boundary: bool = True,
                 hotwords: Union[Hotwords, Iterable[str], None] = None, hotword_weight: float = 9.0) -> None:
        self.vocab = list(vocab)
        self.blank_id = int(blank_id)
        self.skip_ids = frozenset(int(i) for i in skip_ids)
        self.delim_token = delim_token
        self.beam_width = beam_width
        self.beam_prune_logp = beam_prune_logp
        self.token_min_logp = token_min_logp
        self.max_candidates = max_candidates
        self.lm = None if lm is None else as_language_model(lm)
        self.alpha = alpha
        self.beta = beta
        self.unk_score_offset = unk_score_offset
        self.score_boundary = score_boundary
        self.hotwords = as_hotwords(hotwords)
        if self.hotwords is not None and not math.isfinite(float(hotword_weight)):
            raise ValueError(f"hotword_weight must be finite, got {hotword_weight}")
        self.hotword_weight = hotword_weight

    def stream(self, batch: int, max_frames: Optional[int], device=None, *, max_pending: Optional[int] = None,
               max_chunk_frames: Optional[int] = None, commit_log: int = 4096, times: bool = False,
               frame_seconds: float = 0.04, hotword_rows: Optional[Tuple[int, int]] = None) -> "BeamCTCStream":
        """A resumable search configured like this decoder (beam knobs, lm, hotwords) over `batch` utterances of at most
        `max_frames` frames in all: BeamCTCStream.  max_pending (tokens) with max_chunk_frames (logit frames per step) and
        max_frames=None: a stream without an end in commit mode (beam_ctc_stream_init).  times: the search records token
        timestamps and the stream hands out Words (pop_committed_words, partial_words, finish_words), frame_seconds per frame.
        hotword_rows=(max_phrases, max_code_points): every utterance may take its own hotword list within those bounds
        (BeamCTCStream.set_hotwords); None: the stream exactly as before."""
        return BeamCTCStream(self, batch, max_frames, device, max_pending=max_pending, max_chunk_frames=max_chunk_frames,
                             commit_log=commit_log, times=times, frame_seconds=frame_seconds, hotword_rows=hotword_rows)

    def words(self, logits: torch.Tensor, lengths: Optional[torch.Tensor] = None, frame_seconds: float = 0.04, *,
              hotwords=None, hotword_weight=None) -> List[List[Word]]:
        """The best hypothesis of every utterance of logits (B,T,V) as align.Words timed by the search itself (INTEGRATION.md
        "Beam-search timestamps": a token's frame is its entry into the surviving lineage, not the Viterbi start CTCAligner
        returns; Word.score is the mean token log-probability).  Synchronises.  hotwords, hotword_weight: as __call__."""
        fs = positive_seconds("BeamCTCDecoder.words", "frame_seconds", frame_seconds)
        if lengths is not None and not (isinstance(lengths, torch.Tensor) and lengths.is_cuda):
            lengths = torch.as_tensor(lengths, dtype=torch.int64).reshape(-1).to(logits.device)
        fusion = self._call_fusion(logits.shape[0], hotwords, hotword_weight)
        out = _beam_search(logits, self.blank_id, lengths, 1, self.beam_width, self.token_min_logp, self.beam_prune_logp,
                           self.max_candidates, self.vocab, fusion, True)
        tk, ct = out[0][:, 0].cpu().tolist(), out[1][:, 0].cpu().tolist()
        fr, lp = out[-1][0][:, 0].cpu().tolist(), out[-1][1][:, 0].cpu().tolist()
        return [token_words(self, tk[b][:n], fr[b][:n], lp[b][:n], fs) for b, n in enumerate(ct)]

    def text(self, ids: Sequence[int]) -> str:
        joined = "".join(self.vocab[i] for i in ids if i not in self.skip_ids)
        return " ".join(joined.replace(self.delim_token, " ").split())

    def _fusion(self, device) -> _Fusion:
        """The decoder's fusion group on `device`: its LM and hotword tables (packed and copied once per device) and knobs."""
        if self.lm is None and self.hotwords is None:
            return _PLAIN
        skip = tuple(sorted(self.skip_ids))
        lm_tables = None if self.lm is None else self.lm.device_tables(self.vocab, self.delim_token, skip, device)
        hw_tables = None if self.hotwords is None else self.hotwords.device_tables(self.vocab, self.delim_token, skip, device)
        return _Fusion(lm_tables, hw_tables, self.alpha, self.beta, self.unk_score_offset, self.score_boundary,
                       self.hotword_weight)

    def _texts(self, tokens: torch.Tensor, counts: torch.Tensor, decode_func: Optional[Callable[[str], str]] = None
               ) -> List[str]:
        preds = []
        for row, n in zip(tokens[:, 0].cpu().tolist(), counts[:, 0].cpu().tolist()):
            text = self.text(row[:n])
            preds.append(decode_func(text) if decode_func is not None else text)
        return preds

    def _call_fusion(self, B: int, hotwords, hotword_weight):
        """The `fusion` argument of _beam_search for one call: the decoder's own group, or, with per-request hotwords, the
        group with a table and a weight per utterance (packed and uploaded for this call; no cache of the decoder grows)."""
        if hotwords is None and hotword_weight is None:
            return None if self.lm is None and self.hotwords is None else self._fusion
        rows = HotwordRows([None] * B if hotwords is None else hotwords, hotword_weight, self.vocab, self.delim_token,
                           self.skip_ids, batch=B, default=self.hotwords, default_weight=self.hotword_weight)

        def fusion(device):
            skip = tuple(sorted(self.skip_ids))
            lm_tables = None if self.lm is None else self.lm.device_tables(self.vocab, self.delim_token, skip, device)
            return _Fusion(lm_tables, None, self.alpha, self.beta, self.unk_score_offset, self.score_boundary,
                           rows=rows.to_device(device))
        return fusion

    def __call__(self, logits: torch.Tensor, lengths: Optional[torch.Tensor] = None,
                 decode_func: Optional[Callable[[str], str]] = None, *, hotwords=None, hotword_weight=None
                 ) -> Union[str, List[str]]:
        """hotwords: one entry per utterance (B of them; for (T,V) logits a list of one) -- None: the decoder's own list, () or
        []: no hotwords, a Hotwords, or a sequence of phrases, which REPLACES the decoder's list for that utterance;
        hotword_weight: one float or B of them (None: the decoder's).  Utterance b's text is what a decoder constructed with
        its list and weight returns for it alone (INTEGRATION.md "Per-request hotwords").  Neither given: the call as before."""
        single = logits.dim() == 2
        if single:
            logits = logits.unsqueeze(0)
        if lengths is not None and not (isinstance(lengths, torch.Tensor) and lengths.is_cuda):
            lengths = torch.as_tensor(lengths, dtype=torch.int64).reshape(-1).to(logits.device)   # numpy lengths, as lm.py takes
        fusion = self._call_fusion(logits.shape[0], hotwords, hotword_weight)
        out = _beam_search(logits, self.blank_id, lengths, 1, self.beam_width, self.token_min_logp, self.beam_prune_logp,
                           self.max_candidates, self.vocab, fusion)
        preds = self._texts(out[0], out[1], decode_func)
        return preds[0] if single else preds


# ---- streaming (resumable) search: INTEGRATION.md "Streaming (resumable) search" ------------------------------------------

def nbest_rows(tokens: torch.Tensor, counts: torch.Tensor, num_hyps: Optional[torch.Tensor], max_len: Optional[int],
               who: str = "ctc_nbest_scores") -> Tuple[torch.Tensor, int]:
    """(hyp_len (B,N) int64 with -1 in the rows n >= num_hyps[b], the lattice width) of an n-best list as the search returns
    it.  max_len=None reads counts.max() on the host: the ONE synchronisation of the n-best scores."""
    if not (isinstance(tokens, torch.Tensor) and tokens.dim() == 3 and isinstance(counts, torch.Tensor)
            and tuple(counts.shape) == tuple(tokens.shape[:2])):
        raise ValueError(f"{who}: tokens must be (B,N,L) with counts (B,N)")
    hyp_len = counts.to(torch.int64)
    if num_hyps is not None:
        if tuple(num_hyps.shape) != (tokens.shape[0],):
            raise ValueError(f"{who}: num_hyps must be (B), got {tuple(num_hyps.shape)}")
        n = torch.arange(tokens.shape[1], device=counts.device)
        hyp_len = hyp_len.masked_fill(n[None, :] >= num_hyps.to(counts.device)[:, None], -1)
    if max_len is None:
        max_len = int(hyp_len.max()) if hyp_len.numel() else 0
    elif not isinstance(max_len, int) or isinstance(max_len, bool) or max_len < 0:
        raise ValueError(f"{who}: max_len must be a non-negative int or None, got {max_len!r}")
    return hyp_len, max_len


def ctc_nbest_scores(logits: torch.Tensor, tokens: torch.Tensor, counts: torch.Tensor, blank_id: int,
                     lengths: Optional[torch.Tensor] = None, num_hyps: Optional[torch.Tensor] = None,
                     max_len: Optional[int] = None) -> torch.Tensor:
    """The exact CTC log-likelihood log p(tokens[b, n] | logits[b]) of every hypothesis of an n-best list: ll (B,N) float64.
    The beam search's scores are pruned sums; these run over the full lattice, all N rows of an utterance against its one
    logits block (INTEGRATION.md "MWER training and n-best scores").  logits (B,T,V) on the HIP device (fp32, or bf16 / fp16
    cast to fp32); tokens (B,N,L) int64 and counts (B,N) int64 as the search returns them (positions at or behind a count are
    never read); lengths (B) int64: frames per utterance (None: all).  num_hyps (B), as the search returns it, marks the rows
    n >= num_hyps[b] UNUSED; without it a row of count 0 is the empty hypothesis.  ll is -inf for an unused row and for a row
    without an alignment (more labels plus repeats than frames).
    max_len=None reads counts.max() once on the host -- the one synchronisation; an int avoids it and bounds the lattice width
    (a longer row is cut to it).  Differentiable with respect to the logits when they require grad."""
    from . import autograd as ag
    x = logits.float() if isinstance(logits, torch.Tensor) and logits.dtype in (torch.bfloat16, torch.float16) else logits
    x = ops._req(x, "logits")
    hyp_len, max_len = nbest_rows(tokens, counts, num_hyps, max_len)
    if lengths is None:
        lengths = torch.full((x.shape[0],), x.shape[1], dtype=torch.int64, device=x.device)
    return ag.CtcNbestScoreFn.apply(x, tokens, hyp_len, lengths, int(blank_id), max_len)


def nbest_posterior(logits: torch.Tensor, tokens: torch.Tensor, counts: torch.Tensor, blank_id: int,
                    lengths: Optional[torch.Tensor] = None, num_hyps: Optional[torch.Tensor] = None,
                    max_len: Optional[int] = None) -> torch.Tensor:
    """The posterior of every hypothesis within its n-best list, (B,N) fp32: the softmax of ctc_nbest_scores over the live rows
    (used, with an alignment), formed in float64; unused and infeasible rows get 0, and so does a list without a live row.  Row
    0's value is an utterance-level confidence, and the filter for pseudo-labels.  Arguments as ctc_nbest_scores."""
    ll = ctc_nbest_scores(logits, tokens, counts, blank_id, lengths, num_hyps, max_len)
    live = torch.isfinite(ll)
    ll = ll.masked_fill(~live, -math.inf)
    top = ll.amax(dim=1, keepdim=True).masked_fill(~live.any(dim=1, keepdim=True), 0.0)
    e = (ll - top).exp()                                     # 0 for a dead row
    return (e / e.sum(dim=1, keepdim=True).clamp_min(1e-300)).float()


class _StreamState:
    """The device buffer of one resumable search and the mode it was initialised for (what beam_ctc_stream_* pass back)."""

    def __init__(self, buf: torch.Tensor, B: int, t_max: int, beam_width: int, max_candidates: int, fusion: _Fusion) -> None:
        self.buf, self.B, self.t_max = buf, B, t_max
        self.beam_width, self.max_candidates = beam_width, max_candidates
        self.fusion = fusion
        self.t_used = 0                    # chunk frames stepped since the init: a bound on what any utterance consumed
        # commit mode (beam_ctc_stream_init(max_pending=...)): t_max is the tree's max_pending + max_chunk_frames frames
        self.max_pending: Optional[int] = None
        self.max_chunk_frames: Optional[int] = None
        self.log: Optional[torch.Tensor] = None          # (B, L) int32 ring of committed tokens
        self.total: Optional[torch.Tensor] = None        # (B) int64 tokens committed since the init / the slot's reset
        self.committed: Optional[torch.Tensor] = None    # (B) int32 tokens the latest step committed
        # timestamps (beam_ctc_stream_init(times=True)): the times buffer beside `buf`, and in commit mode the rings beside `log`
        self.times: Optional[torch.Tensor] = None
        self.log_frames: Optional[torch.Tensor] = None   # (B, L) int64
        self.log_logp: Optional[torch.Tensor] = None     # (B, L) fp32
        # per-request hotwords (beam_ctc_stream_init(hotword_rows=...)): the reserved regions (fusion.rows holds the arrays)
        self.regions: Optional["_HotwordRegions"] = None

    def times_outputs(self, N: int):
        """(times buffer, its size, token_frames, token_logp) as the *_times entries take them, and the pair they fill"""
        tf = torch.empty(self.B, N, self.t_max, dtype=torch.int64, device=self.buf.device)
        tl = torch.empty(self.B, N, self.t_max, dtype=torch.float32, device=self.buf.device)
        return (self.times.data_ptr(), self.times.numel(), tf.data_ptr(), tl.data_ptr()), (tf, tl)


class _HotwordRegions:
    """The reservation of a stream with per-request hotwords: one uint8 tensor of B regions of `stride` bytes (each large enough
    for any list within `bounds`, each starting as the table of the empty list), the (B) int64 pointers the search reads -- to
    an utterance's own region, or to `shared`, the decoder's own table -- and the (B) float64 weights.  Nothing is allocated
    on the device after construction."""

    def __init__(self, B: int, bounds, vocab: Sequence[str], delim_token: str, skip_ids, device, shared: Optional[torch.Tensor],
                 weight: float) -> None:
        self.bounds = _hw.check_bounds(bounds)
        self.vocab, self.delim_token, self.skip = list(vocab), delim_token, frozenset(int(i) for i in skip_ids)
        self.empty = torch.from_numpy(_hw._EMPTY.pack(self.vocab, delim_token, self.skip))
        self.stride = _hw._align(_hw.reserved_bytes(*self.bounds, self.vocab, delim_token, self.skip))
        self.shared, self.default_weight = shared, _hw.row_weight(weight, 0.0)
        self.buf = torch.empty(B * self.stride, dtype=torch.uint8, device=device)
        self.buf.view(B, self.stride)[:, :self.empty.numel()] = self.empty.to(device)
        base = self.buf.data_ptr()
        self.own = [base + b * self.stride for b in range(B)]
        ptrs = self.own if shared is None else [shared.data_ptr()] * B
        self.ptrs = torch.tensor(ptrs, dtype=torch.int64).to(device)
        self.weights = torch.full((B,), self.default_weight, dtype=torch.float64).to(device)

    def pack(self, hotwords, who: str) -> torch.Tensor:
        """The table of a list (a Hotwords or phrases) as a host tensor, refused with ValueError over the reserved bounds."""
        hw = hotwords if isinstance(hotwords, Hotwords) else Hotwords(hotwords)
        _hw.fits(hw, self.bounds, who)
        if not len(hw):
            return self.empty
        blob = hw.pack(self.vocab, self.delim_token, self.skip) if hotwords is hw else hw._pack(self.vocab, self.delim_token, self.skip)
        if blob.nbytes > self.stride:            # (reserved_bytes is an upper bound: not reached)
            raise ValueError(f"{who}: a table of {blob.nbytes} bytes, the region holds {self.stride}")
        return torch.from_numpy(blob)


def beam_ctc_stream_set_hotwords(st: "_StreamState", b: int, table: Optional[torch.Tensor], weight: float) -> None:
    """Utterance b of a state made with hotword_rows= takes `table` (a packed host table, _HotwordRegions.pack; None: the shared
    table the state was made with, or no hotwords without one) and `weight`.  The caller guarantees that b's search is at the
    empty prefix.  The table, the pointer and the weight go through ONE fresh pinned tensor per call (so no copy in flight ever
    reads memory that is written again) and the copies are only enqueued on the current stream."""
    r = st.regions
    if r is None:
        raise ValueError("beam_ctc_stream_set_hotwords: the state was made without hotword_rows")
    b = int(b)
    if not 0 <= b < st.B:
        raise ValueError(f"beam_ctc_stream_set_hotwords: utterance {b} outside [0, {st.B})")
    if table is None and r.shared is None:
        table = r.empty
    n = 0 if table is None else table.numel()
    n8 = (n + 7) // 8 * 8
    host = torch.empty(n8 + 16, dtype=torch.uint8, pin_memory=r.buf.is_cuda)
    if n:
        host[:n] = table
    host[n8:n8 + 8].view(torch.int64)[0] = r.shared.data_ptr() if table is None else r.own[b]
    host[n8 + 8:].view(torch.float64)[0] = _hw.row_weight(weight, r.default_weight)
    if n:
        r.buf[b * r.stride:b * r.stride + n].copy_(host[:n], non_blocking=True)
    r.ptrs[b:b + 1].copy_(host[n8:n8 + 8].view(torch.int64), non_blocking=True)
    r.weights[b:b + 1].copy_(host[n8 + 8:].view(torch.float64), non_blocking=True)


def _commit_args(who: str, max_frames, max_pending, max_chunk_frames, commit_log=4096):
    """The sizing arguments of a search, checked on the host: None (the search ends at max_frames) or (M, k_cap)."""
    if max_pending is None and max_chunk_frames is None:
        if max_frames is None:
            raise ValueError(f"{who}: max_frames=None (a stream without an end) needs max_pending and max_chunk_frames")
        return None
    if max_pending is None:
        raise ValueError(f"{who}: max_chunk_frames sizes the tree of commit mode: give max_pending too")
    if max_chunk_frames is None:
        raise ValueError(f"{who}: max_pending needs max_chunk_frames (the tree is sized for the largest step)")
    if max_frames is not None:
        raise ValueError(f"{who}: max_frames={max_frames} together with max_pending: a committing search has no end, pass "
                         "max_frames=None")
    M, k_cap = int(max_pending), int(max_chunk_frames)
    if M < 1 or k_cap < 1:
        raise ValueError(f"{who}: max_pending and max_chunk_frames must be >= 1, got {M} and {k_cap}")
    if int(commit_log) < 1:
        raise ValueError(f"{who}: commit_log must be >= 1 token, got {commit_log}")
    return M, k_cap


def beam_ctc_stream_init(batch: int, max_frames: Optional[int], device, *, beam_width: int = 100, max_candidates: int = 16,
                         lm_tables: Optional[torch.Tensor] = None, hw_tables: Optional[torch.Tensor] = None,
                         alpha: float = 2.1, beta: float = 9.2, unk_score_offset: float = -10.0, score_boundary: bool = True,
                         hotword_weight: float = 9.0, max_pending: Optional[int] = None,
                         max_chunk_frames: Optional[int] = None, commit_log: int = 4096, times: bool = False,
                         hotword_rows: Optional[Tuple[int, int]] = None, vocab: Optional[Sequence[str]] = None,
                         delim_token: str = "|", skip_ids: Sequence[int] = ()) -> _StreamState:
    """Allocate and initialise the state of a resumable CTC prefix beam search over `batch` utterances of at most
    `max_frames` frames, every utterance at the empty prefix.  `lm_tables` / `hw_tables`: the device blobs of
    NgramLanguageModel.device_tables / Hotwords.device_tables (None: not used).  Enqueues only.
    Commit mode: max_pending = M tokens with max_chunk_frames = k_cap logit frames per step and max_frames=None.  The state is
    then sized by (B, M, k_cap, W, K, lm, hw) alone and the stream has no end; the committed tokens go to a ring of
    max(commit_log, M + k_cap) tokens per utterance (beam_ctc_stream_committed reads it).
    times: the search records token timestamps (INTEGRATION.md "Beam-search timestamps") in a buffer beside the state; step and
    finish then return a trailing (token_frames, token_logp) and the commit log has frames and log-probabilities beside it.
    hotword_rows=(max_phrases, max_code_points) with vocab (and delim_token, skip_ids): per-request hotwords (INTEGRATION.md
    "Per-request hotwords").  The state reserves, per utterance, a table region for any list within those bounds (each starts
    as the table of the empty list), a table pointer and a weight; every utterance starts with `hw_tables` (None: no hotwords)
    and `hotword_weight`, and beam_ctc_stream_set_hotwords gives one its own.  Nothing is allocated after this call."""
    _flag("beam_ctc_stream_init", "times", times)
    commit = _commit_args("beam_ctc_stream_init", max_frames, max_pending, max_chunk_frames, commit_log)
    regions = None
    if hotword_rows is not None:
        if vocab is None:
            raise ValueError("beam_ctc_stream_init: hotword_rows needs vocab (the tables spell the tokens)")
        regions = _HotwordRegions(int(batch), hotword_rows, vocab, delim_token, skip_ids, device, hw_tables, hotword_weight)
        fusion = _Fusion(lm_tables, None, alpha, beta, unk_score_offset, score_boundary,
                         rows=(regions.buf, regions.ptrs, regions.weights))
    else:
        fusion = _Fusion(lm_tables, hw_tables, alpha, beta, unk_score_offset, score_boundary, hotword_weight)
    st = _stream_alloc("beam_ctc_stream_init", int(batch), max_frames, device, int(beam_width), int(max_candidates), fusion,
                       commit, commit_log, times)
    st.regions = regions
    return st


def _stream_alloc(who: str, B: int, max_frames: Optional[int], device, W: int, K: int, fusion: _Fusion, commit, commit_log: int,
                  times: bool) -> _StreamState:
    """The buffers of a resumable search (commit: None or (M, k_cap) of _commit_args), initialised."""
    lib = _lib.load()
    lm, hw = int(fusion.lm_tables is not None), int(fusion.hw_tables is not None)
    if commit is None:
        Tm = int(max_frames)
        nbytes = int(lib.cfm_ctc_beam_stream_state_bytes(B, Tm, W, K, lm, hw))
    else:
        Tm = commit[0] + commit[1]
        nbytes = int(lib.cfm_ctc_beam_commit_state_bytes(B, commit[0], commit[1], W, K, lm, hw))
    tbytes = int(lib.cfm_ctc_beam_times_bytes(B, Tm, W, 0 if commit is None else commit[0])) if times and nbytes else 0
    if nbytes == 0 or (times and tbytes == 0):
        raise ValueError(f"{who}: unsupported arguments (B={B}, max_frames={max_frames}, beam_width={W}, max_candidates={K}, "
                         f"(max_pending, max_chunk_frames)={commit})")
    buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
    st = _StreamState(buf, B, Tm, W, K, fusion)
    if commit is not None:
        st.max_pending, st.max_chunk_frames = commit
        st.log = torch.zeros(B, max(int(commit_log), Tm), dtype=torch.int32, device=device)
        st.total = torch.zeros(B, dtype=torch.int64, device=device)
    if times:
        st.times = torch.empty(tbytes, dtype=torch.uint8, device=device)
        if commit is not None:
            st.log_frames = torch.full(st.log.shape, -1, dtype=torch.int64, device=device)
            st.log_logp = torch.full(st.log.shape, -math.inf, dtype=torch.float32, device=device)
    beam_ctc_stream_reset(st)
    return st


def beam_ctc_stream_reset(st: _StreamState) -> None:
    """Every utterance back at the empty prefix (enqueues only)."""
    f = st.fusion
    _lib.call("cfm_ctc_beam_stream_init", st.B, st.t_max, st.beam_width, st.max_candidates, ops._p(f.lm_tables), f.score_boundary,
              ops._p(f.hw_tables), st.buf.data_ptr(), st.buf.numel(), ops._stream())
    st.t_used = 0
    if st.max_pending is not None:
        st.total.zero_()
        st.committed = None
    if st.times is not None:               # (every utterance's frames count from 0 again)
        _lib.call("cfm_ctc_beam_times_reset", st.B, None, 0, st.times.data_ptr(), st.times.numel(), ops._stream())


def beam_ctc_stream_reset_slots(st: _StreamState, slots: torch.Tensor) -> None:
    """The utterances `slots` ((n) int64 device tensor of batch rows) back at the empty prefix, the others untouched
    (independent streams, conformer_amd/slots.py; enqueues only)."""
    slots = ops._req(slots, "slots", torch.int64)
    if slots.dim() != 1 or not 1 <= slots.numel() <= st.B or not slots.is_contiguous():
        raise ValueError(f"beam_ctc_stream_reset_slots: expected 1..{st.B} slot indices, got shape {tuple(slots.shape)}")
    f = st.fusion
    _lib.call("cfm_ctc_beam_stream_reset_slots", st.B, st.t_max, st.beam_width, st.max_candidates, ops._p(f.lm_tables),
              f.score_boundary, ops._p(f.hw_tables), slots.data_ptr(), slots.numel(), st.buf.data_ptr(), st.buf.numel(),
              ops._stream())
    if st.max_pending is not None:         # (the slots' committed prefixes are empty again; the other slots' logs stay)
        _lib.call("cfm_ctc_beam_commit_reset_slots", st.B, slots.data_ptr(), slots.numel(), st.total.data_ptr(), ops._stream())
    if st.times is not None:               # (a slot's frames count from its own opening)
        _lib.call("cfm_ctc_beam_times_reset", st.B, slots.data_ptr(), slots.numel(), st.times.data_ptr(), st.times.numel(),
                  ops._stream())


def beam_ctc_stream_step(st: _StreamState, logits: torch.Tensor, blank_id: int, lengths: Optional[torch.Tensor] = None, *,
                         n_best: int = 1, token_min_logp: float = -5.0, beam_prune_logp: float = -10.0,
                         t_used: Optional[int] = None):
    """Consume the next chunk logits (B,Tc,V) (fp32, or bf16 / fp16 cast to fp32): per utterance its first lengths[b] frames
    (None: all).  Returns the interim best (tokens (B,N,max_frames) int64 padded with -1, counts (B,N), scores (B,N) fp32
    without end-of-utterance terms, am_scores (B,N) fp32 or None without LM and hotwords, num_hyps (B)), device tensors;
    nothing synchronises with the host.  t_used: the caller's own bound on the frames any utterance consumed before this
    step (independent streams pass max_b(frames_b + lengths_b) - Tc, having checked frames_b + lengths_b <= max_frames);
    None: the chunk frames stepped since the init, which this call then advances.
    Commit mode: Tc <= max_chunk_frames; the step is followed by the commit, the returned tokens are (B,N,max_pending +
    max_chunk_frames) and relative to the committed prefix as it was BEFORE this step (st.committed: the (B) int32 tokens this
    step then committed, so the pending best is tokens[b, r, st.committed[b]:counts[b, r]]); t_used is taken as a bound on
    the frames stepped and capped at max_pending, which bounds what the tree holds after a commit.
    A state made with times=True: the result gains a trailing pair (token_frames, token_logp), shaped and padded like tokens."""
    x = _logits(logits)
    if x.dim() != 3 or x.shape[0] != st.B:
        raise ValueError(f"logits: expected ({st.B},Tc,V), got {tuple(x.shape)}")
    _, Tc, V = x.shape
    if Tc < 1:
        raise ValueError("beam_ctc_stream_step: the chunk has no frames")
    used = st.t_used if t_used is None else int(t_used)
    if st.max_pending is not None:
        if Tc > st.max_chunk_frames:
            raise ValueError(f"beam_ctc_stream_step: a chunk of {Tc} frames, the tree was sized for max_chunk_frames="
                             f"{st.max_chunk_frames}")
        used = min(used, st.max_pending)
    if used < 0 or Tc > st.t_max - used:
        raise ValueError(f"beam_ctc_stream_step: {Tc} more frames would pass max_frames={st.t_max} "
                         f"({used} stepped so far)")
    if lengths is not None:
        lengths = ops._req(lengths, "lengths", torch.int64)
    tokens, counts, scores, am_scores, num_hyps = _beam_outputs(st.B, int(n_best), st.t_max, x.device, st.fusion.fused)
    step = (x.data_ptr(), ops._p(lengths), st.B, Tc, V, int(blank_id), st.beam_width, st.max_candidates, float(token_min_logp),
            float(beam_prune_logp), int(n_best), *st.fusion.args, st.buf.data_ptr(), st.buf.numel(), st.t_max, used,
            tokens.data_ptr(), counts.data_ptr(), scores.data_ptr(), ops._p(am_scores), num_hyps.data_ptr())
    pair = None
    if st.times is not None:
        targs, pair = st.times_outputs(int(n_best))
    if st.fusion.rows is not None:         # per-request hotwords: one entry, the times group nullable
        _lib.call("cfm3_ctc_beam_hw_rows_stream_step_f32", *step, *(targs if pair is not None else _NO_TIMES), ops._stream())
    elif st.times is None:
        _lib.call("cfm_ctc_beam_stream_step_f32", *step, ops._stream())
    else:
        _lib.call("cfm_ctc_beam_stream_step_times_f32", *step, *targs, ops._stream())
    if t_used is None:
        st.t_used += Tc
    if st.max_pending is not None:
        st.committed = torch.empty(st.B, dtype=torch.int32, device=x.device)
        f = st.fusion
        commit = (st.B, st.max_pending, st.max_chunk_frames, st.beam_width, st.max_candidates, int(f.lm_tables is not None),
                  int(f.hw_tables is not None), ops._p(lengths), st.buf.data_ptr(), st.buf.numel(), st.log.data_ptr(),
                  st.log.shape[1], st.total.data_ptr(), st.committed.data_ptr())
        if st.times is None:
            _lib.call("cfm_ctc_beam_stream_commit", *commit, ops._stream())
        else:
            _lib.call("cfm_ctc_beam_stream_commit_times", *commit, st.times.data_ptr(), st.times.numel(),
                      st.log_frames.data_ptr(), st.log_logp.data_ptr(), ops._stream())
    if pair is not None:
        return tokens, counts, scores, am_scores, num_hyps, pair
    return tokens, counts, scores, am_scores, num_hyps


def beam_ctc_stream_committed(st: _StreamState, popped: Sequence[int], only: Optional[Sequence[int]] = None,
                              times: bool = False):
    """Commit mode: per utterance the committed tokens from position popped[b] on, and the totals.  Synchronises.  `only`: the
    utterances to read (the others get an empty list and are not checked; only their rows of the log are copied).  RuntimeError
    naming the utterances, before anything is copied, where more than the ring holds were committed since popped[b] (the
    oldest are overwritten).  times (a state made with times=True): (tokens, totals, frames, logps), the frames and
    log-probabilities of the same rows and positions."""
    rows = list(range(st.B)) if only is None else [int(b) for b in only]
    total = st.total.cpu().tolist()
    L = st.log.shape[1]
    over = [b for b in rows if total[b] - popped[b] > L]
    if over:
        raise RuntimeError(f"utterance(s) {over}: {[total[b] - popped[b] for b in over]} tokens committed since the last pop, the "
                           f"commit log holds {L}: pop more often, give a larger commit_log, or discard them")
    out: List[List[int]] = [[] for _ in range(st.B)]
    frames: List[List[int]] = [[] for _ in range(st.B)]
    logps: List[List[float]] = [[] for _ in range(st.B)]
    if rows:
        def copy(ring):
            return ring.cpu() if only is None else ring[torch.tensor(rows, device=ring.device)].cpu()
        log = copy(st.log)
        lf, ll = (copy(st.log_frames), copy(st.log_logp)) if times else (None, None)
        for i, b in enumerate(rows):
            at = torch.arange(popped[b], total[b]) % L
            out[b] = log[i, at].tolist()
            if times:
                frames[b], logps[b] = lf[i, at].tolist(), ll[i, at].tolist()
    if times:
        return out, total, frames, logps
    return out, total


def beam_ctc_stream_finish(st: _StreamState, n_best: int = 1):
    """The end-of-utterance step over the consumed frames: (tokens (B,N,max_frames), counts, scores, am_scores or None
    without LM and hotwords, num_hyps), equal bit for bit to one-shot decoding of the consumed frames (with T = max_frames).
    Commit mode: the tokens are (B,N,max_pending + max_chunk_frames) and follow the committed prefix (st.log / st.total).
    A state made with times=True: the result gains a trailing pair (token_frames, token_logp)."""
    tokens, counts, scores, am_scores, num_hyps = _beam_outputs(st.B, int(n_best), st.t_max, st.buf.device,
                                                                st.fusion.fused)
    fin = (st.B, st.beam_width, st.max_candidates, int(n_best), *st.fusion.args, st.buf.data_ptr(), st.buf.numel(), st.t_max,
           tokens.data_ptr(), counts.data_ptr(), scores.data_ptr(), ops._p(am_scores), num_hyps.data_ptr())
    rows = st.fusion.rows is not None
    if st.times is None:
        if rows:
            _lib.call("cfm3_ctc_beam_hw_rows_stream_finish_f32", *fin, *_NO_TIMES, ops._stream())
        else:
            _lib.call("cfm_ctc_beam_stream_finish_f32", *fin, ops._stream())
        return tokens, counts, scores, am_scores, num_hyps
    targs, pair = st.times_outputs(int(n_best))
    _lib.call("cfm3_ctc_beam_hw_rows_stream_finish_f32" if rows else "cfm_ctc_beam_stream_finish_times_f32", *fin, *targs,
              ops._stream())
    return tokens, counts, scores, am_scores, num_hyps, pair


class BeamCTCStream:
    """A BeamCTCDecoder's search over a stream of logits chunks (BeamCTCDecoder.stream).  `step` enqueues the chunk and returns
    the interim best as device tensors; `partial_text` is the one call that synchronises; `finish` returns the strings
    BeamCTCDecoder.__call__ returns on the concatenated logits; `reset` starts a new batch of utterances.
    Commit mode (max_pending, max_chunk_frames, max_frames=None): the stream has no end.  `pop_committed` hands out the tokens
    that have become final since the previous pop; `committed_text`, `partial_text` and `finish` speak of the text from the
    last pop on: (unpopped committed) [+ pending best | + final tokens], joined as token ids before `decoder.text`.
    Independent utterances (conformer_amd/slots.py): `step(t_used=)` takes the caller's bound, `reset_slots` starts some again
    and `only=` reads (`finish`: ends) those utterances alone; the returned lists keep length B, "" or [] for the others.
    times=True (INTEGRATION.md "Beam-search timestamps"): the search records when each token entered, and the stream hands out
    align.Words: `partial_words`, `finish_words` and, in commit mode, `pop_committed_words`, which returns complete words only and
    HOLDS the committed tokens after the last committed delimiter on the host until their delimiter is committed or the stream
    finishes.  Held tokens count as popped: `pop_committed` never returns them, while the texts and words of `partial_*`,
    `committed_text` and `finish*` still begin with them.
    hotword_rows=(max_phrases, max_code_points) (INTEGRATION.md "Per-request hotwords"): every utterance starts with the
    decoder's own list and weight, and `set_hotwords(b, ...)` gives utterance b its own while its search is at the empty prefix:
    after construction, `reset` or `reset_slots`, before the next `step`.  `reset` and `reset_slots` do not change the lists."""

    def __init__(self, decoder: "BeamCTCDecoder", batch: int, max_frames: Optional[int], device=None, *,
                 max_pending: Optional[int] = None, max_chunk_frames: Optional[int] = None, commit_log: int = 4096,
                 times: bool = False, frame_seconds: float = 0.04, hotword_rows: Optional[Tuple[int, int]] = None) -> None:
        self.times = _flag("BeamCTCStream", "times", times)
        self.frame_seconds = positive_seconds("BeamCTCStream", "frame_seconds", frame_seconds)
        self.commit = _commit_args("BeamCTCStream", max_frames, max_pending, max_chunk_frames, commit_log) is not None
        self.decoder = decoder
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        d, f = decoder, decoder._fusion(self.device)
        self.state = beam_ctc_stream_init(batch, max_frames, self.device, beam_width=d.beam_width,
                                          max_candidates=d.max_candidates, lm_tables=f.lm_tables, hw_tables=f.hw_tables,
                                          alpha=d.alpha, beta=d.beta, unk_score_offset=d.unk_score_offset,
                                          score_boundary=d.score_boundary, hotword_weight=d.hotword_weight,
                                          max_pending=max_pending, max_chunk_frames=max_chunk_frames, commit_log=commit_log,
                                          times=self.times,
                                          **({} if hotword_rows is None else dict(
                                              hotword_rows=hotword_rows, vocab=d.vocab, delim_token=d.delim_token,
                                              skip_ids=tuple(sorted(d.skip_ids)))))
        self.finished = False
        self.last = None                   # interim outputs of the latest step
        self.last_committed = None         # commit mode: the (B) tokens the latest step committed
        self.popped = [0] * int(batch)     # commit mode: committed tokens handed out by pop_committed, per utterance
        self.fresh = set(range(int(batch)))    # utterances reset since the latest step: `last` holds no row of theirs
        # times: per utterance the (id, frame, logp) of the committed tokens pop_committed_words took but has not handed out
        self.held: List[List[Tuple[int, int, float]]] = [[] for _ in range(int(batch))]

    def step(self, logits_chunk: torch.Tensor, lengths: Optional[torch.Tensor] = None, *, t_used: Optional[int] = None):
        """logits_chunk (B,Tc,V): the next frames of every utterance; `lengths` (B) int64: frames of the chunk to consume per
        utterance (None: all); t_used: beam_ctc_stream_step.  Returns (tokens (B,1,max_frames), counts (B,1), scores (B,1))."""
        if self.finished:
            raise RuntimeError("BeamCTCStream.step after finish(): call reset() to start a new stream")
        d = self.decoder
        if lengths is not None and not (isinstance(lengths, torch.Tensor) and lengths.is_cuda):
            lengths = torch.as_tensor(lengths, dtype=torch.int64).reshape(-1).to(self.device)
        out = beam_ctc_stream_step(self.state, logits_chunk, d.blank_id, lengths, n_best=1, token_min_logp=d.token_min_logp,
                                   beam_prune_logp=d.beam_prune_logp, t_used=t_used)
        self.last = out
        self.last_committed = self.state.committed if self.commit else None
        self.fresh.clear()
        return out[0], out[1], out[2]

    def plan_hotwords(self, hotwords, hotword_weight=None):
        """The host half of set_hotwords: (table or None, weight), packed and checked; ValueError (naming the limit) for a list
        over the reserved bounds, a malformed list or a non-finite weight.  Nothing is enqueued."""
        r = self.state.regions
        if r is None:
            raise ValueError("BeamCTCStream.set_hotwords: the stream was made without hotword_rows=(max_phrases, "
                             "max_code_points), no table region is reserved")
        weight = _hw.row_weight(hotword_weight, r.default_weight)
        return (None if hotwords is None else r.pack(hotwords, "BeamCTCStream.set_hotwords")), weight

    def apply_hotwords(self, b: int, plan) -> None:
        """The device half of set_hotwords for a plan_hotwords result: RuntimeError unless utterance b is at the empty prefix."""
        b = int(b)
        if not 0 <= b < len(self.popped):
            raise ValueError(f"BeamCTCStream.set_hotwords: utterance {b} outside [0, {len(self.popped)})")
        if b not in self.fresh or self.finished:
            raise RuntimeError(f"BeamCTCStream.set_hotwords: utterance {b} has been stepped since its last reset; a hotword list "
                               "can only change at the empty prefix (the saved trie nodes index the old tables): reset() or "
                               "reset_slots([b]) first")
        beam_ctc_stream_set_hotwords(self.state, b, plan[0], plan[1])

    def set_hotwords(self, b: int, hotwords, hotword_weight: Optional[float] = None) -> None:
        """Utterance b's hotword list and weight (a stream made with hotword_rows=).  hotwords: None (the decoder's own list),
        () or [] (no hotwords), a Hotwords, or phrases, which replace the decoder's list; hotword_weight: None is the
        decoder's.  Packs on the host, then only enqueues the copies into b's reserved region on the current stream.
        ValueError, before anything is enqueued, for a list over the reserved bounds; RuntimeError once b has been stepped
        since its last reset (a step with lengths[b] == 0 counts: the host does not read the lengths)."""
        self.apply_hotwords(b, self.plan_hotwords(hotwords, hotword_weight))

    def reset_slots(self, slots: Sequence[int]) -> None:
        """The utterances `slots` (host ints) back at the empty prefix with nothing committed and nothing popped, the others
        untouched; until the next step their partial text is empty.  Enqueues only.  `finished` stays as it is."""
        slots = [int(b) for b in slots]
        idx = torch.tensor(slots, dtype=torch.int64)
        if self.device.type == "cuda":
            idx = idx.pin_memory().to(self.device, non_blocking=True)
        beam_ctc_stream_reset_slots(self.state, idx)       # (commit mode: the utterances' committed totals too)
        for b in slots:
            self.popped[b] = 0
            self.held[b] = []
        self.fresh.update(slots)

    def _need_commit(self, what: str) -> None:
        if not self.commit:
            raise RuntimeError(f"BeamCTCStream.{what}: the stream was made without max_pending, nothing is committed before "
                               "finish()")

    def _rows(self, only: Optional[Sequence[int]]) -> List[int]:
        return list(range(len(self.popped))) if only is None else [int(b) for b in only]

    def _unpopped(self, only: Optional[Sequence[int]] = None) -> Tuple[List[List[int]], List[int]]:
        if not self.commit:                # nothing is committed before the end
            return [[] for _ in self.popped], self.popped
        return beam_ctc_stream_committed(self.state, self.popped, only)

    def _from_last_pop(self, only: Optional[Sequence[int]] = None) -> List[List[int]]:
        """Per utterance the token ids the texts begin with: the held tokens (times), then the unpopped committed ones."""
        ids = self._unpopped(only)[0]
        return [[t[0] for t in h] + i for h, i in zip(self.held, ids)]

    # ---- words (times=True)
    def _need_times(self, what: str) -> None:
        if not self.times:
            raise RuntimeError(f"BeamCTCStream.{what}: the stream was made without times=True, the search recorded no timestamps")

    def _unpopped_timed(self, only: Optional[Sequence[int]] = None):
        """Per utterance the (id, frame, logp) of the held tokens and then of the unpopped committed ones; the totals."""
        if not self.commit:
            return [list(h) for h in self.held], self.popped
        ids, total, frames, logps = beam_ctc_stream_committed(self.state, self.popped, only, times=True)
        return [h + list(zip(i, f, p)) for h, i, f, p in zip(self.held, ids, frames, logps)], total

    def _words(self, timed: Sequence[Tuple[int, int, float]]) -> List[Word]:
        return token_words(self.decoder, [t[0] for t in timed], [t[1] for t in timed], [t[2] for t in timed],
                           self.frame_seconds)

    def pop_committed_words(self, only: Optional[Sequence[int]] = None) -> List[List[Word]]:
        """Commit mode with times: per utterance the COMPLETE words committed since the previous pop: the committed tokens up
        to the last committed delimiter.  The committed tokens after it are held on the host until their delimiter is committed
        (or finish_words ends the stream); they count as popped, so pop_committed never returns them.  Synchronises; raises
        like pop_committed, with nothing popped, when the commit log was lapped."""
        self._need_times("pop_committed_words")
        self._need_commit("pop_committed_words")
        timed, total = self._unpopped_timed(only)
        v = self.decoder.vocab
        delim = v.index(self.decoder.delim_token) if self.decoder.delim_token in v else None
        words: List[List[Word]] = [[] for _ in self.popped]
        for b in self._rows(only):
            seq = timed[b]
            cut = max((i + 1 for i, t in enumerate(seq) if t[0] == delim), default=0)
            words[b] = self._words(seq[:cut])
            self.held[b] = seq[cut:]
            self.popped[b] = total[b]
        return words

    def partial_words(self, only: Optional[Sequence[int]] = None) -> List[List[Word]]:
        """With times: the words of partial_text: the held tokens, the committed tokens not yet popped and the pending best
        of the latest step ([] before the first step and for an utterance reset since).  Changes nothing."""
        self._need_times("partial_words")
        words: List[List[Word]] = [[] for _ in self.popped]
        rows = [b for b in self._rows(only) if b not in self.fresh]
        if not rows:
            return words
        timed = self._unpopped_timed(only)[0]
        tk, ct = self.last[0][:, 0].cpu().tolist(), self.last[1][:, 0].cpu().tolist()
        fr, lp = self.last[5][0][:, 0].cpu().tolist(), self.last[5][1][:, 0].cpu().tolist()
        nc = self.last_committed.cpu().tolist() if self.commit else [0] * len(ct)
        for b in rows:
            words[b] = self._words(timed[b] + list(zip(tk[b][nc[b]:ct[b]], fr[b][nc[b]:ct[b]], lp[b][nc[b]:ct[b]])))
        return words

    def finish_words(self, only: Optional[Sequence[int]] = None) -> List[List[Word]]:
        """With times: the words of finish(): the held tokens, the unpopped committed tokens and the final tokens.  Ends the
        stream as finish() does (only=[...]: those utterances alone)."""
        self._need_times("finish_words")
        if self.finished:
            raise RuntimeError("BeamCTCStream.finish_words() after the finish: call reset() to start a new stream")
        out = beam_ctc_stream_finish(self.state, n_best=1)
        self.finished = only is None
        timed = self._unpopped_timed(only)[0]
        rows = self._rows(only)
        idx = torch.tensor(rows, dtype=torch.int64, device=out[0].device)
        tk, ct = out[0][idx, 0].cpu().tolist(), out[1][idx, 0].cpu().tolist()
        fr, lp = out[5][0][idx, 0].cpu().tolist(), out[5][1][idx, 0].cpu().tolist()
        words: List[List[Word]] = [[] for _ in self.popped]
        for i, b in enumerate(rows):
            n = ct[i]
            words[b] = self._words(timed[b] + list(zip(tk[i][:n], fr[i][:n], lp[i][:n])))
        return words

    def pop_committed(self, only: Optional[Sequence[int]] = None) -> List[List[int]]:
        """Commit mode: per utterance the token ids committed since the previous pop (they will never change), which are then
        forgotten.  Synchronises.  RuntimeError, with nothing popped, if more than commit_log tokens were committed in between."""
        self._need_commit("pop_committed")
        ids, total = self._unpopped(only)
        for b in self._rows(only):
            self.popped[b] = total[b]
        return ids

    def discard_committed(self, only: Optional[Sequence[int]] = None) -> None:
        """Commit mode: forget every committed token not yet popped (the way out after pop_committed raised: the ring was
        lapped and those tokens cannot all be read any more).  Synchronises."""
        self._need_commit("discard_committed")
        total = self.state.total.cpu().tolist()
        for b in self._rows(only):
            self.popped[b] = total[b]

    def committed_text(self, only: Optional[Sequence[int]] = None) -> List[str]:
        """Commit mode: the text of the committed tokens not yet popped."""
        self._need_commit("committed_text")
        return [self.decoder.text(ids) for ids in self._from_last_pop(only)]

    def partial_text(self, only: Optional[Sequence[int]] = None) -> List[str]:
        """The interim best transcript of every utterance after the latest step (empty strings before the first, and for an
        utterance reset since).  Commit mode: from the last pop on, the committed tokens and then the pending best."""
        texts = [""] * len(self.popped)
        rows = [b for b in self._rows(only) if b not in self.fresh]
        if not rows:
            return texts
        ids = self._from_last_pop(only)
        tk, ct = self.last[0][:, 0].cpu().tolist(), self.last[1][:, 0].cpu().tolist()
        nc = self.last_committed.cpu().tolist() if self.commit else [0] * len(ct)     # the best is relative to the prefix before the step
        for b in rows:
            texts[b] = self.decoder.text(ids[b] + tk[b][nc[b]:ct[b]])
        return texts

    def finish(self, decode_func: Optional[Callable[[str], str]] = None, only: Optional[Sequence[int]] = None) -> List[str]:
        """only=[...]: those utterances' end alone (no search state is saved: the others go on); only their rows are copied."""
        if self.finished:
            raise RuntimeError("BeamCTCStream.finish() called twice: call reset() to start a new stream")
        tokens, counts = beam_ctc_stream_finish(self.state, n_best=1)[:2]
        self.finished = only is None
        ids = self._from_last_pop(only)
        if only is None:
            tk, ct = tokens[:, 0].cpu().tolist(), counts[:, 0].cpu().tolist()
        texts = [""] * len(self.popped)
        for b in self._rows(only):
            row = tk[b][:ct[b]] if only is None else tokens[b, 0, :int(counts[b, 0])].tolist()
            text = self.decoder.text(ids[b] + row)
            texts[b] = decode_func(text) if decode_func is not None else text
        return texts

    def reset(self) -> None:
        beam_ctc_stream_reset(self.state)
        self.finished = False
        self.popped = [0] * len(self.popped)
        self.held = [[] for _ in self.popped]
        self.fresh = set(range(len(self.popped)))
