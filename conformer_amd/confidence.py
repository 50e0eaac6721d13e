"""Confidence: how sure was the model of a token or a word?  A number in [0, 1], on the device (INTEGRATION.md "Confidence").

Per frame the posterior softmax(x) is turned into one number that is 0 when it is uniform and 1 when it is one-hot: the
maximum probability, or one minus the linearly normalised Shannon, Tsallis or Renyi entropy (Laptev and Ginsburg, "Fast
entropy-based methods of word-level confidence estimation for end-to-end automatic speech recognition", SLT 2022).  A token or a
word then takes the mean, minimum, maximum or product over its frames; with `exclude_blank` only the frames whose argmax is
not the blank count, as long as there is one.

The frame pass is cfm_confidence_frames_f32, the aggregation cfm_confidence_spans_f32, the greedy decoder's spans
cfm_confidence_greedy_spans_i64 (include/conformer_hip_confidence.h).  A frame's value depends on its V logits alone, so how a
stream is cut into steps changes no bit.  Everything enqueues only, except the two calls that return Python floats for Words
(`word_confidence`, `StreamingConfidence.words`).  There is no CPU path.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib, ops
from ._slot_state import SlotFollower, frame_chunks
from .align import Alignment, Word

_C = _lib.HEADERS["conformer_hip_confidence.h"].constants
METHODS = {"max_prob": _C["CFM_CONFIDENCE_MAX_PROB"], "entropy": _C["CFM_CONFIDENCE_ENTROPY"],
           "tsallis": _C["CFM_CONFIDENCE_TSALLIS"], "renyi": _C["CFM_CONFIDENCE_RENYI"]}
AGGREGATIONS = {"mean": _C["CFM_CONFIDENCE_MEAN"], "min": _C["CFM_CONFIDENCE_MIN"], "max": _C["CFM_CONFIDENCE_MAX"],
                "prod": _C["CFM_CONFIDENCE_PROD"]}
ALPHA_RANGES = ((1 / 16, 15 / 16), (17 / 16, 8.0))     # nearer to 1 the normaliser cancels: "entropy" is that limit
MAX_EXCLUDE_IDS, V_MAX = 8, 65536


@dataclass(frozen=True)
class ConfidenceConfig:
    """method: "max_prob", "entropy", "tsallis" or "renyi" (the last two with `alpha`); aggregation over the frames of a token
    or word: "mean", "min", "max" or "prod"; exclude_blank: frames whose argmax is the blank do not count, unless all are."""
    method: str = "tsallis"
    alpha: float = 0.33
    aggregation: str = "min"
    exclude_blank: bool = True

    def check(self) -> Tuple[int, float, int]:
        """Refuse a bad configuration (ValueError, on the host); (method, alpha, aggregation) as the C entries take them."""
        if self.method not in METHODS:
            raise ValueError(f"ConfidenceConfig: method must be one of {sorted(METHODS)}, got {self.method!r}")
        if self.aggregation not in AGGREGATIONS:
            raise ValueError(f"ConfidenceConfig: aggregation must be one of {sorted(AGGREGATIONS)}, got {self.aggregation!r}")
        if not isinstance(self.exclude_blank, bool):
            raise ValueError(f"ConfidenceConfig: exclude_blank must be True or False, got {self.exclude_blank!r}")
        a = self.alpha
        if isinstance(a, bool) or not isinstance(a, (int, float)) or not math.isfinite(a):
            raise ValueError(f"ConfidenceConfig: alpha must be a finite number, got {a!r}")
        if self.method in ("tsallis", "renyi") and not any(lo <= a <= hi for lo, hi in ALPHA_RANGES):
            raise ValueError(f"ConfidenceConfig: alpha = {a!r} outside [1/16, 15/16] and [17/16, 8] (at 1 the {self.method} "
                             "normaliser is 0/0; method=\"entropy\" is that limit)")
        return METHODS[self.method], float(a), AGGREGATIONS[self.aggregation]


def _config(who: str, config) -> Tuple[int, float, int]:
    if not isinstance(config, ConfidenceConfig):
        raise ValueError(f"{who}: config must be a ConfidenceConfig, got {type(config).__name__}")
    return config.check()


def _exclude(who: str, ids: Sequence[int]) -> List[int]:
    out: List[int] = []
    for i in ids:
        if isinstance(i, bool) or not isinstance(i, int):
            raise ValueError(f"{who}: exclude_ids must be token ids, got {list(ids)}")
        if i not in out:
            out.append(i)
    if len(out) > MAX_EXCLUDE_IDS:
        raise ValueError(f"{who}: {len(out)} exclude_ids, the kernel compares at most {MAX_EXCLUDE_IDS}")
    return out


def _device_logits(logits) -> torch.Tensor:
    """fp32 logits on the device, as decode._logits (bf16 / fp16 cast to fp32) but without asking for contiguity: the entry
    takes the pitches of a view."""
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda:
        raise _lib.ConformerHipError(f"logits: expected a tensor on a HIP device, got {getattr(logits, 'device', type(logits))}; "
                                     "confidence only exists as gfx950 kernels (no CPU fallback)")
    if logits.dtype in (torch.bfloat16, torch.float16):
        logits = logits.float()
    if logits.dtype != torch.float32:
        raise _lib.ConformerHipError(f"logits: expected dtype torch.float32, got {logits.dtype}")
    return logits


def _frames(x: torch.Tensor, k: torch.Tensor, method: int, alpha: float, conf: torch.Tensor, ids: torch.Tensor,
            total: torch.Tensor) -> None:
    """One call of the frame entry on x (S, k_max <= R, V), a view or not."""
    n, V = x.shape[1], x.shape[2]
    if x.stride(2) != 1 or x.stride(1) < V or x.stride(0) < n * x.stride(1):
        x = x.contiguous()
    _lib.call("cfm_confidence_frames_f32", x.data_ptr(), x.stride(0), x.stride(1), k.data_ptr(), n, V, method, alpha,
              conf.data_ptr(), ids.data_ptr(), total.data_ptr(), conf.shape[1], x.shape[0], ops._stream())


def _exclude_ids(exclude: Sequence[int], device) -> Optional[torch.Tensor]:
    """The excluded ids as the span entry takes them: (n) int32 on the device, None for none."""
    if not exclude:
        return None
    return torch.tensor(list(exclude), dtype=torch.int32).pin_memory().to(device, non_blocking=True)


def _spans(conf: torch.Tensor, ids: torch.Tensor, total: torch.Tensor, starts: torch.Tensor, ends: torch.Tensor,
           n_spans: torch.Tensor, aggregation: int, exclude) -> torch.Tensor:
    """One call of the span entry: (S, L) fp32.  exclude: a sequence of ids, or what _exclude_ids made of one."""
    S, L = starts.shape
    out = torch.empty(S, L, dtype=torch.float32, device=conf.device)
    ex = exclude if exclude is None or isinstance(exclude, torch.Tensor) else _exclude_ids(exclude, conf.device)
    _lib.call("cfm_confidence_spans_f32", conf.data_ptr(), ids.data_ptr(), total.data_ptr(), conf.shape[1], starts.data_ptr(),
              ends.data_ptr(), n_spans.data_ptr(), L, aggregation, ops._p(ex), 0 if ex is None else ex.numel(), out.data_ptr(), S,
              ops._stream())
    return out


def _lengths(lengths, B: int, T: int, device) -> torch.Tensor:
    if lengths is None:
        return torch.full((B,), T, dtype=torch.int64, device=device)
    lengths = ops._req(lengths, "lengths", torch.int64)
    if lengths.dim() != 1 or lengths.numel() != B:
        raise ValueError(f"lengths: expected {B} frame counts, got shape {tuple(lengths.shape)}")
    return lengths


@torch.no_grad()
def frame_confidence(logits: torch.Tensor, lengths: Optional[torch.Tensor] = None,
                     config: ConfidenceConfig = ConfidenceConfig()) -> Tuple[torch.Tensor, torch.Tensor]:
    """logits (B, T, V) on the device (fp32; bf16 / fp16 are cast), `lengths` (B) int64 frames per utterance (None: all T).
    Returns (conf (B, T) fp32, frame_ids (B, T) int64): per frame its confidence and its argmax, NaN and -1 behind an
    utterance's length.  Enqueues only."""
    method, alpha, _ = _config("frame_confidence", config)
    x = _device_logits(logits)
    if x.dim() != 3 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"logits: expected (B, T, V), got {tuple(x.shape)}")
    B, T, V = x.shape
    if not 2 <= V <= V_MAX:
        raise ValueError(f"logits: V = {V} outside [2, {V_MAX}]")
    conf = torch.full((B, T), math.nan, dtype=torch.float32, device=x.device)
    ids = torch.full((B, T), -1, dtype=torch.int64, device=x.device)
    total = torch.zeros(B, dtype=torch.int64, device=x.device)
    _frames(x, _lengths(lengths, B, T, x.device), method, alpha, conf, ids, total)
    return conf, ids


def _req_history(conf: torch.Tensor, frame_ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    conf, frame_ids = ops._req(conf, "conf"), ops._req(frame_ids, "frame_ids", torch.int64)
    if conf.dim() != 2 or conf.shape[1] < 1 or frame_ids.shape != conf.shape:
        raise ValueError(f"conf, frame_ids: expected two (B, T) tensors, got {tuple(conf.shape)} and {tuple(frame_ids.shape)}")
    return conf, frame_ids


@torch.no_grad()
def span_confidence(conf: torch.Tensor, frame_ids: torch.Tensor, starts: torch.Tensor, ends: torch.Tensor,
                    lengths: Optional[torch.Tensor] = None, config: ConfidenceConfig = ConfidenceConfig(),
                    exclude_ids: Sequence[int] = ()) -> torch.Tensor:
    """The aggregation of frame_confidence's (conf, frame_ids) over the spans [starts[b, j], ends[b, j]) (B, L) int64, end
    exclusive, clamped to the utterance's length: (B, L) fp32, NaN for an empty span (padding written as -1, -1 is one).  The
    frames whose frame_ids entry is in `exclude_ids` do not count, unless that leaves none.  Enqueues only."""
    _, _, agg = _config("span_confidence", config)
    exclude = _exclude("span_confidence", exclude_ids)
    conf, frame_ids = _req_history(conf, frame_ids)
    B, T = conf.shape
    starts, ends = ops._req(starts, "starts", torch.int64), ops._req(ends, "ends", torch.int64)
    if starts.dim() != 2 or starts.shape[0] != B or ends.shape != starts.shape:
        raise ValueError(f"starts, ends: expected two ({B}, L) tensors, got {tuple(starts.shape)} and {tuple(ends.shape)}")
    n_spans = torch.full((B,), starts.shape[1], dtype=torch.int64, device=conf.device)
    return _spans(conf, frame_ids, _lengths(lengths, B, T, conf.device), starts, ends, n_spans, agg, exclude)


class GreedyConfidence(NamedTuple):
    frame_ids: torch.Tensor         # (B, T) int64: these three are greedy_ctc_decode's, bit for bit
    tokens: torch.Tensor            # (B, T) int64 padded with -1
    counts: torch.Tensor            # (B) int64
    token_start: torch.Tensor       # (B, T) int64: the frame at which token j is emitted, -1 from counts[b] on
    token_end: torch.Tensor         # (B, T) int64: the next token's start, the utterance's length for the last
    token_confidence: torch.Tensor  # (B, T) fp32: the aggregation over [token_start, token_end), NaN from counts[b] on
    frame_confidence: torch.Tensor  # (B, T) fp32, NaN behind the utterance's length


@torch.no_grad()
def greedy_ctc_confidence(logits: torch.Tensor, pad_id: int, unk_id: int, lengths: Optional[torch.Tensor] = None,
                          config: ConfidenceConfig = ConfidenceConfig()) -> GreedyConfidence:
    """greedy_ctc_decode with a confidence per token.  A token's span runs from the frame that emits it to the frame that emits
    the next one; with exclude_blank the pad and unk frames in it do not count.  Enqueues only."""
    from .decode import greedy_ctc_decode
    _, _, agg = _config("greedy_ctc_confidence", config)
    x = ops._req(_device_logits(logits), "logits")
    B, T, _ = x.shape
    frame_ids, tokens, counts = greedy_ctc_decode(x, pad_id, unk_id, lengths)
    conf, _ = frame_confidence(x, lengths, config)
    token_start = torch.empty(B, T, dtype=torch.int64, device=x.device)
    token_end = torch.empty(B, T, dtype=torch.int64, device=x.device)
    lengths = None if lengths is None else _lengths(lengths, B, T, x.device)
    _lib.call("cfm_confidence_greedy_spans_i64", frame_ids.data_ptr(), ops._p(lengths), token_start.data_ptr(),
              token_end.data_ptr(), B, T, int(pad_id), int(unk_id), ops._stream())
    exclude = _exclude("greedy_ctc_confidence", [int(pad_id), int(unk_id)]) if config.exclude_blank else []
    token_conf = _spans(conf, frame_ids, _lengths(lengths, B, T, x.device), token_start, token_end, counts, agg, exclude)
    return GreedyConfidence(frame_ids, tokens, counts, token_start, token_end, token_conf, conf)


def _blank(who: str, blank_id, config: ConfidenceConfig) -> List[int]:
    if isinstance(blank_id, bool) or not isinstance(blank_id, int) or blank_id < 0:
        raise ValueError(f"{who}: blank_id must be a token id >= 0, got {blank_id!r}")
    return [blank_id] if config.exclude_blank else []


@torch.no_grad()
def alignment_confidence(alignment: Alignment, conf: torch.Tensor, frame_ids: torch.Tensor, blank_id: int,
                         config: ConfidenceConfig = ConfidenceConfig()) -> torch.Tensor:
    """The confidence of every target token of a ctc_forced_align result over its run [token_start, token_end): (B, Lmax)
    fp32, NaN where the alignment has no run.  conf, frame_ids: frame_confidence of the same logits.  Enqueues only."""
    _config("alignment_confidence", config)
    return span_confidence(conf, frame_ids, alignment.token_start, alignment.token_end, None, config,
                           _blank("alignment_confidence", blank_id, config))


def _word_spans(who: str, words: Sequence[Sequence[Word]], rows: int, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(starts, ends (rows, L) int64, n_spans (rows)) on the device from per-row lists of Words: one pinned copy."""
    if len(words) != rows:
        raise ValueError(f"{who}: {len(words)} lists of words for {rows} rows")
    L = max(1, max((len(w) for w in words), default=0))
    host = torch.full((2 * rows * L + rows,), -1, dtype=torch.int64)
    for b, ws in enumerate(words):
        for j, w in enumerate(ws):
            host[b * L + j] = int(w.start_frame)
            host[(rows + b) * L + j] = int(w.end_frame)
        host[2 * rows * L + b] = len(ws)
    dev = host.pin_memory().to(device, non_blocking=True)
    return dev[:rows * L].view(rows, L), dev[rows * L:2 * rows * L].view(rows, L), dev[2 * rows * L:]


@torch.no_grad()
def word_confidence(words: Sequence[Sequence[Word]], conf: torch.Tensor, frame_ids: torch.Tensor, blank_id: int,
                    lengths: Optional[torch.Tensor] = None, config: ConfidenceConfig = ConfidenceConfig()) -> List[List[float]]:
    """Per utterance the confidence of each of its align.Words (from CTCAligner, BeamCTCDecoder.words or a stream): the
    aggregation over the frames [start_frame, end_frame).  One copy of the spans to the device, one launch, one copy back:
    synchronises."""
    _, _, agg = _config("word_confidence", config)
    exclude = _blank("word_confidence", blank_id, config)
    conf, frame_ids = _req_history(conf, frame_ids)
    B, T = conf.shape
    starts, ends, n = _word_spans("word_confidence", words, B, conf.device)
    out = _spans(conf, frame_ids, _lengths(lengths, B, T, conf.device), starts, ends, n, agg, exclude).cpu().tolist()
    return [row[:len(ws)] for row, ws in zip(out, words)]


class StreamingConfidence(SlotFollower):
    """Frame confidence for `slots` independent streams (or the utterances of a lockstep batch), kept for the last `history`
    frames of each.

        sc = StreamingConfidence(S, blank_id); sc.step(logits, k); ...; sc.words(words_per_slot); sc.reset_slots([s])

    `conf` (S, history) fp32 and `ids` (S, history) int64 are rings: frame t of slot b, counted from its last reset, is at
    column t mod history; `total` (S) int64 is the number of frames the slot has taken.  step and the resets enqueue only;
    after reset_slots the slots' histories start again at frame 0 (conf NaN, ids -1, total 0)."""

    _what = "confidence only exists as gfx950 kernels"

    def __init__(self, slots: int, blank_id: int, config: ConfidenceConfig = ConfidenceConfig(), history: int = 4096,
                 device=None) -> None:
        self.method, self.alpha, self.aggregation = _config("StreamingConfidence", config)
        self.exclude = _blank("StreamingConfidence", blank_id, config)
        self.config, self.blank_id = config, blank_id
        self._init_slots("StreamingConfidence", slots, strict=False)
        if isinstance(history, bool) or not isinstance(history, int) or history < 1:
            raise ValueError(f"StreamingConfidence: history must be a number of frames >= 1, got {history!r}")
        self.R = history
        self._init_device("StreamingConfidence", device)
        self.conf = torch.full((self.S, self.R), math.nan, dtype=torch.float32, device=self.device)
        self.ids = torch.full((self.S, self.R), -1, dtype=torch.int64, device=self.device)
        self.total = torch.zeros(self.S, dtype=torch.int64, device=self.device)
        self.exclude_dev = _exclude_ids(self.exclude, self.device)
        self._armed_state = [(self.conf, math.nan), (self.ids, -1), (self.total, 0)]

    @torch.no_grad()
    def step(self, logits: torch.Tensor, k=None) -> None:
        """logits (S, k_max, V) on the device: slot b's next frames are rows 0 .. k[b]-1 (the rest is never read).  k: a device
        int64 tensor (a slot step's own), a host sequence, or None: every row of every slot.  Enqueues only."""
        x = _device_logits(logits)
        if x.dim() != 3 or x.shape[0] != self.S:
            raise ValueError(f"logits: expected ({self.S}, k_max, V), got {tuple(x.shape)}")
        _, k_max, V = x.shape
        if not 2 <= V <= V_MAX:
            raise ValueError(f"logits: V = {V} outside [2, {V_MAX}]")
        if k_max == 0:
            return
        k = self._frame_counts(k, k_max)
        for t0, n, kk in frame_chunks(k, k_max, self.R):                   # (a launch takes at most one lap of the ring)
            _frames(x[:, t0:t0 + n], kk, self.method, self.alpha, self.conf, self.ids, self.total)

    @torch.no_grad()
    def spans(self, starts: torch.Tensor, ends: torch.Tensor, n_spans: torch.Tensor) -> torch.Tensor:
        """The aggregation over the spans (S, L) int64 of absolute frames, n_spans (S) int64 of them per slot: (S, L) fp32 on
        the device, NaN for a span whose start has left the history.  Enqueues only."""
        starts, ends = ops._req(starts, "starts", torch.int64), ops._req(ends, "ends", torch.int64)
        n_spans = ops._req(n_spans, "n_spans", torch.int64)
        if starts.dim() != 2 or starts.shape[0] != self.S or ends.shape != starts.shape or n_spans.numel() != self.S:
            raise ValueError(f"starts, ends, n_spans: expected ({self.S}, L), ({self.S}, L) and ({self.S}), got "
                             f"{tuple(starts.shape)}, {tuple(ends.shape)} and {tuple(n_spans.shape)}")
        return _spans(self.conf, self.ids, self.total, starts, ends, n_spans, self.aggregation, self.exclude_dev)

    def words(self, words_per_slot: Sequence[Sequence[Word]]) -> List[List[float]]:
        """Per slot the confidence of each of its Words, whose frames count from the slot's last reset; `nan` for a word whose
        start has left the history.  One copy of the spans to the device, one launch, one copy back: synchronises."""
        starts, ends, n = _word_spans("StreamingConfidence.words", words_per_slot, self.S, self.device)
        out = self.spans(starts, ends, n).cpu().tolist()
        return [row[:len(ws)] for row, ws in zip(out, words_per_slot)]


def transcriber_confidence(who: str, confidence, confidence_history, times: bool) -> Optional[Tuple[ConfidenceConfig, int]]:
    """The transcribers' confidence options, checked on the host before anything else: None, or (config, history)."""
    if confidence is None:
        return None
    if not isinstance(confidence, ConfidenceConfig):
        raise ValueError(f"{who}: confidence must be a ConfidenceConfig, got {type(confidence).__name__}")
    confidence.check()
    if not times:
        raise ValueError(f"{who}: confidence= needs times=True (a word's confidence is taken over the frames its Word carries)")
    if isinstance(confidence_history, bool) or not isinstance(confidence_history, int) or confidence_history < 1:
        raise ValueError(f"{who}: confidence_history must be a number of frames >= 1, got {confidence_history!r}")
    return confidence, confidence_history
