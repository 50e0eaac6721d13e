"""Keyword spotting (spoken-term detection): where, if anywhere, was this phrase said?  On the fp32 logits of the acoustic
model, on the device (INTEGRATION.md "Keyword spotting").

The definition (conformer_amd/csrc/conformer_hip3_kws.h states the arithmetic).  A keyword of L tokens is a chain of 2 L - 1
states, token, blank, token, ..., with no blank in front or behind.  Per frame t of a stream, counted from when it was armed, a
state's score is the logit of its label less the largest logit of the frame: the log-likelihood ratio against the best symbol,
<= 0 and exactly 0 where the label is the argmax (a frame whose maximum is not finite is a BREAK: every score -inf).  A Viterbi
pass with a FREE START runs over the chain: state 0 may begin anew at any frame with score 0, every state keeps the start of
its best path, and the score of the last state at frame t is the score of the best occurrence that ends at t.  It qualifies
when it is at least the keyword's threshold, -(threshold * L); overlapping qualifying hypotheses are reduced to the best one
(the later one on a tie) and a detection is emitted once a qualifying hypothesis starts behind it or a frame does not qualify.

Two launches per step (cfm3_kws_rowmax_f32, cfm3_kws_scan_f32).  The carried state is (a, start) per state and one held
detection per keyword; how a stream is cut into steps changes no bit of it.  `step`, `reset_slots` and `reset` enqueue only;
`pop` and `flush` synchronise.  There is no CPU path.

Not measured: miss and false-alarm rates, and therefore any recommendation for `threshold`.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops
from ._slot_state import SlotFollower, positive_seconds

_C = _lib.OPEN_CONSTANTS["conformer_hip3_kws.h"]
STATE_ROWS = _C["CFM3_KWS_STATE_ROWS"]         # words per lane: a, start, held, held_start, held_end, held_score, frames, 0
GROUP_LANES = _C["CFM3_KWS_GROUP_LANES"]       # states per group (one wave)
MAX_TOKENS = _C["CFM3_KWS_MAX_TOKENS"]         # tokens per keyword: 2 L - 1 <= 64 lanes
RING_FRAMES = _C["CFM3_KWS_RING_FRAMES"]       # frames whose gathers the scan keeps in flight
FLAG_FIRST, FLAG_SKIP, FLAG_LAST = _C["CFM3_KWS_FLAG_FIRST"], _C["CFM3_KWS_FLAG_SKIP"], _C["CFM3_KWS_FLAG_LAST"]
V_MAX = _C["CFM3_KWS_V_MAX"]
DETECTIONS_MAX = 1 << 24
_NEG_INF_BITS = -8388608                       # float32 -inf as an int32


class Detection(NamedTuple):
    """One occurrence: keyword (its index in the Keywords), phrase, start and end in seconds (align.Word's convention: start =
    start_frame * frame_seconds, end = end_frame * frame_seconds with end_frame exclusive), score (the sum over its frames of
    logit[label] - max logit, <= 0 and 0.0 for an occurrence that is the argmax on every frame), and the frames themselves."""
    keyword: int
    phrase: str
    start: float
    end: float
    score: float
    start_frame: int
    end_frame: int                 # exclusive


def _threshold(who: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
        raise ValueError(f"{who}: a threshold must be a finite number of nats per token >= 0, got {v!r}")
    return float(v)


class Keywords:
    """The phrases to spot, normalised and packed for the kernels.

        kws = Keywords(["open the door", "stop"], CTCAligner.from_decoder(decoder), threshold=1.5)

    phrases: strs, tokenised by `tokenizer` (a CTCAligner, or anything with .tokenize, .blank_id and .vocab), or token-id
    sequences (then `blank_id` and `vocab_size` may stand in for the tokenizer).  threshold: nats per token, >= 0, and it has NO
    default: the useful value depends on a trained model's posteriors and no labelled audio was at hand; a keyword of L tokens
    qualifies at a score >= float32(-(threshold * L)).  thresholds: one per phrase, instead of `threshold`.
    Refused (ValueError): no phrase, an empty phrase, a phrase given twice (as token ids), the blank or an id outside the
    vocabulary, more than 32 tokens, a threshold that is not finite or negative.
    Packing: a group is 64 lanes, a lane is a state, a keyword's 2 L - 1 states are consecutive lanes of one group.  The
    keywords fill the groups in the order given; a keyword that does not fit the lanes left opens the next group.
    `lanes` (G, 3, 64) int32 {label (-1: idle), keyword (-1: idle), flags}, `thresholds` (K) float32, `packing` [(keyword, group,
    first lane)], `tokens` the id lists, `phrases` their spelling."""

    def __init__(self, phrases: Sequence, tokenizer=None, *, threshold: Optional[float] = None,
                 thresholds: Optional[Sequence[float]] = None, blank_id: Optional[int] = None,
                 vocab_size: Optional[int] = None) -> None:
        if tokenizer is not None:
            if blank_id is not None or vocab_size is not None:
                raise ValueError("Keywords: blank_id and vocab_size come from the tokenizer")
            blank_id, vocab_size = tokenizer.blank_id, len(tokenizer.vocab)
        for name, v in (("blank_id", blank_id), ("vocab_size", vocab_size)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"Keywords: without a tokenizer {name} must be given as an int, got {v!r}")
        if not 2 <= vocab_size <= V_MAX or not 0 <= blank_id < vocab_size:
            raise ValueError(f"Keywords: blank_id {blank_id} and a vocabulary of {vocab_size} (2 to {V_MAX}) do not go together")
        if isinstance(phrases, str) or len(phrases) == 0:
            raise ValueError(f"Keywords: phrases must be a non-empty sequence of phrases, got {phrases!r}")
        if thresholds is None:
            if threshold is None:
                raise TypeError("Keywords: threshold (nats per token) has no default: give threshold= or thresholds=")
            per = [_threshold("Keywords", threshold)] * len(phrases)
        else:
            if threshold is not None:
                raise ValueError("Keywords: give threshold or thresholds, not both")
            if len(thresholds) != len(phrases):
                raise ValueError(f"Keywords: {len(thresholds)} thresholds for {len(phrases)} phrases")
            per = [_threshold("Keywords", v) for v in thresholds]
        self.blank_id, self.vocab_size = int(blank_id), int(vocab_size)
        self.tokens: List[List[int]] = []
        self.phrases: List[str] = []
        for q, p in enumerate(phrases):
            if isinstance(p, str):
                if tokenizer is None:
                    raise ValueError(f"Keywords: phrase {q} is a str and there is no tokenizer")
                ids = [int(i) for i in tokenizer.tokenize(p)]
                text = p
            else:
                if isinstance(p, torch.Tensor):
                    p = p.tolist()
                if any(isinstance(i, bool) or not isinstance(i, (int, np.integer)) for i in p):
                    raise ValueError(f"Keywords: phrase {q} holds something that is no token id: {list(p)!r}")
                ids = [int(i) for i in p]
                vocab = getattr(tokenizer, "vocab", None)
                text = "".join(vocab[i] for i in ids if 0 <= i < len(vocab)) if vocab is not None else " ".join(map(str, ids))
            if not ids:
                raise ValueError(f"Keywords: phrase {q} ({p!r}) is empty")
            bad = [i for i in ids if not 0 <= i < self.vocab_size or i == self.blank_id]
            if bad:
                raise ValueError(f"Keywords: phrase {q} ({p!r}) holds the ids {bad}: outside [0, {self.vocab_size}) or the blank "
                                 f"{self.blank_id}")
            if len(ids) > MAX_TOKENS:
                raise ValueError(f"Keywords: phrase {q} ({p!r}) has {len(ids)} tokens, a keyword takes at most {MAX_TOKENS}")
            if ids in self.tokens:
                raise ValueError(f"Keywords: phrase {q} ({p!r}) is phrase {self.tokens.index(ids)} again")
            self.tokens.append(ids)
            self.phrases.append(text)
        self.per_token = per
        self.thresholds = np.array([np.float32(-(t * len(ids))) for t, ids in zip(per, self.tokens)], dtype=np.float32)
        self.packing: List[tuple] = []
        g, at = 0, 0
        for q, ids in enumerate(self.tokens):
            n = 2 * len(ids) - 1
            if at + n > GROUP_LANES:
                g, at = g + 1, 0
            self.packing.append((q, g, at))
            at += n
        self.G = g + 1
        self.lanes = np.zeros((self.G, 3, GROUP_LANES), dtype=np.int32)
        self.lanes[:, :2] = -1
        for (q, g, at), ids in zip(self.packing, self.tokens):
            for i in range(2 * len(ids) - 1):
                flags = (FLAG_FIRST if i == 0 else 0) | (FLAG_LAST if i == 2 * len(ids) - 2 else 0)
                if i >= 2 and i % 2 == 0 and ids[i // 2] != ids[i // 2 - 1]:
                    flags |= FLAG_SKIP
                self.lanes[g, :, at + i] = (ids[i // 2] if i % 2 == 0 else self.blank_id, q, flags)

    def __len__(self) -> int:
        return len(self.tokens)


def suppress_overlaps(detections: Sequence[Detection]) -> List[Detection]:
    """Per keyword, of any detections whose frame ranges [start_frame, end_frame) overlap only the best-scoring one is kept
    (greedy, best first; the earlier one on a tie).  Detections of different keywords never suppress each other.  The result
    is sorted by (end_frame, keyword).  Host arithmetic; nothing applies it by default."""
    kept: List[Detection] = []
    for d in sorted(detections, key=lambda d: (-d.score, d.end_frame, d.start_frame)):
        if not any(k.keyword == d.keyword and d.start_frame < k.end_frame and k.start_frame < d.end_frame for k in kept):
            kept.append(d)
    return sorted(kept, key=lambda d: (d.end_frame, d.keyword))


class StreamingKeywordSpotter(SlotFollower):
    """Keyword spotting for `slots` independent streams.

        sp = StreamingKeywordSpotter(S, keywords); sp.step(logits, k); ...; sp.pop(); sp.flush(s)

    It takes what SlotTranscriber.step returns (or any (S, k_max, V) fp32 logits).  Every slot starts armed.  Device tensors:
    `state` (S, G, 8, 64) int32 words per lane {a, start, held, held_start, held_end, held_score, frames (lane 0), 0},
    `detections` (S, G, max_detections, 4) int32 {keyword, start, end, score bits}, `counts` (S, G) int32 and, of the last
    step, `rowmax` (S, k_max) fp32 (columns at or beyond a slot's frames are not written).  max_chunk_frames: allocate the
    row-maximum workspace up front (steps of up to that many frames then allocate nothing); otherwise it is made once per
    k_max.  `lost[s]`: the detections of slot s that did not fit max_detections between two pops, so far.
    reset_slots arms the slots again: frame 0, every state at -inf, nothing held, no detection waiting (what was not popped is
    dropped)."""

    _what = "keyword spotting only exists as gfx950 kernels"

    def __init__(self, slots: int, keywords: Keywords, frame_seconds: float = 0.04, max_detections: int = 64,
                 max_chunk_frames: Optional[int] = None, device=None) -> None:
        if not isinstance(keywords, Keywords):
            raise ValueError(f"StreamingKeywordSpotter: keywords must be a Keywords, got {type(keywords).__name__}")
        self.frame_seconds = positive_seconds("StreamingKeywordSpotter", "frame_seconds", frame_seconds)
        self._init_slots("StreamingKeywordSpotter", slots, strict=True, max_slots=65535)
        if isinstance(max_detections, bool) or not isinstance(max_detections, int) or not 1 <= max_detections <= DETECTIONS_MAX:
            raise ValueError(f"StreamingKeywordSpotter: max_detections must be 1 to {DETECTIONS_MAX}, got {max_detections!r}")
        if max_chunk_frames is not None and (isinstance(max_chunk_frames, bool) or not isinstance(max_chunk_frames, int)
                                             or max_chunk_frames < 1):
            raise ValueError(f"StreamingKeywordSpotter: max_chunk_frames must be a number of frames >= 1, got {max_chunk_frames!r}")
        self.keywords, self.G, self.max_detections = keywords, keywords.G, max_detections
        self._init_device("StreamingKeywordSpotter", device)
        self.lanes = torch.from_numpy(keywords.lanes).to(self.device)
        self.thresholds = torch.from_numpy(keywords.thresholds).to(self.device)
        armed = torch.zeros(1, self.G, STATE_ROWS, GROUP_LANES, dtype=torch.int32)
        armed[:, :, 0] = _NEG_INF_BITS
        self._armed = armed.to(self.device)
        self.state = self._armed.repeat(self.S, 1, 1, 1)
        self.detections = torch.zeros(self.S, self.G, max_detections, 4, dtype=torch.int32, device=self.device)
        self.counts = torch.zeros(self.S, self.G, dtype=torch.int32, device=self.device)
        self.rowmax = torch.zeros(self.S, 0, dtype=torch.float32, device=self.device)
        self.lost = [0] * self.S
        self._chunk = max_chunk_frames
        self._work = None if max_chunk_frames is None else torch.zeros(self.S, max_chunk_frames, dtype=torch.float32,
                                                                       device=self.device)
        self._buffers: dict = {}           # k_max -> rowmax, made once per k_max (beyond max_chunk_frames)
        self._armed_state = [(self.state, self._armed), (self.counts, 0)]

    @torch.no_grad()
    def step(self, logits: torch.Tensor, k=None) -> None:
        """logits (S, k_max, V) fp32 on the device: slot b's next frames are rows 0 .. k[b]-1 (the rest is never read).  k: a
        device int64 tensor (a slot step's own), a host sequence, or None: every row of every slot.  Enqueues only: two
        launches."""
        logits = self._device_input(logits, "logits")
        if logits.dim() != 3 or logits.shape[0] != self.S:
            raise ValueError(f"logits: expected ({self.S}, k_max, V), got {tuple(logits.shape)}")
        _, k_max, V = logits.shape
        if V != self.keywords.vocab_size:
            raise ValueError(f"logits: V = {V}, the keywords were made for a vocabulary of {self.keywords.vocab_size}")
        if k_max == 0:
            return
        k = self._frame_counts(k, k_max)
        x, ld_slot, ld_row = self._pitches(logits, k_max, V)
        if self._chunk is not None and k_max <= self._chunk:
            self.rowmax = self._work
        else:
            if k_max not in self._buffers:
                self._buffers[k_max] = torch.zeros(self.S, k_max, dtype=torch.float32, device=self.device)
            self.rowmax = self._buffers[k_max]
        ld_rowmax, stream = self.rowmax.stride(0), ops._stream()
        _lib.call("cfm3_kws_rowmax_f32", x.data_ptr(), ld_slot, ld_row, k.data_ptr(), k_max, V, self.rowmax.data_ptr(),
                  ld_rowmax, self.S, stream)
        _lib.call("cfm3_kws_scan_f32", x.data_ptr(), ld_slot, ld_row, self.rowmax.data_ptr(), ld_rowmax, k.data_ptr(), k_max, V,
                  self.lanes.data_ptr(), self.thresholds.data_ptr(), self.G, len(self.keywords), self.state.data_ptr(),
                  self.detections.data_ptr(), self.max_detections, self.counts.data_ptr(), self.S, stream)

    def _detection(self, q: int, start: int, end: int, score: float) -> Detection:
        fs = self.frame_seconds
        return Detection(q, self.keywords.phrases[q], start * fs, (end + 1) * fs, score, start, end + 1)

    def pop(self, only: Optional[Sequence[int]] = None) -> List[Optional[List[Detection]]]:
        """Per slot the detections emitted since its last pop, merged over the groups and sorted by (end_frame, keyword) (None
        for the slots not in `only`); the slots' counts are then cleared, on the stream.  The one call of a running stream that
        synchronises: a copy of the counts and of the detections.  What did not fit max_detections in a group is lost and
        counted in `lost[s]`: pop more often or raise max_detections."""
        want = self._slot_list(only)
        out: List[Optional[List[Detection]]] = [None] * self.S
        if not want:
            return out
        idx = self._slot_index(want)
        counts = self.counts.index_select(0, idx).cpu().numpy()
        rows = self.detections.index_select(0, idx).cpu().numpy()
        for i, s in enumerate(want):
            found = []
            for g in range(self.G):
                n = min(int(counts[i, g]), self.max_detections)
                self.lost[s] += int(counts[i, g]) - n
                block = rows[i, g, :n]
                scores = np.ascontiguousarray(block[:, 3]).view(np.float32)
                found += [self._detection(int(r[0]), int(r[1]), int(r[2]), float(sc)) for r, sc in zip(block, scores)]
            out[s] = sorted(found, key=lambda d: (d.end_frame, d.keyword))
        self.counts.index_fill_(0, idx, 0)
        return out

    def held(self, s: int) -> List[Detection]:
        """The detections slot s holds back: per keyword the best qualifying hypothesis that no later frame has closed yet.
        Synchronises; changes nothing."""
        (s,) = self._slot_list([s])
        words = self.state[s].cpu()
        scores = words[:, 5].contiguous().view(torch.float32)
        out = []
        for (q, g, at), ids in zip(self.keywords.packing, self.keywords.tokens):
            lane = at + 2 * len(ids) - 2
            if int(words[g, 2, lane]):
                out.append(self._detection(q, int(words[g, 3, lane]), int(words[g, 4, lane]), float(scores[g, lane])))
        return sorted(out, key=lambda d: (d.end_frame, d.keyword))

    def flush(self, s: int) -> List[Detection]:
        """End slot s's stream: pop([s]) together with what the slot still holds, sorted by (end_frame, keyword); the slot is
        then armed again.  Synchronises."""
        out = sorted(self.pop([s])[s] + self.held(s), key=lambda d: (d.end_frame, d.keyword))
        self.reset_slots([s])
        return out


@torch.no_grad()
def spot_keywords(logits: torch.Tensor, keywords: Keywords, lengths=None, frame_seconds: float = 0.04,
                  max_detections: Optional[int] = None) -> List[List[Detection]]:
    """The offline form: one fresh StreamingKeywordSpotter fed everything, then `flush`.  logits (B, T, V) or (T, V) fp32 on the
    device, `lengths` (B) frames per utterance (None: all T).  Returns per utterance its detections sorted by (end_frame,
    keyword).  max_detections: rows per utterance and group of keywords.  A keyword can emit once per frame at the most, so
    T * min(K, 64) rows cannot overflow; None takes that, capped at 4096.  RuntimeError if a group emitted more.
    Synchronises."""
    if not isinstance(logits, torch.Tensor) or logits.dim() not in (2, 3):
        raise ValueError(f"logits: expected (B, T, V) or (T, V), got {tuple(getattr(logits, 'shape', ()))}")
    if logits.dim() == 2:
        if lengths is not None:
            raise ValueError("spot_keywords: lengths goes with a (B, T, V) batch")
        return spot_keywords(logits.unsqueeze(0), keywords, None, frame_seconds, max_detections)
    if not isinstance(keywords, Keywords):
        raise ValueError(f"spot_keywords: keywords must be a Keywords, got {type(keywords).__name__}")
    B, T, _ = logits.shape
    if B < 1:
        raise ValueError(f"logits: expected (B, T, V) with B >= 1, got {tuple(logits.shape)}")
    if max_detections is None:
        max_detections = max(1, min(4096, T * min(len(keywords), GROUP_LANES)))
    sp = StreamingKeywordSpotter(B, keywords, frame_seconds, max_detections, None, logits.device if logits.is_cuda else None)
    sp.step(logits, lengths)
    out = [sp.flush(s) for s in range(B)]
    if any(sp.lost):
        raise RuntimeError(f"spot_keywords: {sp.lost} detections per utterance did not fit max_detections = {max_detections}")
    return out
