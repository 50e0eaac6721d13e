"""Endpointing: when is an utterance over?  Rule-based, on the CTC blank posterior, on the device (INTEGRATION.md
"Endpointing").

The definition is Kaldi's endpoint rules as WeNet applies them to CTC models.  A frame is SILENT when the probability of the
blank (plus any `silence_ids`, the word delimiter for instance) is at least `blank_threshold`.  Per stream three counters run
over the frames since it was armed: `frames`, `trailing` (the silent run that ends at the last frame) and `speech` (the
non-silent frames).  Rule r holds after a frame iff trailing >= min_trailing[r], frames >= min_frames[r] and speech >=
min_speech[r]; the utterance ENDS at the first frame at which any rule holds, with the lowest such rule index, and that
(rule, frame, trailing) is latched until the stream is armed again.  The counters go on counting.

Everything per frame happens in one launch per step (cfm_endpoint_step_f32, include/conformer_hip_endpoint.h) on the logits a
streaming step returned; a frame's flag depends on its V logits alone, so how a stream is cut into steps changes no integer of
the state.  `step` and `reset_slots` enqueue only; `read` is the one call that synchronises.  There is no CPU path.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib, ops
from ._slot_state import SlotFollower, frame_chunks, positive_seconds

STATE_COLS = 8             # int32 per slot: frames, trailing, speech, rule, end_frame, end_trailing, 0, 0
RULE_COLS = 4              # int32 per rule: min_trailing, min_frames, min_speech, 0
MAX_RULES, MAX_SILENCE_IDS = 4, 8      # (the blank counts as one of the 8)
K_MAX, V_MAX = 4096, 65536             # frames per slot and launch, vocabulary
_ARMED = (0, 0, 0, -1, 0, 0, 0, 0)


class EndpointRule(NamedTuple):
    """One rule, in seconds: the utterance ends once it has `min_trailing_silence` of silence at its end, is at least
    `min_utterance_length` long and holds at least `min_speech` of non-silent frames.  must_contain_speech with min_speech ==
    0 asks for one non-silent frame."""
    min_trailing_silence: float
    min_utterance_length: float = 0.0
    min_speech: float = 0.0
    must_contain_speech: bool = True

    def frames(self, frame_seconds: float) -> Tuple[int, int, int, int]:
        """The rule's row of the device table: round(seconds / frame_seconds), done once on the host."""
        for name, v in zip(self._fields[:3], self[:3]):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError(f"EndpointRule: {name} must be a finite time >= 0 in seconds, got {v!r}")
        if not isinstance(self.must_contain_speech, bool):
            raise ValueError(f"EndpointRule: must_contain_speech must be True or False, got {self.must_contain_speech!r}")
        row = [int(round(float(v) / frame_seconds)) for v in self[:3]]
        if self.must_contain_speech and row[2] == 0:
            row[2] = 1
        if max(row) >= 2 ** 31:
            raise ValueError(f"EndpointRule: {self} is {max(row)} frames of {frame_seconds} s, the counters are int32")
        return row[0], row[1], row[2], 0


# WeNet's three: 5 s of silence with nothing spoken; 1 s of silence after speech; 20 s of utterance whatever it holds
DEFAULT_RULES = (EndpointRule(5.0, 0.0, 0.0, False), EndpointRule(1.0, 0.0, 0.0, True), EndpointRule(0.0, 20.0, 0.0, False))


class EndpointConfig(NamedTuple):
    rules: Sequence[EndpointRule] = DEFAULT_RULES
    blank_threshold: float = 0.8
    silence_ids: Sequence[int] = ()        # ids counted as silence beside the blank

    def check(self, frame_seconds: float) -> List[Tuple[int, int, int, int]]:
        """Refuse a bad configuration (ValueError, on the host); the rules' table rows."""
        t = self.blank_threshold
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not 0.0 < t < 1.0:
            raise ValueError(f"EndpointConfig: blank_threshold must be a probability inside (0, 1), got {t!r}")
        rules = list(self.rules)
        if not 1 <= len(rules) <= MAX_RULES:
            raise ValueError(f"EndpointConfig: {len(rules)} rules, the kernel evaluates 1 to {MAX_RULES}")
        for r in rules:
            if not isinstance(r, EndpointRule):
                raise ValueError(f"EndpointConfig: rules holds {r!r}, expected EndpointRule")
        ids = list(self.silence_ids)
        if any(isinstance(i, bool) or not isinstance(i, int) for i in ids):
            raise ValueError(f"EndpointConfig: silence_ids must be token ids, got {ids}")
        if len(ids) > MAX_SILENCE_IDS - 1:
            raise ValueError(f"EndpointConfig: {len(ids)} silence_ids, at most {MAX_SILENCE_IDS} ids with the blank")
        return [r.frames(frame_seconds) for r in rules]


class Endpoint(NamedTuple):
    """An utterance's end: the index of the rule that fired, the 0-based frame at which it did, `seconds` = (frame + 1) *
    frame_seconds (the end of that frame) and the silent run that ended there."""
    rule: int
    frame: int
    seconds: float
    trailing_frames: int


def silence_ids(blank_id: int, config: EndpointConfig, vocab: Optional[int] = None) -> List[int]:
    """[blank, then config.silence_ids without repeats]; with `vocab` every id is checked against [0, V)."""
    if isinstance(blank_id, bool) or not isinstance(blank_id, int) or blank_id < 0:
        raise ValueError(f"blank_id must be a token id >= 0, got {blank_id!r}")
    ids = [blank_id]
    for i in config.silence_ids:
        if i not in ids:
            ids.append(int(i))
    bad = [i for i in ids if i < 0 or (vocab is not None and i >= vocab)]
    if bad:
        raise ValueError(f"silence ids {bad} outside [0, {'V' if vocab is None else vocab})")
    return ids


def endpoint_of(row: Sequence[int], frame_seconds: float) -> Optional[Endpoint]:
    """A slot's row of the state as an Endpoint, None while no rule has fired."""
    if row[3] < 0:
        return None
    return Endpoint(int(row[3]), int(row[4]), (int(row[4]) + 1) * frame_seconds, int(row[5]))


class StreamingEndpointer(SlotFollower):
    """Endpoint detection for `slots` independent streams (or the utterances of a lockstep batch).

        ep = StreamingEndpointer(S, blank_id); ep.step(logits, k); ...; ep.read(); ep.reset_slots([s])

    Every slot starts armed.  `state` is the (S, 8) int32 device tensor {frames, trailing, speech, rule, end_frame,
    end_trailing, 0, 0}.  reset_slots arms the slots again: counters 0, nothing latched."""

    _what = "endpointing only exists as a gfx950 kernel"

    def __init__(self, slots: int, blank_id: int, config: EndpointConfig = EndpointConfig(), frame_seconds: float = 0.04,
                 device=None) -> None:
        self.frame_seconds = positive_seconds("StreamingEndpointer", "frame_seconds", frame_seconds)
        if not isinstance(config, EndpointConfig):
            raise ValueError(f"StreamingEndpointer: config must be an EndpointConfig, got {type(config).__name__}")
        self.rule_rows = config.check(self.frame_seconds)
        self.ids = silence_ids(blank_id, config)
        self._init_slots("StreamingEndpointer", slots, strict=False)
        self.config = config
        self.log_threshold = math.log(float(config.blank_threshold))
        self._init_device("StreamingEndpointer", device)
        self.rules = torch.tensor(self.rule_rows, dtype=torch.int32).to(self.device)
        self.ids_dev = torch.tensor(self.ids, dtype=torch.int32).to(self.device)
        self._armed = torch.tensor([_ARMED], dtype=torch.int32).to(self.device)
        self.state = self._armed.repeat(self.S, 1)
        self._armed_state = [(self.state, self._armed)]

    @torch.no_grad()
    def step(self, logits: torch.Tensor, k=None) -> None:
        """logits (S, k_max, V) fp32 on the device: slot b's next frames are rows 0 .. k[b]-1 (the rest is never read).  k: a
        device int64 tensor (a slot step's own), a host sequence, or None: every row of every slot.  Enqueues only."""
        logits = self._device_input(logits, "logits")
        if logits.dim() != 3 or logits.shape[0] != self.S:
            raise ValueError(f"logits: expected ({self.S}, k_max, V), got {tuple(logits.shape)}")
        _, k_max, V = logits.shape
        if not 2 <= V <= V_MAX:
            raise ValueError(f"logits: V = {V} outside [2, {V_MAX}]")
        silence_ids(self.ids[0], self.config, V)
        if k_max == 0:
            return
        k = self._frame_counts(k, k_max)
        for t0, n, kk in frame_chunks(k, k_max, K_MAX):                    # (a launch takes 4096 frames per slot)
            x, ld_slot, ld_row = self._pitches(logits[:, t0:t0 + n], n, V)
            _lib.call("cfm_endpoint_step_f32", x.data_ptr(), ld_slot, ld_row, kk.data_ptr(), n, V,
                      self.ids_dev.data_ptr(), len(self.ids), self.log_threshold, self.rules.data_ptr(), len(self.rule_rows),
                      self.state.data_ptr(), self.S, ops._stream())

    def read(self, only: Optional[Sequence[int]] = None) -> List[Optional[Endpoint]]:
        """Per slot its Endpoint, or None while its utterance goes on (and for the slots not in `only`).  The one call that
        synchronises: one copy of the state."""
        rows = self.state.cpu().tolist()
        want = range(self.S) if only is None else [int(s) for s in only]
        out: List[Optional[Endpoint]] = [None] * self.S
        for s in want:
            out[s] = endpoint_of(rows[s], self.frame_seconds)
        return out


@torch.no_grad()
def ctc_endpoints(logits: torch.Tensor, blank_id: int, lengths: Optional[torch.Tensor] = None,
                  config: EndpointConfig = EndpointConfig(), frame_seconds: float = 0.04) -> Tuple[torch.Tensor, torch.Tensor]:
    """The offline form: logits (B, T, V) fp32 on the device, `lengths` (B) int64 frames per utterance (None: all T).  Returns
    (end_frame (B) int64, -1 where no rule fired; rule (B) int64, -1 likewise) as device tensors; nothing synchronises."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 3 or logits.shape[0] < 1:
        raise ValueError(f"logits: expected (B, T, V), got {tuple(getattr(logits, 'shape', ()))}")
    ep = StreamingEndpointer(logits.shape[0], blank_id, config, frame_seconds,
                             logits.device if logits.is_cuda else None)
    ep.step(logits, lengths)
    rule = ep.state[:, 3].to(torch.int64)
    return torch.where(rule >= 0, ep.state[:, 4].to(torch.int64), rule), rule
