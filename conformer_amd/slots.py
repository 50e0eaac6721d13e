"""Independent streams in one batch (INTEGRATION.md "Independent streams (slots)").

A streaming service holds a fixed set of batch SLOTS, each carrying one utterance of its own: a slot is opened when a call
starts, fed whatever mel frames have arrived (any count per step, 0 included), and closed when the call ends; then another
call reuses it.  Every slot keeps its own position -- K/V cache length, depthwise-convolution state, buffered mel tail, LSTM
(h, c) and beam-search state -- where StreamingEncoder / StreamingTranscriber move the whole batch in lockstep.

Per step the slots' new rows are COMPACT: slot b contributes k_b new encoder frames as rows 0 .. k_b-1 of (S, k_max, .)
tensors, so the stem, the GEMMs, LayerNorm, the feed-forward modules and the GLU run once for all slots.  Only these parts are
per slot: the cache append at row frames_b, the attention of the new rows (ops.relpos_attention_slots), the depthwise window
(GLU rows >= k_b are the zero padding of frames not received yet) with its carried state, and the mel tail.  The per-slot
counts come from the caller, so the host knows every offset; they reach the device as one small non-blocking copy per step and
nothing synchronises except partial_text() and close().

Semantics: for each slot, the sequence of frame counts it received from open to close is that utterance's own chunking, and
its results are those of a one-utterance StreamingEncoder / StreamingTranscriber fed the same chunks (to GEMM rounding: the
compact rows may tile differently).  Inference only.

Precision is fixed at construction (`dtype=`): None / torch.float32 is the fp32 object; torch.bfloat16 / torch.float16 runs every
step inside its own torch.autocast of that type, keeps the per-layer K/V caches in it (the q|k|v GEMM writes the 16-bit rows the
attention core would round to anyway: half the cache bytes, no change in arithmetic) and attends with the 16-bit slots kernel
(cfm_relpos_attention_slots_mfma16_f32).  The depthwise state, the mel tail, the LSTM state and what step() returns stay fp32.  A
stream must not change precision between chunks, so ambient autocast of another type is refused.

Bounded history (`left_context=`, `max_chunk_mel_frames=`: streaming.py): every slot's caches are rings (S, R, 3d) and the window
kernel attends; a reopened slot starts again at frame 0 over whatever its ring still holds, which the kernel never reads (rows
outside a query's window are selected away at staging).  fp32 only.
"""
from __future__ import annotations

import contextlib
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._slot_state import OpenSlots
from .align import Word
from .confidence import ConfidenceConfig, StreamingConfidence, transcriber_confidence
from .decode import BeamCTCDecoder
from .endpoint import Endpoint, EndpointConfig, StreamingEndpointer
from .model.modules.encoder import Encoder
from .stream_frontend import StreamingAudioFrontend
from .streaming import ChunkedEncoder, _refuse_window_autocast, encoder_frames
from .transcribe import decode_frames, lstm_state, search_plan, search_stream, times_plan

_TAIL = 8                  # mel-tail buffer width: a slot carries 0..6 un-consumed frames


def slot_plan(tails: Sequence[int], frames: Sequence[int]) -> Tuple[List[int], List[int]]:
    """The host bookkeeping of one step: per slot, with tails[b] buffered mel frames and frames[b] new ones, the encoder frames
    k_b that become computable and the new tail.  Encoder frame t covers mel frames 4t .. 4t+6 of the slot's stream."""
    ks, new_tails = [], []
    for t, f in zip(tails, frames):
        total = int(t) + int(f)
        k = max(0, encoder_frames(total))
        ks.append(k)
        new_tails.append(total - 4 * k)
    return ks, new_tails


def append_rows(n0: Sequence[int], ks: Sequence[int], k_max: int, t_max: Optional[int],
                ring: Optional[int] = None) -> Tuple[List[int], List[int]]:
    """The cache append of one step as flat row indices: compact row b*k_max + r of the new (S, k_max, .) rows goes to row
    n0[b] + r of slot b's linear cache (S, t_max, .), or, ring caches (S, ring, .), to row (n0[b] + r) mod ring."""
    S = len(ks)
    src = [b * k_max + r for b in range(S) for r in range(ks[b])]
    if ring is None:
        dst = [b * t_max + n0[b] + r for b in range(S) for r in range(ks[b])]
    else:
        dst = [b * ring + (n0[b] + r) % ring for b in range(S) for r in range(ks[b])]
    return src, dst


def _slot_dtype(who: str, dtype: Optional[torch.dtype]) -> Optional[torch.dtype]:
    """The `dtype=` keyword of the slot objects: None for the fp32 object, else the 16-bit type of every stream it carries."""
    if dtype is None or dtype == torch.float32:
        return None
    if dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"{who}: dtype must be None, torch.float32, torch.bfloat16 or torch.float16, got {dtype}")
    return dtype


def _refuse_autocast(who: str, dtype: Optional[torch.dtype] = None) -> None:
    """The precision of a stream was fixed when the object was made: an fp32 object refuses any ambient autocast, a 16-bit
    object the other 16-bit type."""
    if not torch.is_autocast_enabled("cuda"):
        return
    if dtype is None:
        raise RuntimeError(f"{who}: this object is fp32; leave torch.autocast before stepping (construct it with dtype= for the "
                           "16-bit slot path)")
    if torch.get_autocast_dtype("cuda") != dtype:
        raise RuntimeError(f"{who}: this object's streams are {dtype}; it cannot step under torch.autocast of "
                           f"{torch.get_autocast_dtype('cuda')}")


def _autocast(dtype: Optional[torch.dtype]):
    return contextlib.nullcontext() if dtype is None else torch.autocast("cuda", dtype=dtype)


class _Step:
    """Device views of one step's per-slot offsets (one pinned host buffer, one non-blocking copy)."""

    def __init__(self, dev: torch.device, tails, totals, n0, ks, k_max: int, t_max: int, ring: Optional[int] = None) -> None:
        S = len(ks)
        src, dst = append_rows(n0, ks, k_max, t_max, ring)
        nk = len(src)
        host = torch.empty(5 * S + 2 * nk, dtype=torch.int64, pin_memory=True)
        h = host.numpy()
        h[0:S], h[S:2 * S], h[2 * S:3 * S], h[3 * S:4 * S] = tails, totals, n0, ks
        h[4 * S:5 * S] = np.asarray(n0) + np.asarray(ks)
        h[5 * S:5 * S + nk], h[5 * S + nk:] = src, dst
        d = host.to(dev, non_blocking=True)
        self.tail, self.total, self.q_begin, self.k, self.lengths = (d[j * S:(j + 1) * S] for j in range(5))
        self.src, self.dst = d[5 * S:5 * S + nk], d[5 * S + nk:]
        self.nk, self.k_max = nk, k_max
        self.keys_hint = max(a + b for a, b in zip(n0, ks))                    # (windowed: unused, and no bound on it)
        self._keep: Dict[int, torch.Tensor] = {}
        self._mask: Optional[torch.Tensor] = None

    def mel_index(self, pos: torch.Tensor, tc: int) -> torch.Tensor:
        """Column of [tail (8) | chunk (tc) | zero] that holds position `pos` (S, P) of each slot's buffered stream."""
        tail, total = self.tail[:, None], self.total[:, None]
        zero = torch.full_like(pos, _TAIL + tc)
        return torch.where(pos < tail, pos, torch.where(pos < total, pos + (_TAIL - tail), zero))

    def glu_mask(self) -> torch.Tensor:
        """(S, k_max, 1) bool: the rows of each slot that are frames it received."""
        if self._mask is None:
            self._mask = (torch.arange(self.k_max, device=self.k.device)[None, :] < self.k[:, None])[:, :, None]
        return self._mask

    def keep_index(self, half: int) -> torch.Tensor:
        """(S, half, 1): rows k_b .. k_b+half-1 of [state ; g], the depthwise state after the step."""
        if half not in self._keep:
            self._keep[half] = (self.k[:, None] + torch.arange(half, device=self.k.device)[None, :])[:, :, None]
        return self._keep[half]


class _SlotStream:
    """The stream context of ConformerBlock.fused_chain for one slot step: slot b's new rows are the compact rows 0 .. k_b-1,
    `cur` holds the step's device offsets; `i` is the layer the chain is in (ChunkedEncoder._encode sets it)."""

    def __init__(self, st: "SlotStreamingEncoder", cur: _Step) -> None:
        self.st, self.cur, self.i = st, cur, 0
        self.qkv16 = st.dtype is not None          # the q|k|v GEMM writes the rows in the 16-bit type of the cache (for_gemm)

    def attend(self, a, qkv_new: torch.Tensor) -> torch.Tensor:
        """Append every slot's new Q|K|V rows at its own cache row and return the compact context (S, k_max, d)."""
        st, cur, i, d = self.st, self.cur, self.i, self.st.d
        if cur.nk:
            st.qkv[i].view(-1, 3 * d).index_copy_(0, cur.dst, qkv_new.reshape(-1, 3 * d).index_select(0, cur.src))
        if st.left is not None:
            return ops.relpos_attention_window(st.qkv[i], st.pos_all[:, i * d:(i + 1) * d], a.content_bias, a.position_bias,
                                               a.n_heads, cur.q_begin, cur.k, cur.k_max, st.left)
        return ops.relpos_attention_slots(st.qkv[i], st.pos_all[:, i * d:(i + 1) * d], a.content_bias, a.position_bias,
                                          st.lengths, a.n_heads, cur.q_begin, cur.k, cur.k_max, keys_hint=cur.keys_hint)

    def depthwise(self, cv, g: torch.Tensor) -> torch.Tensor:
        """Window: the slot's carried GLU rows, then its new ones (rows >= k_b: zero padding); rows k_b .. k_b+half-1 carry on."""
        state, cur = self.st.conv_state[self.i], self.cur
        half = state.shape[1]
        buf = torch.cat([state, g.masked_fill(~cur.glu_mask(), 0.0)], dim=1)
        s = cv.depthwise_eval(buf)
        state.copy_(torch.gather(buf, 1, cur.keep_index(half).expand(buf.shape[0], half, buf.shape[2])))
        return s[:, half:].contiguous()


class SlotStreamingEncoder(ChunkedEncoder, OpenSlots):
    """The chunked encoder of StreamingEncoder over `slots` independent streams of at most max_mel_frames mel frames each.
    open(s) starts a stream in a free slot, step(mel, frames) feeds every slot its own number of new frames, close(s) frees the
    slot.  Returns compact rows: step -> ((S, k_max, d), k) with slot b's new encoder frames in rows 0 .. k[b]-1.
    dtype: None / torch.float32, or torch.bfloat16 / torch.float16 -- the precision of every stream of this object (module
    docstring): 16-bit K/V caches (d % 8 == 0), every step under its own autocast.
    left_context, max_chunk_mel_frames: bounded history over ring caches as StreamingEncoder (a slot may then bring at most
    max_chunk_mel_frames mel frames per step, and max_mel_frames=None lifts the limit per stream); fp32 only."""

    def __init__(self, encoder: Encoder, slots: int, max_mel_frames: Optional[int] = None, dtype: Optional[torch.dtype] = None, *,
                 left_context: Optional[int] = None, max_chunk_mel_frames: Optional[int] = None) -> None:
        self.dtype = _slot_dtype("SlotStreamingEncoder", dtype)
        if self.dtype is not None and left_context is not None:
            raise NotImplementedError(f"SlotStreamingEncoder: left_context with dtype={self.dtype} (no 16-bit window kernel yet)")
        if self.dtype is not None and encoder.linear.out_features % 8:
            raise ValueError(f"SlotStreamingEncoder: a {self.dtype} K/V cache needs d % 8 == 0, got {encoder.linear.out_features}")
        super().__init__("SlotStreamingEncoder", encoder, slots, max_mel_frames, cache_dtype=self.dtype or torch.float32,
                         left_context=left_context, max_chunk_mel_frames=max_chunk_mel_frames)
        self.S = self.B
        self.max_mel = None if max_mel_frames is None else int(max_mel_frames)
        self._free_all()
        self.n0 = [0] * self.S                                             # encoder frames per slot so far
        self.tails = [0] * self.S                                          # buffered mel frames per slot (0..6)
        self.mel_seen = [0] * self.S                                       # mel frames received per slot
        self.last_step: Optional[_Step] = None                            # the latest step's device offsets (k: SlotTranscriber)

    def open(self, s: int) -> None:
        """Start a new stream in free slot s: K/V length, depthwise state and mel tail back to empty (enqueues only)."""
        s = self._check_slot(s, want_open=False)
        self.lengths[s:s + 1].zero_()
        for t in self.conv_state:
            t[s].zero_()
        self.n0[s] = self.tails[s] = self.mel_seen[s] = 0
        self._mark_open(s)

    def close(self, s: int) -> None:
        self._mark_closed(self._check_slot(s, want_open=True))

    def reset(self) -> None:
        """Every slot free."""
        self._free_all()

    def plan(self, mel_chunk: torch.Tensor, frames: Sequence[int]) -> Tuple[torch.Tensor, List[int], List[int]]:
        """Check a step's arguments against the slots (raises before anything is enqueued): (mel, k, new tails)."""
        if self.enc.training:
            raise RuntimeError("SlotStreamingEncoder: put the encoder in eval() mode (running BatchNorm statistics, no dropout)")
        if self.left is not None:
            _refuse_window_autocast("SlotStreamingEncoder")
        _refuse_autocast("SlotStreamingEncoder", self.dtype)
        x = ops._req(mel_chunk, "mel_chunk")
        if x.dim() != 3 or x.shape[0] != self.S:
            raise ValueError(f"mel_chunk: expected ({self.S}, n_mel, Tc), got {tuple(x.shape)}")
        frames = [int(f) for f in frames]
        if len(frames) != self.S:
            raise ValueError(f"frames: expected {self.S} counts, got {len(frames)}")
        Tc = x.shape[2]
        for b, f in enumerate(frames):
            if not 0 <= f <= Tc:
                raise ValueError(f"frames[{b}] = {f} outside [0, {Tc}]")
            if f and not self.is_open[b]:
                raise RuntimeError(f"frames given for free slot {b}: open() it first")
            if self.left is not None and f > self.max_chunk:
                raise ValueError(f"frames[{b}] = {f}: the ring was sized for max_chunk_mel_frames={self.max_chunk}")
            if self.max_mel is not None and self.mel_seen[b] + f > self.max_mel:
                raise RuntimeError(f"slot {b}: {self.mel_seen[b] + f} mel frames would pass max_mel_frames={self.max_mel}")
        ks, new_tails = slot_plan(self.tails, frames)
        return x, ks, new_tails

    @torch.no_grad()
    def step(self, mel_chunk: torch.Tensor, frames: Sequence[int]) -> Tuple[torch.Tensor, List[int]]:
        """mel_chunk (S, n_mel, Tc): slot b's next frames[b] mel frames are mel_chunk[b, :, :frames[b]] (the rest is ignored).
        Returns the compact new encoder frames (S, k_max, d) and k (host list): rows >= k[b] of slot b are padding."""
        x, ks, new_tails = self.plan(mel_chunk, frames)
        self._follow_weights()
        frames = [int(f) for f in frames]
        with _autocast(self.dtype):
            out, cur = self._step_device(x, frames, ks)
        for b in range(self.S):
            self.n0[b] += ks[b]
            self.mel_seen[b] += frames[b]
        self.tails = new_tails
        self.last_step = cur
        return out, ks

    def _step_device(self, x: torch.Tensor, frames: List[int], ks: List[int]) -> Tuple[torch.Tensor, _Step]:
        """The device work of one step (under the object's autocast, if it has one)."""
        S, Tc, dev = self.S, x.shape[2], x.device
        k_max = max(ks)
        if self.mel_tail_buf is None:
            self.mel_tail_buf = torch.zeros(S, x.shape[1], _TAIL, device=dev, dtype=torch.float32)
        totals = [t + f for t, f in zip(self.tails, frames)]
        cur = _Step(dev, self.tails, totals, self.n0, ks, k_max, self.t_max, self.ring)
        src = torch.cat([self.mel_tail_buf, x, x.new_zeros(S, x.shape[1], 1)], dim=2)   # [tail | chunk | zero column]
        n_mel = x.shape[1]
        keep = cur.k[:, None] * 4 + torch.arange(_TAIL, device=dev)[None, :]
        new_tail = torch.gather(src, 2, cur.mel_index(keep, Tc)[:, None, :].expand(S, n_mel, _TAIL))
        out = x.new_empty(S, 0, self.d)
        if k_max > 0:
            W = 4 * k_max + 3                                              # the mel frames of k_max encoder frames
            pos = torch.arange(W, device=dev)[None, :].expand(S, W)
            mel = torch.gather(src, 2, cur.mel_index(pos, Tc)[:, None, :].expand(S, n_mel, W))
            out = self._encode(mel, _SlotStream(self, cur), lambda: self.lengths.copy_(cur.lengths))
        self.mel_tail_buf.copy_(new_tail)
        return out, cur


class SlotTranscriber:
    """Independent streaming transcription in `slots` batch slots: SlotStreamingEncoder -> the decoder with per-slot LSTM state
    -> the resumable beam search of `decoder` (a BeamCTCDecoder: beam knobs, lm, hotwords) with per-slot progress.

        tr.open(s); logits, k = tr.step(mel, frames); tr.partial_text(); text = tr.close(s)

    close(s) returns what decoder(...) returns on that slot's concatenated logits.  Eval mode only; dtype: as
    SlotStreamingEncoder (the LSTM state and the logits stay fp32; the search consumes the logits the step returned).
    max_pending=M (tokens; needs left_context): every slot's search commits the prefix that can no longer change after each
    of its steps (INTEGRATION.md "Committed-prefix streaming (max_pending)"); the search buffers are sized by M and the largest
    step alone and max_mel_frames may be None.  pop_committed() hands out each open slot's final tokens as they come;
    partial_text() and close(s) then speak of the slot's text from its last pop on.
    times=True: every slot's search records token timestamps, counted from the slot's own open(s) (INTEGRATION.md "Beam-search
    timestamps"): partial_words(), close_words(s) and, with max_pending, pop_committed_words() return align.Words at
    frame_seconds per encoder frame.  A lapped commit log raises for the slot alone, as for the tokens.
    audio=StreamingAudioFrontend(frontend, slots, max_chunk_samples): step_audio(samples, counts, flush=()) takes the waveform
    instead of mel frames (INTEGRATION.md "Streaming audio front end"); open, close and reset reach the front end too.
    endpoint=EndpointConfig(...): every step also runs the endpoint rules on the logits it returns (INTEGRATION.md "Endpointing":
    one more launch, nothing synchronises); open(s) arms slot s, endpoints() reads which open slots' utterances have ended.
    Closing or segmenting an ended slot stays the caller's decision.  Without it nothing is launched or allocated.
    segment(s) / segment_words(s): the text of slot s so far, as close(s) returns it, and the slot goes on OPEN with a new search
    (and a re-armed endpointer) over the same stream: K/V caches, depthwise state, LSTM state and audio tail stay as they are.
    Every time the object reports for s (words, endpoints) still counts from open(s).
    confidence=ConfidenceConfig(...) (needs times=True): every step also keeps the frame confidence of the logits it returns,
    for each slot's last confidence_history frames counted from open(s) (INTEGRATION.md "Confidence": two more launches, nothing
    synchronises); word_confidence(words) gives the Words this object returned their confidence.  Without it nothing is
    launched or allocated.
    keywords=kws.Keywords(...): every step also runs the keyword spotter on the logits it returns, with the step's own device k
    (INTEGRATION.md "Keyword spotting": two more launches, nothing synchronises; max_detections rows per slot and group of
    keywords between two reads).  open(s) arms slot s; segment(s) does NOT arm it again, so every time counts from open(s).
    keywords() pops the open slots' new detections, close_keywords(s) ends slot s's stream of detections (close(s) itself is
    unchanged).  Without it the module is not imported and nothing is launched or allocated.
    slot_hotwords=(max_phrases, max_code_points): every slot may carry its own hotword list within those bounds (INTEGRATION.md
    "Per-request hotwords"): open(s, hotwords=..., hotword_weight=...) sets slot s's list (None: the decoder's own list and
    weight; () or []: none), segment(s) keeps it.  Without it open() refuses a list and the object is exactly as before."""

    audio: Optional[StreamingAudioFrontend] = None
    endpointer: Optional[StreamingEndpointer] = None
    confidence: Optional[StreamingConfidence] = None
    spotter = None                                 # a kws.StreamingKeywordSpotter with keywords=
    seg_start: Optional[List[int]] = None          # per slot the encoder frame at which its current segment began

    def __init__(self, model, decoder: BeamCTCDecoder, slots: int, max_mel_frames: Optional[int],
                 dtype: Optional[torch.dtype] = None, *, left_context: Optional[int] = None,
                 max_chunk_mel_frames: Optional[int] = None, max_pending: Optional[int] = None,
                 commit_log: int = 4096, times: bool = False, frame_seconds: float = 0.04,
                 audio: Optional[StreamingAudioFrontend] = None, endpoint: Optional[EndpointConfig] = None,
                 confidence: Optional[ConfidenceConfig] = None, confidence_history: int = 4096, keywords=None,
                 max_detections: int = 64, slot_hotwords: Optional[Tuple[int, int]] = None) -> None:
        tplan = times_plan("SlotTranscriber", times, frame_seconds)
        cplan = transcriber_confidence("SlotTranscriber", confidence, confidence_history, tplan[0])
        if endpoint is not None:
            if not isinstance(endpoint, EndpointConfig):
                raise ValueError(f"SlotTranscriber: endpoint must be an EndpointConfig, got {type(endpoint).__name__}")
            endpoint.check(tplan[1])
        if audio is not None and audio.S != int(slots):
            raise ValueError(f"SlotTranscriber: the audio front end has {audio.S} slots, the transcriber {int(slots)}")
        self.audio = audio
        self.dtype = _slot_dtype("SlotTranscriber", dtype)
        if self.dtype is not None and left_context is not None:
            raise NotImplementedError(f"SlotTranscriber: left_context with dtype={self.dtype} (no 16-bit window kernel yet)")
        self.commit = search_plan("SlotTranscriber", max_mel_frames, left_context, max_chunk_mel_frames, max_pending)
        self.device, self.state = lstm_state(model, "SlotTranscriber", int(slots))
        self.model = model
        self.encoder = SlotStreamingEncoder(model.encoder, slots, max_mel_frames, dtype=self.dtype, left_context=left_context,
                                            max_chunk_mel_frames=max_chunk_mel_frames)
        self.S = self.encoder.S
        self.slot_hotwords = slot_hotwords
        self.beam = search_stream(decoder, self.commit, self.S, self.encoder.t_max, self.device, commit_log, tplan, slot_hotwords)
        self.frame_seconds = tplan[1]
        self.seg_start = [0] * self.S
        if endpoint is not None:
            self.endpointer = StreamingEndpointer(self.S, decoder.blank_id, endpoint, tplan[1], self.device)
        if cplan is not None:
            self.confidence = StreamingConfidence(self.S, decoder.blank_id, cplan[0], cplan[1], self.device)
        if keywords is not None:                                           # (the module is imported by the objects that use it)
            from .kws import Keywords, StreamingKeywordSpotter
            if not isinstance(keywords, Keywords):
                raise ValueError(f"SlotTranscriber: keywords must be a kws.Keywords or None, got {type(keywords).__name__}")
            if keywords.blank_id != decoder.blank_id:
                raise ValueError(f"SlotTranscriber: the keywords' blank is {keywords.blank_id}, the decoder's {decoder.blank_id}")
            self.spotter = StreamingKeywordSpotter(self.S, keywords, tplan[1], max_detections, None, self.device)

    @property
    def is_open(self) -> List[bool]:
        return list(self.encoder.is_open)

    def _open_slots(self, read) -> dict:
        """{open slot: its entry of read(only=the open slots)}, `read` a reading method of the search."""
        open_slots = [s for s in range(self.S) if self.encoder.is_open[s]]
        out = read(only=open_slots)
        return {s: out[s] for s in open_slots}

    def open(self, s: int, hotwords=None, hotword_weight: Optional[float] = None) -> None:
        """Start an utterance in free slot s (enqueues only).  With slot_hotwords=: the slot's hotword list (None: the decoder's
        own; () or []: none; a Hotwords or phrases replace the decoder's) and weight (None: the decoder's), packed on the host
        and refused with ValueError, before anything is enqueued, over the reserved bounds.  Without slot_hotwords= a list or a
        weight raises ValueError."""
        plan = None
        if self.slot_hotwords is not None:
            plan = self.beam.plan_hotwords(hotwords, hotword_weight)
        elif hotwords is not None or hotword_weight is not None:
            raise ValueError("SlotTranscriber.open: a hotword list per slot needs slot_hotwords=(max_phrases, max_code_points) at "
                             "construction")
        self.encoder.open(s)
        if self.audio is not None:
            self._drop_audio(s)
            self.audio.open(s)
        for h, c in self.state:
            h[s].zero_()
            c[s].zero_()
        self.beam.reset_slots([s])
        if plan is not None:                                               # (the slot's search is at the empty prefix)
            self.beam.apply_hotwords(s, plan)
        self._new_segment(s, 0)
        if self.confidence is not None:                                    # (a segment does not: its words count from open(s))
            self.confidence.reset_slots([s])
        if self.spotter is not None:                                       # (nor here: detections count from open(s))
            self.spotter.reset_slots([s])

    def _new_segment(self, s: int, first_frame: int) -> None:
        """Slot s's segment begins at encoder frame first_frame of its stream: the endpointer armed again (enqueues only)."""
        if self.seg_start is not None:
            self.seg_start[s] = first_frame
        if self.endpointer is not None:
            self.endpointer.reset_slots([s])

    def _drop_audio(self, s: int) -> None:
        """The front end's slot s free (a flush has freed it already; a close without a flush drops its tail)."""
        if self.audio is not None and self.audio.is_open[s]:
            self.audio.close(s)

    def _refuse_step(self) -> None:
        if self.model.training:
            raise RuntimeError("SlotTranscriber: the model is in training mode; put it back in eval()")
        if self.encoder.left is not None:
            _refuse_window_autocast("SlotTranscriber")
        _refuse_autocast("SlotTranscriber", self.dtype)

    @torch.no_grad()
    def step_audio(self, samples: torch.Tensor, counts: Sequence[int], flush=()) -> Tuple[torch.Tensor, List[int]]:
        """step() from the waveform (needs audio=): samples (S, N) fp32 (with a front end built with input=, whatever it takes:
        INTEGRATION.md "Input sample rates"), counts: S host sample counts <= N, flush: the slots
        whose audio ends with this step (StreamingAudioFrontend.step).  Returns what step() returns for the mel frames the
        samples complete.  A flushed slot stays open here: close(s) reads its text.  Every refusal, the front end's or the
        encoder's, raises before anything is enqueued."""
        if self.audio is None:
            raise RuntimeError("SlotTranscriber: step_audio needs the audio= front end")
        self._refuse_step()
        p = self.audio.plan(samples, counts, flush)
        self.encoder.plan(p.samples.new_empty(self.S, self.audio.fe.n_mels, p.f_max), p.frames)
        mel, frames = self.audio.run(p)
        return self.step(mel, frames)

    @torch.no_grad()
    def step(self, mel_chunk: torch.Tensor, frames: Sequence[int]) -> Tuple[torch.Tensor, List[int]]:
        """mel_chunk (S, n_mel, Tc), frames: S host counts <= Tc (0 = nothing for that slot; free slots take 0).  Returns the
        logits (S, k_max, V) of the new encoder frames (slot b's in rows 0 .. k[b]-1) and k; advances each slot's search over
        its own rows.  Nothing synchronises with the host."""
        self._refuse_step()
        n0 = list(self.encoder.n0)
        enc, ks = self.encoder.step(mel_chunk, frames)
        k_max = max(ks)
        if k_max == 0:
            return enc.new_empty(self.S, 0, self.model.decoder.linear.out_features), ks
        k_dev = self.encoder.last_step.k
        with _autocast(self.dtype):
            logits = decode_frames(self.model, self.state, enc, k_dev)
        # the search's bound: the furthest slot after this step, less the chunk (each slot's own frames_b + k_b <= T_max
        # holds: the encoder refused more than max_mel_frames).  After a segment() a slot's search is BEHIND its encoder
        # position n0, so both forms below stay bounds on what the search consumed and the real limits only get looser.
        t_used = max(a + b for a, b in zip(n0, ks)) - k_max
        if self.commit:                    # after a commit a slot's tree holds at most min(max_pending, its frames) frames
            t_used = min(self.commit[0], max(n0))
        self.beam.step(logits, k_dev, t_used=t_used)
        if self.endpointer is not None:
            self.endpointer.step(logits, k_dev)
        if self.confidence is not None:
            self.confidence.step(logits, k_dev)
        if self.spotter is not None:
            self.spotter.step(logits, k_dev)
        return logits, ks

    def keywords(self) -> Dict[int, list]:
        """With keywords=: per open slot the kws.Detections emitted since the last call, sorted by (end_frame, keyword); times
        count from open(s).  A detection is emitted once a later frame has closed it, so the last one of a stream comes with
        close_keywords(s).  Synchronises, as partial_text does."""
        if self.spotter is None:
            raise RuntimeError("SlotTranscriber.keywords: the object was made without keywords=, nothing was spotted")
        return self._open_slots(self.spotter.pop)

    def close_keywords(self, s: int) -> list:
        """With keywords=: end slot s's stream of detections: what keywords() has not handed out yet together with what the
        slot still holds (StreamingKeywordSpotter.flush).  The slot itself stays as it is, open or closed: call it beside
        close(s), before the slot is opened again.  Synchronises."""
        if self.spotter is None:
            raise RuntimeError("SlotTranscriber.close_keywords: the object was made without keywords=, nothing was spotted")
        if isinstance(s, bool) or not isinstance(s, int) or not 0 <= s < self.S:
            raise ValueError(f"slot {s!r} outside [0, {self.S})")
        return self.spotter.flush(s)

    def word_confidence(self, words: Dict[int, List[Word]]) -> Dict[int, List[float]]:
        """With confidence=: the confidence of Words this object returned ({slot: its words}, as partial_words, finish_words
        and pop_committed_words give them, or {s: close_words(s)}), each over its frames [start_frame, end_frame) counted from
        open(s); nan for a word whose start has left the slot's confidence_history.  A closed slot's history stays until it
        is opened again.  Synchronises."""
        if self.confidence is None:
            raise RuntimeError("SlotTranscriber.word_confidence: the object was made without confidence=, no frame was scored")
        bad = [s for s in words if not 0 <= int(s) < self.S]
        if bad:
            raise ValueError(f"slots {bad} outside [0, {self.S})")
        out = self.confidence.words([list(words.get(s, ())) for s in range(self.S)])
        return {s: out[s] for s in words}

    def endpoints(self) -> Dict[int, Endpoint]:
        """With endpoint=: the open slots whose utterance (since open(s) or the last segment(s)) has ended, each with the rule
        that fired and when; `frame` and `seconds` count from open(s).  Synchronises, as partial_text does."""
        if self.endpointer is None:
            raise RuntimeError("SlotTranscriber.endpoints: the object was made without endpoint=, no rule was evaluated")
        out = {}
        for s, e in self._open_slots(self.endpointer.read).items():
            if e is not None:
                f = e.frame + self.seg_start[s]
                out[s] = Endpoint(e.rule, f, (f + 1) * self.frame_seconds, e.trailing_frames)
        return out

    def _shift(self, s: int, words: List[Word]) -> List[Word]:
        """Words of slot s's current segment on the clock of open(s)."""
        off = self.seg_start[s] if self.seg_start is not None else 0
        if not off:
            return words
        sec = off * self.frame_seconds
        return [Word(w.text, w.start_frame + off, w.end_frame + off, w.start + sec, w.end + sec, w.score) for w in words]

    def _shift_all(self, words: Dict[int, List[Word]]) -> Dict[int, List[Word]]:
        return {s: self._shift(s, w) for s, w in words.items()}

    def segment(self, s: int, decode_func: Optional[Callable[[str], str]] = None) -> str:
        """End slot s's utterance but not its stream: returns what close(s) would, then the slot goes on, open, with a new
        search and a re-armed endpointer; encoder caches, LSTM state and audio front end stay as they are.  With max_pending the
        text is from the last pop on, and a lapped commit log raises for s alone (the new segment begun all the same)."""
        s = self.encoder._check_slot(s, want_open=True)
        try:
            return self.beam.finish(decode_func, only=[s])[s]
        finally:
            self.beam.reset_slots([s])
            self._new_segment(s, self.encoder.n0[s])

    def segment_words(self, s: int) -> List[Word]:
        """With times: segment(s) returning the segment's transcript as Words (times counted from open(s))."""
        s = self.encoder._check_slot(s, want_open=True)
        try:
            return self._shift(s, self.beam.finish_words(only=[s])[s])
        finally:
            self.beam.reset_slots([s])
            self._new_segment(s, self.encoder.n0[s])

    def partial_text(self) -> Dict[int, str]:
        """The interim best transcript of every open slot (the one step-side call that synchronises)."""
        return self._open_slots(self.beam.partial_text)

    def pop_committed(self) -> Dict[int, List[int]]:
        """With max_pending: per open slot the token ids that became final since its previous pop, which are then forgotten
        (synchronises).  RuntimeError, with nothing popped, if a slot committed more than commit_log tokens in between."""
        return self._open_slots(self.beam.pop_committed)

    def pop_committed_words(self) -> Dict[int, List[Word]]:
        """With max_pending and times: per open slot the complete words that became final since its previous pop
        (BeamCTCStream.pop_committed_words: the tokens after the slot's last committed delimiter are held back)."""
        return self._shift_all(self._open_slots(self.beam.pop_committed_words))

    def partial_words(self) -> Dict[int, List[Word]]:
        """With times: the words of partial_text(), per open slot."""
        return self._shift_all(self._open_slots(self.beam.partial_words))

    def finish_words(self) -> Dict[int, List[Word]]:
        """With times: close_words(s) for every open slot."""
        return {s: self.close_words(s) for s in range(self.S) if self.encoder.is_open[s]}

    def close_words(self, s: int) -> List[Word]:
        """With times: close(s) returning the final transcript as Words; the slot becomes free all the same."""
        s = self.encoder._check_slot(s, want_open=True)
        try:
            return self._shift(s, self.beam.finish_words(only=[s])[s])
        finally:
            self.beam.reset_slots([s])
            self.encoder.close(s)
            self._drop_audio(s)

    def discard_committed(self, s: int) -> None:
        """With max_pending: forget slot s's committed tokens that were not popped (the way out when the slot committed more
        than commit_log tokens between pops, after which partial_text and pop_committed raise for it; close(s) also frees it)."""
        self.beam.discard_committed(only=[self.encoder._check_slot(s, want_open=True)])

    def close(self, s: int, decode_func: Optional[Callable[[str], str]] = None) -> str:
        """End slot s's utterance: its final transcript (BeamCTCDecoder on its logits); the slot becomes free.  The finish
        saves no search state, so the other slots go on; a lapped commit log raises for s alone, the slot freed all the same."""
        s = self.encoder._check_slot(s, want_open=True)
        try:
            return self.beam.finish(decode_func, only=[s])[s]
        finally:
            self.beam.reset_slots([s])
            self.encoder.close(s)
            self._drop_audio(s)

    def reset(self) -> None:
        """Every slot free (their states, the search's included, are reset when they are opened again)."""
        self.encoder.reset()
        if self.audio is not None:
            self.audio.reset()
        if self.confidence is not None:
            self.confidence.reset()
        if self.spotter is not None:
            self.spotter.reset()
