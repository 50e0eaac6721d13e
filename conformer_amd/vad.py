"""Voice activity detection: where is speech?  Rule-based, on the log-mel frames of the front ends, on the device
(INTEGRATION.md "Voice activity detection").

The definition (conformer_amd/csrc/conformer_hip3_vad.h states the arithmetic).  Per mel frame t of a stream, counted from when
it was armed: the band energy e_t = log sum_{m in band} exp(x[m, t]) (a frame whose e_t is not finite is not speech and is
stored as +inf); s_t, the mean of the stored energies of the last min(smooth, t + 1) frames; the noise floor f_t, the minimum of
s over the last min(noise_window, t + 1) frames, the current one included (trailing minimum statistics: causal); the raw flag
e_t finite and e_t - f_t >= snr and e_t >= min_energy.  A segment opens once `onset` raw frames ran in a row, at the first of
them, and closes once `hangover` frames that are not raw ran in a row, at the first of those (exclusive end).

Two launches per step (cfm3_vad_energy_f32, cfm3_vad_scan_f32).  The carried state is a few integers and a ring of
noise_window + smooth - 1 energies per slot; how a stream is cut into steps changes no bit of any energy, flag, state word or
segment.  `step`, `reset_slots` and `reset` enqueue only; `read` and `finish` synchronise.  There is no CPU path.

Known limits, properties of causal minimum statistics: a stream that starts in the middle of speech has no floor until the
first dip in energy, so its first onset is late; and speech that goes on for longer than noise_window without a pause lifts the
floor to the level of the speech.  There is no look-ahead and no centred window.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib, ops
from ._slot_state import SlotFollower, frame_chunks, positive_seconds

_C = _lib.OPEN_CONSTANTS["conformer_hip3_vad.h"]
STATE_COLS = _C["CFM3_VAD_STATE_COLS"]         # int32 per slot: frames, run_speech, run_silence, in_speech, start, count, 0, 0
SCAN_FRAMES = _C["CFM3_VAD_SCAN_FRAMES"]       # frames per slot and scan launch
SMOOTH_MAX, WINDOW_MAX, BAND_MAX = _C["CFM3_VAD_SMOOTH_MAX"], _C["CFM3_VAD_WINDOW_MAX"], _C["CFM3_VAD_BAND_MAX"]
COUNT_MAX = 1 << 24                            # onset, hangover, max_segments

Segment = Tuple[int, int]                      # (start, exclusive end) in mel frames


def _seconds(who: str, name: str, v, least: float = 0.0) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < least:
        raise ValueError(f"{who}: {name} must be a finite time >= {least} in seconds, got {v!r}")
    return float(v)


class VadFrames(NamedTuple):
    """A VadConfig in the units of the kernels: mel bins, mel frames and nats."""
    m_lo: int
    m_hi: int
    smooth: int
    noise_window: int
    snr: float
    min_energy: float
    onset: int
    hangover: int
    pad_before: int
    pad_after: int
    min_gap: int


class VadConfig(NamedTuple):
    """snr_db: how far above the noise floor a frame's band energy has to lie to count as speech, in dB of power (snr =
    snr_db ln10 / 10 nats).  It has NO default: the useful value depends on the recordings and no labelled audio was at hand.
    band = (lo, hi): the mel bins [lo, hi) the energy is taken over, None: all.  noise_window, smooth, onset, hangover: seconds
    (the definition in the module docstring); each is converted once, with round(seconds / mel_seconds), and has to come to
    1 .. 512, 1 .. 16, >= 1 and >= 1 frames.  min_energy: an absolute floor in nats below which nothing is speech.
    pad_before, pad_after, min_gap: seconds, the island shaping of speech_islands (long-form transcription).
    The defaults are common practice; none of them was measured here."""
    snr_db: float
    band: Optional[Tuple[int, int]] = None
    noise_window: float = 3.0
    smooth: float = 0.05
    onset: float = 0.05
    hangover: float = 0.3
    min_energy: float = -math.inf
    pad_before: float = 0.2
    pad_after: float = 0.2
    min_gap: float = 0.5

    def check(self, mel_seconds: float, n_mel: int) -> VadFrames:
        """Refuse a bad configuration (ValueError, on the host); the configuration in frames."""
        mel_seconds = positive_seconds("VadConfig", "mel_seconds", mel_seconds)
        if isinstance(n_mel, bool) or not isinstance(n_mel, int) or n_mel < 1:
            raise ValueError(f"VadConfig: n_mel must be a number of mel bins >= 1, got {n_mel!r}")
        v = self.snr_db
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"VadConfig: snr_db must be a finite number of decibels, got {v!r}")
        if self.band is None:
            lo, hi = 0, n_mel
        else:
            band = tuple(self.band) if isinstance(self.band, (tuple, list)) else ()
            if len(band) != 2 or any(isinstance(i, bool) or not isinstance(i, int) for i in band):
                raise ValueError(f"VadConfig: band must be (lo, hi) in mel bins or None, got {self.band!r}")
            lo, hi = band
            if not 0 <= lo < hi <= n_mel:
                raise ValueError(f"VadConfig: band = [{lo}, {hi}) is no range of the {n_mel} mel bins")
        if hi - lo > BAND_MAX:
            raise ValueError(f"VadConfig: a band of {hi - lo} mel bins, the kernel sums at most {BAND_MAX}")
        m = self.min_energy
        if isinstance(m, bool) or not isinstance(m, (int, float)) or math.isnan(m) or m == math.inf:
            raise ValueError(f"VadConfig: min_energy must be a number of nats or -inf, got {m!r}")
        frames = {}
        for name in ("noise_window", "smooth", "onset", "hangover", "pad_before", "pad_after", "min_gap"):
            frames[name] = int(round(_seconds("VadConfig", name, getattr(self, name)) / mel_seconds))
        for name, most in (("noise_window", WINDOW_MAX), ("smooth", SMOOTH_MAX), ("onset", COUNT_MAX), ("hangover", COUNT_MAX)):
            if not 1 <= frames[name] <= most:
                raise ValueError(f"VadConfig: {name} = {getattr(self, name)} s is {frames[name]} frames of {mel_seconds} s, "
                                 f"the kernel takes 1 to {most}")
        if max(frames.values()) >= 2 ** 31:
            raise ValueError(f"VadConfig: {self} holds a time of {max(frames.values())} frames, the counters are int32")
        return VadFrames(lo, hi, frames["smooth"], frames["noise_window"], float(v) * math.log(10.0) / 10.0, float(m),
                         frames["onset"], frames["hangover"], frames["pad_before"], frames["pad_after"], frames["min_gap"])


def segment_bound(frames: int, onset: int, hangover: int) -> int:
    """The most segments that can close in `frames` frames: each needs `onset` raw frames and `hangover` others."""
    return frames // (onset + hangover) + 1


def speech_islands(segments: Sequence[Segment], n_mel_frames: int, pad_before: int, pad_after: int,
                   min_gap: int) -> List[Segment]:
    """The stretches of a recording of n_mel_frames mel frames that are worth encoding, from its speech segments (sorted,
    disjoint, in frames).  Host arithmetic, all in frames:
    1. every segment is widened by pad_before and pad_after and clamped to [0, n_mel_frames);
    2. its start is rounded DOWN to a multiple of 4, so the island's encoder frame j is the recording's frame start / 4 + j
       (the grid longform.window_plan relies on);
    3. islands that overlap, or whose gap is shorter than min_gap, are merged;
    4. an island shorter than 7 frames (longform.MIN_MEL_FRAMES) is extended at its end, then, at the end of the recording,
       at its start in steps of 4 (a recording shorter than 7 frames keeps what fits); the merge of 3 is then repeated.
    A recording without speech has no island."""
    for name, v in (("n_mel_frames", n_mel_frames), ("pad_before", pad_before), ("pad_after", pad_after), ("min_gap", min_gap)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"speech_islands: {name} must be a number of frames >= 0, got {v!r}")
    from .longform import MIN_MEL_FRAMES           # (here: longform imports this module only when a Transcriber uses it)
    n = n_mel_frames

    def merged(spans: List[List[int]]) -> List[List[int]]:
        out: List[List[int]] = []
        for a, b in spans:
            if out and (a <= out[-1][1] or a - out[-1][1] < min_gap):
                out[-1][1] = max(out[-1][1], b)
            else:
                out.append([a, b])
        return out

    spans = []
    for a, b in segments:
        a, b = int(a), int(b)
        if not 0 <= a < b:
            raise ValueError(f"speech_islands: ({a}, {b}) is no segment")
        a, b = max(0, a - pad_before), min(n, b + pad_after)
        if a < b:
            spans.append([a // 4 * 4, b])
    spans.sort()
    spans = merged(spans)
    for s in spans:
        if s[1] - s[0] < MIN_MEL_FRAMES:
            s[1] = min(n, s[0] + MIN_MEL_FRAMES)
            while s[1] - s[0] < MIN_MEL_FRAMES and s[0] >= 4:
                s[0] -= 4
    return [(a, b) for a, b in merged(sorted(spans))]


class VadRead(NamedTuple):
    """What `read` knows of a slot: whether it is in speech after the last frame, the segments that closed since the last read
    as (start, end) in mel frames since the slot was armed (end exclusive), and the same in seconds."""
    in_speech: bool
    segments: List[Segment]
    seconds: List[Tuple[float, float]]


class StreamingVad(SlotFollower):
    """Voice activity detection for `slots` independent streams.

        vad = StreamingVad(S, 80, VadConfig(snr_db=9.0)); vad.step(mel, frames); ...; vad.read(); vad.finish([s])

    It takes what StreamingAudioFrontend.step returns and runs beside a SlotTranscriber on the same chunks; what to do with the
    answer is the caller's.  Every slot starts armed.  Device tensors: `state` (S, 8) int32 {frames, run_speech, run_silence,
    in_speech, start, count, 0, 0}, `ring` (S, noise_window + smooth - 1) fp32, `segments` (S, max_segments, 2) int32, and of
    the last step `energy` (S, k_max) fp32 and `flags` (S, k_max) uint8 (columns at or beyond a slot's frames are not written).
    reset_slots arms the slots again: frame 0, no floor, not in speech, no segments."""

    _what = "voice activity detection only exists as gfx950 kernels"

    def __init__(self, slots: int, n_mel: int, config: VadConfig, mel_seconds: float = 0.01, max_segments: int = 64,
                 device=None) -> None:
        if not isinstance(config, VadConfig):
            raise ValueError(f"StreamingVad: config must be a VadConfig, got {type(config).__name__}")
        self.mel_seconds = positive_seconds("StreamingVad", "mel_seconds", mel_seconds)
        self.p = config.check(self.mel_seconds, n_mel)
        self.config, self.n_mel = config, n_mel
        self._init_slots("StreamingVad", slots, strict=True, max_slots=65535)
        if isinstance(max_segments, bool) or not isinstance(max_segments, int) or not 1 <= max_segments <= COUNT_MAX:
            raise ValueError(f"StreamingVad: max_segments must be 1 to {COUNT_MAX}, got {max_segments!r}")
        self.max_segments = max_segments
        self._init_device("StreamingVad", device)
        self.state = torch.zeros(self.S, STATE_COLS, dtype=torch.int32, device=self.device)
        self._armed_state = [(self.state, 0)]
        self.ring = torch.zeros(self.S, self.p.noise_window + self.p.smooth - 1, dtype=torch.float32, device=self.device)
        self.segments = torch.zeros(self.S, max_segments, 2, dtype=torch.int32, device=self.device)
        self.energy = torch.zeros(self.S, 0, dtype=torch.float32, device=self.device)
        self.flags = torch.zeros(self.S, 0, dtype=torch.uint8, device=self.device)
        self._buffers: dict = {}           # k_max -> (energy, flags), made once per k_max

    @torch.no_grad()
    def step(self, mel_chunk: torch.Tensor, frames) -> None:
        """mel_chunk (S, n_mel, k_max) fp32 log-mel on the device: slot b's next frames are the columns 0 .. frames[b]-1 (the
        rest is never read).  frames: a device int64 tensor or a host sequence.  Enqueues only: one energy launch, and one scan
        launch per 4096 columns."""
        mel_chunk = self._device_input(mel_chunk, "mel_chunk")
        if mel_chunk.dim() != 3 or mel_chunk.shape[0] != self.S or mel_chunk.shape[1] != self.n_mel:
            raise ValueError(f"mel_chunk: expected ({self.S}, {self.n_mel}, k_max), got {tuple(mel_chunk.shape)}")
        k_max = mel_chunk.shape[2]
        if k_max == 0:
            return
        k = self._frame_counts(frames, k_max, name="frames", allow_all=False)
        x, ld_slot, ld_mel = self._pitches(mel_chunk, self.n_mel, k_max)
        if k_max not in self._buffers:
            self._buffers[k_max] = (torch.zeros(self.S, k_max, dtype=torch.float32, device=self.device),
                                    torch.zeros(self.S, k_max, dtype=torch.uint8, device=self.device))
        self.energy, self.flags = self._buffers[k_max]
        p, stream = self.p, ops._stream()
        _lib.call("cfm3_vad_energy_f32", x.data_ptr(), ld_slot, ld_mel, k.data_ptr(), k_max, self.n_mel, p.m_lo, p.m_hi,
                  self.energy.data_ptr(), k_max, self.S, stream)
        for t0, n, kk in frame_chunks(k, k_max, SCAN_FRAMES):              # (a scan launch takes 4096 frames per slot)
            _lib.call("cfm3_vad_scan_f32", self.energy.data_ptr() + 4 * t0, k_max, kk.data_ptr(), n, p.smooth, p.noise_window,
                      p.snr, p.min_energy, p.onset, p.hangover, self.state.data_ptr(), self.ring.data_ptr(),
                      self.flags.data_ptr() + t0, k_max, self.segments.data_ptr(), self.max_segments, self.S, stream)

    def read(self, only: Optional[Sequence[int]] = None) -> List[Optional[VadRead]]:
        """Per slot a VadRead (None for the slots not in `only`): whether it is in speech, and the segments that closed since
        the last read; the slot's segment count is then cleared.  The one call that synchronises: a copy of the state and of
        the segments.  RuntimeError when more than max_segments closed in a slot since its last read (nothing was written
        beyond the buffer; the later ones are lost): read more often or raise max_segments."""
        want = self._slot_list(only)
        rows, segs = self.state.cpu().tolist(), self.segments.cpu().tolist()
        out: List[Optional[VadRead]] = [None] * self.S
        over = [(s, rows[s][5]) for s in want if rows[s][5] > self.max_segments]
        for s in want:
            closed = [(a, b) for a, b in segs[s][:min(rows[s][5], self.max_segments)]]
            out[s] = VadRead(bool(rows[s][3]), closed, [(a * self.mel_seconds, b * self.mel_seconds) for a, b in closed])
        if want:
            self.state[:, 5].index_fill_(0, self._slot_index(want), 0)
        if over:
            raise RuntimeError(f"StreamingVad.read: (slot, segments closed since its last read) {over} beyond max_segments = "
                               f"{self.max_segments}; the later segments are lost: call read more often or raise max_segments")
        return out

    def finish(self, slots: Optional[Sequence[int]] = None) -> List[Optional[VadRead]]:
        """End the streams of `slots` (None: all): `read` them, close a segment that is still open at frames - run_silence
        (the last raw frame + 1), and arm the slots again.  Synchronises."""
        want = self._slot_list(slots)
        rows = self.state.cpu().tolist()
        out = self.read(want)
        for s in want:
            frames, _, run_silence, in_speech, start = rows[s][:5]
            if in_speech:
                a, b = start, frames - run_silence
                out[s] = VadRead(False, out[s].segments + [(a, b)],
                                 out[s].seconds + [(a * self.mel_seconds, b * self.mel_seconds)])
        self.reset_slots(want)
        return out


@torch.no_grad()
def speech_segments(mels, lengths=None, *, config: VadConfig, mel_seconds: float = 0.01) -> List[List[Segment]]:
    """The offline form: one fresh StreamingVad fed everything, then `finish`.  mels: (B, n_mel, T) fp32 log-mel on the device
    with `lengths` (B) frames per recording (None: all T), or a sequence of recordings (n_mel, n_i), each then a stream of its
    own (no padded copy is made).  Returns per recording its speech segments [(start, end), ...] in mel frames, end exclusive.
    The segment buffer is sized by segment_bound, so it cannot overflow.  Synchronises."""
    if isinstance(mels, torch.Tensor):
        if mels.dim() != 3 or mels.shape[0] < 1:
            raise ValueError(f"mels: expected (B, n_mel, T), got {tuple(mels.shape)}")
        if not isinstance(config, VadConfig):
            raise ValueError(f"speech_segments: config must be a VadConfig, got {type(config).__name__}")
        B, n_mel, T = mels.shape
        p = config.check(mel_seconds, n_mel)
        vad = StreamingVad(B, n_mel, config, mel_seconds, segment_bound(T, p.onset, p.hangover),
                           mels.device if mels.is_cuda else None)
        vad.step(mels, torch.full((B,), T, dtype=torch.int64) if lengths is None else lengths)
        return [r.segments for r in vad.finish()]
    if lengths is not None:
        raise ValueError("speech_segments: lengths goes with a (B, n_mel, T) batch; a sequence of recordings has their own")
    out = []
    for r, m in enumerate(mels):
        if not isinstance(m, torch.Tensor) or m.dim() != 2:
            raise ValueError(f"mels: recording {r}: expected log-mel frames (n_mel, n), got "
                             f"{tuple(m.shape) if isinstance(m, torch.Tensor) else type(m).__name__}")
        out += speech_segments(m.unsqueeze(0), None, config=config, mel_seconds=mel_seconds)
    return out
