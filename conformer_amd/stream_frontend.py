"""Streaming audio front end: waveform chunks in, log-mel frames out (INTEGRATION.md "Streaming audio front end").

ConformerAudioFrontend.mel_spectrogram needs the whole utterance: it reflect-pads both ends and frames the padded wave once.
StreamingAudioFrontend produces the same frames for `slots` independent live streams, each fed any number of samples per step
(0 included): for every stream the frames emitted from open(s) to its flush are the frames of mel_spectrogram on that stream's
own samples alone, in order, to GEMM rounding.

With pad = n_fft / 2 and n samples received, frame t covers samples [t hop - pad, t hop - pad + n_fft) of the reflect-padded
stream.  Mid-stream E(n) = (n - pad) // hop + 1 frames exist (0 while n <= pad: frame 0 reflects about sample 0 and needs
x[pad]); a flush of a stream of L samples brings the total to L // hop + 1 with its end reflected.  Each slot carries the samples
a later frame still needs, from stream position p0 = max(0, min(E hop - pad, n - (pad + 1))) on: at most n_fft - 1 of them (the
`min` keeps the pad + 1 samples a flush reflects).

Per step the host works out every slot's frames from the counts alone (frame_plan), sends one small table in a non-blocking
copy, and cfm_stream_stage_f32 gathers every slot's segment from [tail | new samples] into the padded-wave layout, both
reflections applied, and writes the new tails (two buffers, swapped per step).  The DFT GEMM over overlapping rows and the
power + mel + log kernel of the offline front end follow, unchanged.  The device sees tail-relative offsets only, so a stream has
no length limit; nothing synchronises with the host.

input=Resampler(device_rate, frontend.sample_rate): the streams arrive at another rate, as float32 or int16, mono or
interleaved (INTEGRATION.md "Input sample rates").  A StreamingResampler runs in front of the staging kernel, per slot, and
max_chunk_samples counts input-rate samples; everything above then holds for the resampled streams.
"""
from __future__ import annotations

from typing import Iterable, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib, ops
from ._slot_state import OpenSlots
from .frontend import ConformerAudioFrontend
from .resample import Resampler, ResampleStep, StreamingResampler

TAIL_LD = 512              # floats per row of a tail buffer (include/conformer_hip_stream_frontend.h)
TABLE_COLS = 8             # int32 per slot: tail_len, n_new, lead, n_frames, flush, off, keep, new_tail_len


class FramePlan(NamedTuple):
    """One slot's share of a step (frame_plan)."""
    frames: int            # frames that become computable
    lead: int              # reflected samples at the head of the segment (the utterance's opening)
    new_tail_len: int      # samples carried on (0 after a flush)
    tail_len: int          # samples carried in
    off: int               # index in [tail | new] of the segment's first sample (0 while lead > 0)
    keep: int              # index in [tail | new] where the new tail starts

    def row(self, new: int, flush: bool) -> Tuple[int, ...]:
        """The slot's row of the device table."""
        return (self.tail_len, new, self.lead, self.frames, int(flush), self.off, self.keep, self.new_tail_len)


def frames_so_far(received: int, hop: int, n_fft: int) -> int:
    """E(n): the frames a stream of n samples so far has emitted mid-stream."""
    pad = n_fft // 2
    return 0 if received <= pad else (received - pad) // hop + 1


def tail_start(emitted: int, received: int, hop: int, n_fft: int) -> int:
    """p0: the stream position of the first carried sample."""
    pad = n_fft // 2
    return max(0, min(emitted * hop - pad, received - (pad + 1)))


def frame_plan(received: int, new: int, flush: bool, emitted: int, hop: int, n_fft: int) -> FramePlan:
    """The host arithmetic of one slot's step: `received` samples and `emitted` frames before it, `new` samples in it, `flush`
    if the stream ends with it.  ValueError for a flush of a stream no longer than the reflect padding."""
    pad = n_fft // 2
    n = received + new
    if flush:
        if n <= pad:
            raise ValueError(f"a stream of {n} samples is not longer than the reflect padding ({pad}): nothing to flush")
        total = n // hop + 1
    else:
        total = frames_so_far(n, hop, n_fft)
    p0 = tail_start(emitted, received, hop, n_fft)
    p1 = n if flush else tail_start(total, n, hop, n_fft)
    return FramePlan(frames=total - emitted, lead=max(0, pad - emitted * hop), new_tail_len=n - p1, tail_len=received - p0,
                     off=max(0, emitted * hop - pad - p0), keep=p1 - p0)


class StepPlan(NamedTuple):
    """A checked step of StreamingAudioFrontend (plan): nothing enqueued, no state changed."""
    samples: torch.Tensor
    counts: List[int]
    flush: List[bool]
    slots: List[FramePlan]
    frames: List[int]
    f_max: int
    resample: Optional[ResampleStep] = None    # with input=: the resampler's checked step; `samples` is then the buffer it fills


class StreamingAudioFrontend(OpenSlots):
    """`slots` independent streams through `frontend`'s log-mel configuration, at most max_chunk_samples new samples per slot
    and step.

        fe.open(s); mel, frames = fe.step(samples, counts, flush=()); fe.close(s)

    Slot b's new frames are mel[b, :, :frames[b]]: what SlotStreamingEncoder.step(mel, frames) takes.
    input: a Resampler to frontend.sample_rate; step() then takes samples at its orig_rate, (S, N) or (S, N, C), float32 or
    int16, and max_chunk_samples counts those."""

    def __init__(self, frontend: ConformerAudioFrontend, slots: int, max_chunk_samples: int,
                 input: Optional[Resampler] = None) -> None:
        hop, n_fft = frontend.hop_length, frontend.n_fft
        if hop % 4 or hop > n_fft:
            raise NotImplementedError(f"StreamingAudioFrontend: hop_length {hop}: the overlapping-rows DFT GEMM needs hop % 4 == 0 "
                                      f"and frames that leave no gap need hop <= n_fft ({n_fft})")
        if int(slots) < 1 or int(max_chunk_samples) < 1:
            raise ValueError(f"StreamingAudioFrontend: slots ({slots}) and max_chunk_samples ({max_chunk_samples}) must be >= 1")
        self.fe, self.S, self.max_chunk = frontend, int(slots), int(max_chunk_samples)
        self.input = None
        if input is not None:
            if input.new_rate != frontend.sample_rate or input.device != frontend.device:
                raise ValueError(f"StreamingAudioFrontend: input resamples to {input.new_rate} Hz on {input.device}, the front end "
                                 f"takes {frontend.sample_rate} Hz on {frontend.device}")
            self.input = StreamingResampler(input, slots, max_chunk_samples)
        # the most samples at the front end's rate one step can bring (with input=: the most outputs of a resampler step)
        self.chunk = self.max_chunk if self.input is None else self.input.out_cap
        self.hop, self.n_fft, self.pad = hop, n_fft, n_fft // 2
        self.extra = (n_fft + hop - 1) // hop                              # rows per slot behind its frames: rpu = f_max + extra
        # the most frames one step can bring: E(n + c) - E(n) <= c // hop + 1, and a flush adds L // hop - (L - pad) // hop
        self.f_cap = self.chunk // hop + 1 + self.pad // hop + 1
        dev, S = frontend.device, self.S
        self.device = dev
        self.tails = [torch.zeros(S, TAIL_LD, device=dev, dtype=torch.float32) for _ in range(2)]
        self.xp = torch.zeros(S * (self.f_cap + self.extra) * hop + n_fft, device=dev, dtype=torch.float32)
        self.spec = torch.empty(S * (self.f_cap + self.extra), frontend.basis.shape[0], device=dev, dtype=torch.float32)
        # with input=, the resampler's table sits behind this one: one copy per step sends both
        self.tables = torch.zeros(1 if self.input is None else 2, S, TABLE_COLS, device=dev, dtype=torch.int32)
        self.table = self.tables[0]
        if self.input is not None:
            self.input.table = self.tables[1]
        self._free_all()
        self.received = [0] * S                                            # samples per slot since open
        self.emitted = [0] * S                                             # frames per slot since open

    def open(self, s: int) -> None:
        """Start a new stream in free slot s (host bookkeeping only: an empty tail is a tail length of 0)."""
        s = self._check_slot(s, want_open=False)
        self.received[s] = self.emitted[s] = 0
        self._mark_open(s)
        if self.input is not None:
            self.input.open(s)

    def close(self, s: int) -> None:
        """Drop slot s's stream without a flush."""
        self._mark_closed(self._check_slot(s, want_open=True))
        if self.input is not None:
            self.input.close(s)

    def reset(self) -> None:
        """Every slot free."""
        self._free_all()
        if self.input is not None:
            self.input.reset()

    def plan(self, samples: torch.Tensor, counts: Sequence[int], flush: Iterable[int] = ()) -> StepPlan:
        """Check a step's arguments against the slots (raises before anything is enqueued, changes nothing).  With input= the
        resampler's checks come first, then the front end's on the resampled counts, which the host knows without the samples."""
        flush = list(flush)
        if self.input is not None:
            rp = self.input.plan(samples, counts, flush)
            return self._plan(None, self.input.out_cap, rp.out_counts, flush, rp)
        if not isinstance(samples, torch.Tensor) or samples.dim() != 2 or samples.shape[0] != self.S:
            raise ValueError(f"samples: expected a ({self.S}, N) tensor, got {tuple(getattr(samples, 'shape', ()))}")
        N = samples.shape[1]
        if N > self.max_chunk:
            raise ValueError(f"samples: {N} per slot, the buffers were sized for max_chunk_samples={self.max_chunk}")
        counts = [int(c) for c in counts]
        if len(counts) != self.S:
            raise ValueError(f"counts: expected {self.S} counts, got {len(counts)}")
        return self._plan(samples, N, counts, flush, None)

    def _plan(self, samples: Optional[torch.Tensor], N: int, counts: List[int], flush: Iterable[int],
              rp: Optional[ResampleStep]) -> StepPlan:
        """The front end's own checks: counts[b] samples at its rate for slot b, of N per row."""
        ends = [False] * self.S
        for s in flush:
            s = int(s)
            if not 0 <= s < self.S:
                raise ValueError(f"flush: slot {s} out of range [0, {self.S})")
            if not self.is_open[s]:
                raise RuntimeError(f"flush of free slot {s}")
            ends[s] = True
        slots = []
        for b, c in enumerate(counts):
            if not 0 <= c <= N:
                raise ValueError(f"counts[{b}] = {c} outside [0, {N}]")
            if c and not self.is_open[b]:
                raise RuntimeError(f"samples given for free slot {b}: open() it first")
            if not self.is_open[b]:
                slots.append(FramePlan(0, 0, 0, 0, 0, 0))
                continue
            try:
                slots.append(frame_plan(self.received[b], c, ends[b], self.emitted[b], self.hop, self.n_fft))
            except ValueError as e:
                raise ValueError(f"slot {b}: {e}") from None
        frames = [p.frames for p in slots]
        if rp is not None:
            # the buffer run() has the resampler fill (an allocation enqueues nothing)
            x = torch.empty(self.S, N, device=self.device, dtype=torch.float32)
        else:
            x = ops._req(samples, "samples")                               # (fp32 on the HIP device: there is no CPU path)
        return StepPlan(x, counts, ends, slots, frames, max(frames), rp)

    @torch.no_grad()
    def step(self, samples: torch.Tensor, counts: Sequence[int], flush: Iterable[int] = ()) -> Tuple[torch.Tensor, List[int]]:
        """samples (S, N) fp32 on the device (with input=: (S, N) or (S, N, C), float32 or int16, at the input rate): slot b's
        next counts[b] samples are samples[b, :counts[b]] (the rest is ignored; free slots take 0).  flush: the slots whose
        stream ends with this step (a count of 0 is allowed); they are closed afterwards.  Returns mel (S, n_mels, f_max) and
        frames (host list): slot b's new frames are mel[b, :, :frames[b]], the columns behind them are finite and otherwise
        unspecified."""
        return self.run(self.plan(samples, counts, flush))

    @torch.no_grad()
    def run(self, p: StepPlan) -> Tuple[torch.Tensor, List[int]]:
        """Enqueue a step that plan() checked (no slot may have changed in between)."""
        S, hop, n_fft, fe = self.S, self.hop, self.n_fft, self.fe
        host = torch.empty(self.tables.shape, dtype=torch.int32, pin_memory=True)  # (a fresh one: the copy below may still be pending)
        host.numpy()[0] = [q.row(c, e) for q, c, e in zip(p.slots, p.counts, p.flush)]
        if p.resample is not None:
            host.numpy()[1] = self.input.rows(p.resample)
        self.tables.copy_(host, non_blocking=True)
        if p.resample is not None:
            self.input.run(p.resample, out=p.samples, table_sent=True)
        x, f_max = p.samples, p.f_max
        stream = ops._stream()
        _lib.call("cfm_stream_stage_f32", x.data_ptr() if x.shape[1] else None, x.shape[1], x.shape[1],
                  self.tails[0].data_ptr(), self.tails[1].data_ptr(), self.table.data_ptr(), self.xp.data_ptr(), S, f_max, hop,
                  n_fft, stream)
        self.tails.reverse()
        for b in range(S):
            self.received[b] += p.counts[b]
            self.emitted[b] += p.frames[b]
            if p.flush[b]:
                self._mark_closed(b)
        out = torch.empty(S, fe.n_mels, f_max, device=self.device, dtype=torch.float32)
        if f_max == 0:
            return out, p.frames
        rpu, nb2 = f_max + self.extra, fe.basis.shape[0]
        _lib.call("cfm_dft_frames_f32", self.xp.data_ptr(), fe.basis.data_ptr(), self.spec.data_ptr(), S * rpu, nb2, n_fft, hop,
                  stream)
        _lib.call("cfm_power_mel_log_mfma_f32", self.spec.data_ptr(), nb2, fe.fbT.data_ptr(), out.data_ptr(), S, f_max, rpu,
                  n_fft // 2 + 1, fe.n_mels, 1e-5, stream)
        return out, p.frames
