"""Input sample rates: resample device audio to the front end's rate, offline and per slot in streams (INTEGRATION.md "Input
sample rates").

The definition is the Hann-windowed-sinc polyphase resampler (torchaudio's default `sinc_interp_hann`).  For rates R_in -> R_out
let g = gcd, o = R_in / g, n = R_out / g, base = min(o, n) rolloff, width = ceil(lpw o / base), K = 2 width + o.  The bank has n
phases of K taps,
    t = clip(((m - width) / o - j / n) base, -lpw, lpw),   k[j, m] = sinc(t) cos(pi t / (2 lpw))^2 base / o,
built in float64 and rounded once to fp32, and output q = i n + j of an utterance of L samples is
    y[q] = sum_m k[j, m] x[i o - width + m]   (x = 0 outside [0, L)),   0 <= q < ceil(n L / o).
Equal rates are no filter: the bank is the single tap 1 and samples pass through bit for bit (after conversion and downmix).

Input is float32 or int16 (float(v) * 2^-15), mono (B, L) or interleaved (B, L, C), C <= 8, downmixed as
(x_0 + ... + x_{C-1}) * fp32(1 / C), summed left to right.

Streaming: a stream that has received N samples has emitted the blocks i < Eb(N) = max(0, (N - width) // o), n Eb samples: the
blocks whose last tap has arrived.  A flush of a stream of L samples brings the total to ceil(n L / o).  The slot carries the
samples from position max(0, Eb o - width) on (< K of them); while that position is 0 the max(0, width - Eb o) leading zeros are
implied.  The added latency is width / R_in seconds.  The host plans every step from the counts alone (resample_plan), sends one
small int32 table in a non-blocking copy, and one launch (cfm_resample_f32 / cfm_resample_i16) gathers [tail | new samples],
writes every slot's outputs, zeros behind them and the new tails (two buffers, swapped per step).  Nothing synchronises.
"""
from __future__ import annotations

import math
from typing import Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from ._slot_state import OpenSlots

TAIL_LD = 1024             # floats per row of a tail buffer (include/conformer_hip_resample.h)
TABLE_COLS = 8             # int32 per slot: tail_len, n_new, lead, n_out, flush, keep, new_tail_len, 0
K_MAX, N_MAX, C_MAX = 1024, 640, 8
_ENTRY = {torch.float32: "cfm_resample_f32", torch.int16: "cfm_resample_i16"}


def resample_geometry(orig_rate: int, new_rate: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> Tuple[int, int, int]:
    """(width, o, n); K = 2 width + o.  Equal rates: (0, 1, 1)."""
    orig_rate, new_rate, lpw = int(orig_rate), int(new_rate), int(lowpass_filter_width)
    if orig_rate < 1 or new_rate < 1 or lpw < 1 or not 0.0 < float(rolloff) <= 1.0:
        raise ValueError(f"resample: rates ({orig_rate}, {new_rate}), lowpass_filter_width {lpw} and rolloff {rolloff} must be "
                         "positive, rolloff at most 1")
    g = math.gcd(orig_rate, new_rate)
    o, n = orig_rate // g, new_rate // g
    if o == n:
        return 0, 1, 1
    return int(math.ceil(lpw * o / (min(o, n) * float(rolloff)))), o, n


def resample_bank(orig_rate: int, new_rate: int, lowpass_filter_width: int = 6,
                  rolloff: float = 0.99) -> Tuple[np.ndarray, Tuple[int, int, int]]:
    """The float64 bank (n, K) and (width, o, n).  Equal rates: the single tap 1, width 0."""
    width, o, n = resample_geometry(orig_rate, new_rate, lowpass_filter_width, rolloff)
    if o == n:
        return np.ones((1, 1), np.float64), (0, 1, 1)
    lpw, base = int(lowpass_filter_width), min(o, n) * float(rolloff)
    m = np.arange(2 * width + o, dtype=np.float64)[None, :]
    j = np.arange(n, dtype=np.float64)[:, None]
    t = np.clip(((m - width) / o - j / n) * base, -lpw, lpw)
    return np.sinc(t) * np.cos(np.pi * t / (2 * lpw)) ** 2 * (base / o), (width, o, n)


def blocks_so_far(received: int, width: int, o: int) -> int:
    """Eb(N): the blocks of n outputs a stream of N samples so far has emitted mid-stream."""
    return max(0, (received - width) // o)


def output_length(length: int, o: int, n: int) -> int:
    """ceil(n L / o): the outputs of a whole utterance of L samples."""
    return -(-n * length // o)


class SlotPlan(NamedTuple):
    """One slot's share of a step (resample_plan)."""
    outputs: int           # outputs that become computable
    lead: int              # implied zeros in front of [tail | new] (while the tail still starts at sample 0)
    new_tail_len: int      # samples carried on (0 after a flush)
    tail_len: int          # samples carried in
    keep: int              # index in [tail | new] where the new tail starts

    def row(self, new: int, flush: bool) -> Tuple[int, ...]:
        """The slot's row of the device table."""
        return (self.tail_len, new, self.lead, self.outputs, int(flush), self.keep, self.new_tail_len, 0)


def resample_plan(received: int, new: int, flush: bool, width: int, o: int, n: int) -> SlotPlan:
    """The host arithmetic of one slot's step: `received` samples before it, `new` samples in it, `flush` if the stream ends
    with it."""
    eb0, total_in = blocks_so_far(received, width, o), received + new
    p0 = max(0, eb0 * o - width)
    if flush:
        total_out, p1 = output_length(total_in, o, n), total_in
    else:
        eb1 = blocks_so_far(total_in, width, o)
        total_out, p1 = n * eb1, max(0, eb1 * o - width)
    return SlotPlan(outputs=total_out - n * eb0, lead=max(0, width - eb0 * o), new_tail_len=total_in - p1,
                    tail_len=received - p0, keep=p1 - p0)


def step_output_cap(max_chunk: int, width: int, o: int, n: int) -> int:
    """The most outputs one step of at most max_chunk new samples can bring.  A flush at N + c samples after Eb(N) blocks brings
    ceil(n (N + c) / o) - n Eb(N) <= n (N + c) / o + 1 - n (N - width - o + 1) / o = n (c + width + o - 1) / o + 1, and a step
    without one brings n (Eb(N + c) - Eb(N)) <= n (c / o + 1), which is not more."""
    return n * (max_chunk + width + o - 1) // o + 1


def _check_samples(x: torch.Tensor, name: str, device: torch.device) -> Tuple[torch.Tensor, int]:
    """(x contiguous, channels) of a (B, L) or (B, L, C) float32 / int16 tensor on the device."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3):
        raise ValueError(f"{name}: expected a (B, L) or (B, L, C) tensor, got {tuple(getattr(x, 'shape', ()))}")
    if x.dtype not in _ENTRY:
        raise _lib.ConformerHipError(f"{name}: expected float32 or int16 samples, got {x.dtype}")
    x = ops._req(x, name, x.dtype)
    if x.device != device and not (device.index is None and x.device.type == device.type):
        raise _lib.ConformerHipError(f"{name}: on {x.device}, the resampler is on {device}")
    C = x.shape[2] if x.dim() == 3 else 1
    if not 1 <= C <= C_MAX:
        raise NotImplementedError(f"{name}: {C} interleaved channels, the kernel downmixes 1 to {C_MAX}")
    return x, C


class Resampler:
    """orig_rate -> new_rate on the device.

        y, out_lengths = Resampler(44100)(x, lengths)

    x (B, L) or (B, L, C) float32 / int16; row b's samples behind lengths[b] are never read; y (B, ceil(n L / o)) fp32 with
    zeros behind out_lengths[b] = ceil(n lengths[b] / o)."""

    def __init__(self, orig_rate: int, new_rate: int = 16000, device="cuda:0", lowpass_filter_width: int = 6,
                 rolloff: float = 0.99) -> None:
        self.width, self.o, self.n = resample_geometry(orig_rate, new_rate, lowpass_filter_width, rolloff)
        self.orig_rate, self.new_rate = int(orig_rate), int(new_rate)
        self.K = 2 * self.width + self.o
        if self.K > K_MAX or self.n > N_MAX:                             # (before the bank is built: it has n K entries)
            raise NotImplementedError(f"Resampler: {orig_rate} -> {new_rate} Hz needs {self.n} phases of {self.K} taps, the kernel "
                                      f"holds at most {N_MAX} phases of {K_MAX} taps")
        bank, _ = resample_bank(orig_rate, new_rate, lowpass_filter_width, rolloff)
        self.device = torch.device(device)
        self.bank = bank                                                             # float64 (n, K): the definition
        self.bank_t = torch.from_numpy(np.ascontiguousarray(bank.T.astype(np.float32))).to(self.device)   # (K, n): what the kernel reads

    def output_length(self, length: int) -> int:
        return output_length(int(length), self.o, self.n)

    def launch(self, x: torch.Tensor, C: int, n_max: int, tails: Optional[Tuple[torch.Tensor, torch.Tensor]],
               table: torch.Tensor, y: torch.Tensor) -> None:
        """One cfm_resample_* launch: x (S, ...) contiguous, y (S, ld_y) fp32, table (S, 8) int32 on the device."""
        S = y.shape[0]
        ld = n_max * C                                                     # (x is contiguous, n_max = x.shape[1])
        tin, tout = (tails[0].data_ptr(), tails[1].data_ptr()) if tails is not None else (None, None)
        _lib.call(_ENTRY[x.dtype], x.data_ptr() if n_max else None, ld, n_max, C, tin, tout, table.data_ptr(),
                  self.bank_t.data_ptr(), self.o, self.n, self.width, y.data_ptr(), y.shape[1], S, ops._stream())

    @torch.no_grad()
    def __call__(self, x: torch.Tensor, lengths=None) -> Tuple[torch.Tensor, List[int]]:
        x, C = _check_samples(x, "x", self.device)
        B, L = x.shape[0], x.shape[1]
        if B < 1:
            raise ValueError("x: an empty batch")
        if lengths is None:
            lengths = [L] * B
        elif isinstance(lengths, torch.Tensor):
            lengths = lengths.tolist()
        lengths = [int(v) for v in lengths]
        if len(lengths) != B or any(not 0 <= v <= L for v in lengths):
            raise ValueError(f"lengths: expected {B} lengths in [0, {L}], got {lengths}")
        out = [self.output_length(v) for v in lengths]
        ld_y = (self.output_length(L) + 3) // 4 * 4
        y = torch.empty(B, ld_y, device=self.device, dtype=torch.float32)
        # the streaming launch with empty tails and every row flushed
        table = torch.tensor([(0, v, self.width, q, 1, 0, 0, 0) for v, q in zip(lengths, out)], dtype=torch.int32).to(self.device)
        self.launch(x, C, L, None, table, y)
        return y[:, :self.output_length(L)], out


class ResampleStep(NamedTuple):
    """A checked step of StreamingResampler (plan): nothing enqueued, no state changed."""
    samples: torch.Tensor
    channels: int
    counts: List[int]
    flush: List[bool]
    slots: List[SlotPlan]
    out_counts: List[int]


class StreamingResampler(OpenSlots):
    """`slots` independent streams through `resampler`, at most max_chunk_samples new (input-rate) samples per slot and step.

        rs.open(s); y, out_counts = rs.step(samples, counts, flush=()); rs.close(s)

    Slot b's new output samples are y[b, :out_counts[b]], zeros behind them; y is (S, out_cap)."""

    def __init__(self, resampler: Resampler, slots: int, max_chunk_samples: int) -> None:
        if int(slots) < 1 or int(max_chunk_samples) < 1:
            raise ValueError(f"StreamingResampler: slots ({slots}) and max_chunk_samples ({max_chunk_samples}) must be >= 1")
        self.rs, self.S, self.max_chunk = resampler, int(slots), int(max_chunk_samples)
        self.device = resampler.device
        r = resampler
        self.out_cap = (step_output_cap(self.max_chunk, r.width, r.o, r.n) + 3) // 4 * 4     # (the kernel's pitch: 16 bytes)
        self.tails = [torch.zeros(self.S, TAIL_LD, device=self.device, dtype=torch.float32) for _ in range(2)]
        self.table = torch.zeros(self.S, TABLE_COLS, device=self.device, dtype=torch.int32)
        self._free_all()
        self.received = [0] * self.S                                       # input samples per slot since open

    def open(self, s: int) -> None:
        """Start a new stream in free slot s (host bookkeeping only: an empty tail is a tail length of 0)."""
        s = self._check_slot(s, want_open=False)
        self.received[s] = 0
        self._mark_open(s)

    def close(self, s: int) -> None:
        """Drop slot s's stream without a flush."""
        self._mark_closed(self._check_slot(s, want_open=True))

    def reset(self) -> None:
        """Every slot free."""
        self._free_all()

    def plan(self, samples: torch.Tensor, counts: Sequence[int], flush: Iterable[int] = ()) -> ResampleStep:
        """Check a step's arguments against the slots (raises before anything is enqueued, changes nothing)."""
        x, C = _check_samples(samples, "samples", self.device)
        if x.shape[0] != self.S:
            raise ValueError(f"samples: expected {self.S} rows, got {tuple(x.shape)}")
        N = x.shape[1]
        if N > self.max_chunk:
            raise ValueError(f"samples: {N} per slot, the buffers were sized for max_chunk_samples={self.max_chunk}")
        counts = [int(c) for c in counts]
        if len(counts) != self.S:
            raise ValueError(f"counts: expected {self.S} counts, got {len(counts)}")
        ends = [False] * self.S
        for s in flush:
            s = int(s)
            if not 0 <= s < self.S:
                raise ValueError(f"flush: slot {s} out of range [0, {self.S})")
            if not self.is_open[s]:
                raise RuntimeError(f"flush of free slot {s}")
            ends[s] = True
        slots, r = [], self.rs
        for b, c in enumerate(counts):
            if not 0 <= c <= N:
                raise ValueError(f"counts[{b}] = {c} outside [0, {N}]")
            if c and not self.is_open[b]:
                raise RuntimeError(f"samples given for free slot {b}: open() it first")
            slots.append(resample_plan(self.received[b], c, ends[b], r.width, r.o, r.n) if self.is_open[b]
                         else SlotPlan(0, 0, 0, 0, 0))
        return ResampleStep(x, C, counts, ends, slots, [p.outputs for p in slots])

    @torch.no_grad()
    def step(self, samples: torch.Tensor, counts: Sequence[int], flush: Iterable[int] = ()) -> Tuple[torch.Tensor, List[int]]:
        """samples (S, N) or (S, N, C), float32 or int16 on the device: slot b's next counts[b] samples are samples[b,
        :counts[b]] (the rest is never read; free slots take 0).  flush: the slots whose stream ends with this step (a count of
        0 is allowed); they are free afterwards.  Returns y (S, out_cap) fp32 and out_counts (host list)."""
        return self.run(self.plan(samples, counts, flush))

    @staticmethod
    def rows(p: ResampleStep) -> List[Tuple[int, ...]]:
        """The device table of a checked step."""
        return [q.row(c, e) for q, c, e in zip(p.slots, p.counts, p.flush)]

    @torch.no_grad()
    def run(self, p: ResampleStep, out: Optional[torch.Tensor] = None, table_sent: bool = False) -> Tuple[torch.Tensor, List[int]]:
        """Enqueue a step that plan() checked (no slot may have changed in between).  out: a (S, out_cap) fp32 buffer to write.
        table_sent: the caller has enqueued the copy of rows(p) into self.table itself (StreamingAudioFrontend sends it with its
        own table in one copy)."""
        S = self.S
        if not table_sent:
            host = torch.empty(S, TABLE_COLS, dtype=torch.int32, pin_memory=True)  # (a fresh one: the copy below may still be pending)
            host.numpy()[:] = self.rows(p)
            self.table.copy_(host, non_blocking=True)
        y = torch.empty(S, self.out_cap, device=self.device, dtype=torch.float32) if out is None else out
        self.rs.launch(p.samples, p.channels, p.samples.shape[1], (self.tails[0], self.tails[1]), self.table, y)
        self.tails.reverse()
        for b in range(S):
            self.received[b] += p.counts[b]
            if p.flush[b]:
                self._mark_closed(b)
        return y, p.out_counts
