"""What the per-slot objects share, stated once: the skeleton of a stream follower (StreamingEndpointer, StreamingConfidence,
StreamingKeywordSpotter, StreamingVad) and the open/close registry of the slot front ends (SlotStreamingEncoder,
StreamingAudioFrontend, StreamingResampler).

A follower keeps device state per slot, takes (S, rows, cols) fp32 input with a frame count per slot, and arms slots again
between streams.  The rules that every one of them follows live here: a host sequence of counts or slots goes to the device in
one pinned non-blocking copy; the stride of a dimension of 1 says nothing about a tensor's layout; a launch that takes at most
`cap` frames per slot sees the counts clamped to its own window.  Host code only: no kernel is called from this module.
"""
from __future__ import annotations

import math
from typing import Iterator, List, Optional, Sequence, Tuple

import torch

from . import _lib, ops


def positive_seconds(who: str, name: str, value) -> float:
    """The duration of a frame (`name`: frame_seconds, mel_seconds), checked on the host."""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or value <= 0:
        raise ValueError(f"{who}: {name} must be a positive finite number, got {value!r}")
    return float(value)


def frame_chunks(k: torch.Tensor, k_max: int, cap: int) -> Iterator[Tuple[int, int, torch.Tensor]]:
    """A step of k_max frames per slot for an entry that takes at most `cap` per launch: (t0, n, kk) per launch, the window
    [t0, t0 + n) and each slot's count inside it.  A step that fits one launch gets `k` itself: no device operation."""
    for t0 in range(0, k_max, cap):
        n = min(cap, k_max - t0)
        yield t0, n, k if k_max <= cap else (k - t0).clamp_(0, n)


class SlotFollower:
    """Base of the per-slot stream followers.  A subclass sets `_what` (the feature, as its refusals name it), calls
    _init_slots and _init_device from its constructor (host-argument refusals come before the device's) and declares
    `_armed_state`: the (tensor, fill) pairs that make a slot new, `fill` a Python scalar or a (1, ...) row of the tensor.
    reset_slots(slots) arms those slots again, reset() all of them; both enqueue only."""

    _what = ""
    _armed_state: Sequence[Tuple[torch.Tensor, object]] = ()

    def _init_slots(self, who: str, slots, *, strict: bool, max_slots: Optional[int] = None) -> None:
        """self.S.  strict: a true int in 1 .. max_slots (the kernels' grid); otherwise anything int() makes >= 1 of."""
        if strict:
            if isinstance(slots, bool) or not isinstance(slots, int) or not 1 <= slots <= max_slots:
                raise ValueError(f"{who}: slots must be 1 to {max_slots}, got {slots!r}")
        elif int(slots) < 1:
            raise ValueError(f"{who}: slots must be >= 1, got {slots}")
        self.S = int(slots)
        self._all: dict = {}               # k=None: the (S) int64 tensor of a k_max, made once per k_max

    def _init_device(self, who: str, device) -> None:
        """self.device: `device`, None: the current HIP device.  There is no CPU path."""
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise _lib.ConformerHipError(f"{who}: device {self.device}; {self._what} (no CPU fallback)")

    def _frame_counts(self, k, k_max: int, name: str = "k", allow_all: bool = True) -> torch.Tensor:
        """A step's frame counts as the entries take them, (S) int64 on the device: a device tensor as it is, a host sequence
        in one pinned non-blocking copy, None (with allow_all): k_max for every slot."""
        if k is None and allow_all:
            if k_max not in self._all:
                self._all[k_max] = torch.full((self.S,), k_max, dtype=torch.int64, device=self.device)
            return self._all[k_max]
        if isinstance(k, torch.Tensor) and k.is_cuda:
            k = ops._req(k, name, torch.int64)
        else:
            host = torch.as_tensor(k, dtype=torch.int64).reshape(-1)
            k = host.pin_memory().to(self.device, non_blocking=True)
        if k.dim() != 1 or k.numel() != self.S:
            raise ValueError(f"{name}: expected {self.S} frame counts, got shape {tuple(k.shape)}")
        return k

    def _device_input(self, x, name: str) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise _lib.ConformerHipError(f"{name}: expected a tensor on a HIP device, got {getattr(x, 'device', type(x))}; "
                                         f"{self._what} (no CPU fallback)")
        if x.dtype != torch.float32:
            raise _lib.ConformerHipError(f"{name}: expected dtype torch.float32, got {x.dtype}")
        return x

    def _pitches(self, x: torch.Tensor, rows: int, cols: int) -> Tuple[torch.Tensor, int, int]:
        """(x, ld_slot, ld_row) for x (S, rows, cols), a view or not: x itself where its rows are dense and neither rows nor
        slots overlap, a contiguous copy otherwise."""
        ld_row = x.stride(1) if rows > 1 else cols                         # (the stride of a dimension of 1 says nothing)
        if x.stride(2) != 1 or ld_row < cols or (self.S > 1 and x.stride(0) < rows * ld_row):
            x, ld_row = x.contiguous(), cols
        return x, (x.stride(0) if self.S > 1 else rows * ld_row), ld_row

    def _slot_list(self, slots=None) -> List[int]:
        slots = list(range(self.S)) if slots is None else [int(s) for s in slots]
        if any(not 0 <= s < self.S for s in slots):
            raise ValueError(f"slots {slots} outside [0, {self.S})")
        return slots

    def _slot_index(self, slots: Sequence[int]) -> torch.Tensor:
        return torch.tensor(list(slots), dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)

    def reset_slots(self, slots: Sequence[int]) -> None:
        slots = self._slot_list(slots)
        if not slots:
            return
        idx = self._slot_index(slots)
        for t, fill in self._armed_state:
            if isinstance(fill, torch.Tensor):
                t.index_copy_(0, idx, fill.expand(len(slots), *t.shape[1:]))
            else:
                t.index_fill_(0, idx, fill)

    def reset(self) -> None:
        for t, fill in self._armed_state:
            if isinstance(fill, torch.Tensor):
                t.copy_(fill.expand_as(t))
            else:
                t.fill_(fill)


class OpenSlots:
    """The registry of `self.S` slots that are open (a stream runs in them) or free: `is_open`, one bool per slot."""

    is_open: List[bool]

    def _check_slot(self, s: int, want_open: bool) -> int:
        s = int(s)
        if not 0 <= s < self.S:
            raise ValueError(f"slot {s} out of range [0, {self.S})")
        if self.is_open[s] != want_open:
            raise RuntimeError(f"slot {s} is {'free' if want_open else 'already open'}")
        return s

    def _mark_open(self, s: int) -> None:
        self.is_open[s] = True

    def _mark_closed(self, s: int) -> None:
        self.is_open[s] = False

    def _free_all(self) -> None:
        self.is_open = [False] * self.S
