"""Waveform augmentation on the device, in front of the log-mel: speed perturbation, reverberation, additive noise at a drawn
SNR and a gain (INTEGRATION.md "Waveform augmentation"; the C entries: csrc/conformer_hip3_waveaug.h).

Input is `wave (B, Lmax)` fp32 on the device with host `lengths`; samples behind lengths[b] are never read.  The stages run in
this order, and a row that a stage skips leaves that stage bit for bit unchanged:

 1. Speed.  Factor (num, den): the row passes through Resampler(orig_rate=num, new_rate=den) (resample.py), length
    ceil(den L / num).  Rows are grouped by factor, one resampler launch per factor present; rows at (1, 1) are copied.
 2. Reverb.  y[t] = sum_k h_r[k] x[t + d_r - k], 0 <= t < L, x = 0 outside [0, L), with d_r the first index of max |h_r|: the
    length is kept and the direct path stays where it was.
 3. Mix.  n[t] = clip_c[(s + t) mod N_c], Px = sum x^2 and Pn = sum n^2 over t < L in double,
    g = sqrt(Px / (Pn 10^(snr_db / 10))) (0 unless Px > 0 and Pn > 0), a = 10^(gain_db / 20),
    y[t] = fp32(a) x[t] + fp32(a g) n[t].

`draw` is host only and draws one (B, 8) float64 block, u = torch.rand(B, 8, dtype=float64, generator=self.generator), row b =
(speed, reverb?, rir, noise?, clip, offset, snr, gain): speed index = floor(u0 len(speeds)); a reverb iff u1 < p_reverb, its
response floor(u2 R); noise iff u3 < p_noise, its clip c = floor(u4 N), offset floor(u5 N_c);
snr_db = lo + u6 (hi - lo); gain_db = lo + u7 (hi - lo).  All eight are drawn for every row whether used or not, so a seed
reproduces a plan and a row's choices do not depend on its neighbours'.

`apply` checks the whole plan before the first launch, sends every per-row table in ONE pinned non-blocking copy, reads nothing
back, and launches at most: for the speed stage one gather of the rows to resample, one resampler launch per factor other than
(1, 1) present, one scatter and one copy of the (1, 1) rows; one FIR launch; one power launch and one mix launch.  A stage
nobody drew launches nothing (with no stage at all: one copy, for the zeros behind the lengths)."""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from .resample import K_MAX, N_MAX, output_length, resample_geometry

_C = _lib.OPEN_CONSTANTS["conformer_hip3_waveaug.h"]
FIR_TILE_T = _C["CFM3_WAVE_FIR_TILE_T"]          # outputs of one row per workgroup of the FIR kernel
FIR_TILE_K = _C["CFM3_WAVE_FIR_TILE_K"]          # taps per staged tile
FIR_MAX_TAPS = _C["CFM3_WAVE_FIR_MAX_TAPS"]      # the longest impulse response
POWER_CHUNK = _C["CFM3_WAVE_POWER_CHUNK"]        # samples per partial sum of the powers
MIX_TILE = _C["CFM3_WAVE_MIX_TILE"]              # samples per workgroup of the mix kernel
ROW_COLS = _C["CFM3_WAVE_ROW_COLS"]
DEFAULT_SPEEDS = ((9, 10), (1, 1), (11, 10))
_INT_MAX = 2 ** 31 - 1


def _as_rows(items, what: str) -> List[np.ndarray]:
    """A list of 1-D arrays from a list of 1-D tensors / arrays."""
    out = []
    for i, h in enumerate(items):
        a = h.detach().cpu().numpy() if isinstance(h, torch.Tensor) else np.asarray(h)
        if a.ndim != 1:
            raise ValueError(f"{what}[{i}]: expected a 1-D tensor, got shape {tuple(a.shape)}")
        if a.shape[0] < 1:
            raise ValueError(f"{what}[{i}] is empty")
        if not np.isfinite(a).all():
            raise ValueError(f"{what}[{i}] holds a NaN or an infinity")
        out.append(a)
    if not out:
        raise ValueError(f"{what}: an empty bank")
    return out


class _Bank:
    """Arrays back to back in one fp32 buffer with an (n + 1) int32 offset table; the device copy is made on first use."""

    def __init__(self, arrays: List[np.ndarray], what: str) -> None:
        self.sizes = [int(a.shape[0]) for a in arrays]
        if sum(self.sizes) > _INT_MAX:
            raise NotImplementedError(f"{what}: {sum(self.sizes)} samples in all, the offset table is int32")
        self.data = np.concatenate(arrays).astype(np.float32, copy=False)
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int32)
        self._on: Dict[torch.device, tuple] = {}

    def __len__(self) -> int:
        return len(self.sizes)

    def _extra(self) -> tuple:
        return ()

    def on(self, device: torch.device) -> tuple:
        if device not in self._on:
            self._on[device] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device)
                                     for a in (self.data, self.offsets, *self._extra()))
        return self._on[device]


class RirBank(_Bank):
    """R impulse responses of K_r >= 1 taps (1-D float tensors or arrays).  In float64: d_r = the first index of max |h_r| (the
    direct path); with normalize=True h_r is divided by its L2 norm (an all-zero response is refused); then the taps are rounded
    once to fp32.  normalize=False keeps fp32 taps bit for bit.  `taps[r]` is what the kernel reads, `delays[r]` is d_r."""

    def __init__(self, rirs, normalize: bool = True) -> None:
        rows = _as_rows(rirs, "rirs")
        taps, delays = [], []
        for r, h in enumerate(rows):
            if h.shape[0] > FIR_MAX_TAPS:
                raise NotImplementedError(f"rirs[{r}] has {h.shape[0]} taps, the FIR kernel holds at most {FIR_MAX_TAPS}")
            h64 = h.astype(np.float64)
            delays.append(int(np.argmax(np.abs(h64))))                      # (argmax: the first maximum)
            if normalize:
                norm = math.sqrt(float(np.dot(h64, h64)))
                if not norm > 0.0:
                    raise ValueError(f"rirs[{r}] is all zero: it has no norm to divide by")
                h64 = h64 / norm
            taps.append(h64.astype(np.float32))
        super().__init__(taps, "rirs")
        self.normalize = bool(normalize)
        self.taps = [self.data[a:b] for a, b in zip(self.offsets[:-1], self.offsets[1:])]
        self.delays = delays
        self.k_max = max(self.sizes)

    def _extra(self) -> tuple:
        return (np.asarray(self.delays, np.int32),)


class NoiseBank(_Bank):
    """N noise clips of N_c >= 1 samples (1-D float tensors or arrays), rounded once to fp32; a row starts at offset s in its
    clip and wraps around: n[t] = clip[(s + t) mod N_c]."""

    def __init__(self, clips) -> None:
        super().__init__([c.astype(np.float32) for c in _as_rows(clips, "clips")], "clips")
        self.clips = [self.data[a:b] for a, b in zip(self.offsets[:-1], self.offsets[1:])]


class WavePlan(NamedTuple):
    """The choices of one batch, one entry per row; built by WaveAugment.draw or by hand."""
    speed: List[int]           # index into WaveAugment.speeds
    rir: List[int]             # index into the RirBank, -1 = no reverb
    clip: List[int]            # index into the NoiseBank, -1 = no noise
    offset: List[int]          # where the row starts in its clip, 0 <= offset < N_c (0 without a clip)
    snr_db: List[float]        # the SNR of the mix (not used without a clip)
    gain_db: List[float]       # the gain; a row with neither a clip nor a gain other than 0 skips the mix


def _range(v, what: str) -> Tuple[float, float]:
    lo, hi = (float(v), float(v)) if isinstance(v, (int, float)) else (float(v[0]), float(v[1]))
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError(f"{what}: expected finite (lo, hi) with lo <= hi, got {v}")
    return lo, hi


def _pitch(t: torch.Tensor) -> int:
    """floats from one row of a (rows, columns) tensor to the next (a single row's own stride says nothing)"""
    return t.stride(0) if t.shape[0] > 1 else max(1, t.shape[1])


class WaveAugment:
    """wave2, lengths2 = wa(wave, lengths)        # = wa.apply(wave, lengths, wa.draw(lengths))

    speeds: the factors (num, den) a row draws from uniformly (None or (): no speed stage).  p_reverb / rirs, p_noise / noise:
    the probability of the stage for a row and its bank; a probability above 0 needs its bank.  snr_db, gain_db: (lo, hi), drawn
    uniformly.  `generator`: the CPU generator `draw` uses; None = torch's default."""

    def __init__(self, speeds: Optional[Sequence[Tuple[int, int]]] = DEFAULT_SPEEDS, p_reverb: float = 0.0,
                 rirs: Optional[RirBank] = None, p_noise: float = 0.0, noise: Optional[NoiseBank] = None,
                 snr_db=(5.0, 25.0), gain_db=(0.0, 0.0), device="cuda:0") -> None:
        self.speeds = tuple((int(a), int(b)) for a, b in (speeds or ((1, 1),)))
        self.geometry = []                                                 # (width, o, n) per factor
        for num, den in self.speeds:
            width, o, n = resample_geometry(num, den)
            if 2 * width + o > K_MAX or n > N_MAX:
                raise NotImplementedError(f"WaveAugment: speed {num}:{den} needs {n} phases of {2 * width + o} taps, the resampler "
                                          f"holds at most {N_MAX} phases of {K_MAX} taps")
            self.geometry.append((width, o, n))
        self.p_reverb, self.p_noise = float(p_reverb), float(p_noise)
        if not (0.0 <= self.p_reverb <= 1.0 and 0.0 <= self.p_noise <= 1.0):
            raise ValueError(f"WaveAugment: p_reverb ({p_reverb}) and p_noise ({p_noise}) are probabilities")
        if rirs is not None and not isinstance(rirs, RirBank) or noise is not None and not isinstance(noise, NoiseBank):
            raise TypeError("WaveAugment: rirs is a RirBank and noise a NoiseBank")
        if self.p_reverb > 0.0 and rirs is None:
            raise ValueError(f"WaveAugment: p_reverb = {p_reverb} without a RirBank")
        if self.p_noise > 0.0 and noise is None:
            raise ValueError(f"WaveAugment: p_noise = {p_noise} without a NoiseBank")
        self.rirs, self.noise = rirs, noise
        self.snr_db, self.gain_db = _range(snr_db, "snr_db"), _range(gain_db, "gain_db")
        self.device = torch.device(device)
        self.generator: Optional[torch.Generator] = None            # None = torch's default CPU generator
        self._resamplers: dict = {}                                 # speed index -> Resampler, made on first use

    # ---- host ------------------------------------------------------------------------------------------------------------------
    def draw(self, lengths: Sequence[int]) -> WavePlan:
        """The plan of a batch of len(lengths) rows (host only; the order of the draws is in the module docstring)."""
        B = len(lengths)
        u = torch.rand(B, 8, dtype=torch.float64, generator=self.generator).tolist()

        def pick(x: float, n: int) -> int:
            return min(int(x * n), n - 1)

        plan = WavePlan([], [], [], [], [], [])
        for row in u:
            plan.speed.append(pick(row[0], len(self.speeds)))
            plan.rir.append(pick(row[2], len(self.rirs)) if row[1] < self.p_reverb else -1)
            c = pick(row[4], len(self.noise)) if row[3] < self.p_noise else -1
            plan.clip.append(c)
            plan.offset.append(pick(row[5], self.noise.sizes[c]) if c >= 0 else 0)
            plan.snr_db.append(self.snr_db[0] + row[6] * (self.snr_db[1] - self.snr_db[0]))
            plan.gain_db.append(self.gain_db[0] + row[7] * (self.gain_db[1] - self.gain_db[0]))
        return plan

    def check(self, lengths: Sequence[int], Lmax: int, plan: WavePlan) -> List[int]:
        """Validate a plan against a (B, Lmax) batch (host only, raises ValueError); returns the lengths as ints."""
        if isinstance(lengths, torch.Tensor):
            if lengths.is_cuda:
                raise ValueError("lengths: expected host lengths (apply reads nothing back from the device)")
            lengths = lengths.tolist()
        lengths = [int(v) for v in lengths]
        B = len(lengths)
        if not 1 <= B <= 65535:
            raise ValueError(f"lengths: expected 1 to 65535 rows, got {B}")
        if any(not 0 <= v <= Lmax for v in lengths):
            raise ValueError(f"lengths: expected {B} lengths in [0, {Lmax}], got {lengths}")
        if not isinstance(plan, WavePlan) or any(len(f) != B for f in plan):
            raise ValueError(f"plan: expected a WavePlan of {B} rows")
        R, N = len(self.rirs) if self.rirs is not None else 0, len(self.noise) if self.noise is not None else 0
        for b in range(B):
            if not 0 <= int(plan.speed[b]) < len(self.speeds):
                raise ValueError(f"plan.speed[{b}] = {plan.speed[b]} outside [0, {len(self.speeds)})")
            if not -1 <= int(plan.rir[b]) < R:
                raise ValueError(f"plan.rir[{b}] = {plan.rir[b]} outside [-1, {R})")
            c = int(plan.clip[b])
            if not -1 <= c < N:
                raise ValueError(f"plan.clip[{b}] = {c} outside [-1, {N})")
            if not 0 <= int(plan.offset[b]) < (self.noise.sizes[c] if c >= 0 else 1):
                raise ValueError(f"plan.offset[{b}] = {plan.offset[b]} outside its clip")
            if not (math.isfinite(plan.snr_db[b]) and math.isfinite(plan.gain_db[b])):
                raise ValueError(f"plan: row {b} has a snr_db or gain_db that is not finite")
        return lengths

    def output_lengths(self, lengths: Sequence[int], plan: WavePlan) -> List[int]:
        """lengths' of a plan: ceil(den L / num) per row."""
        return [output_length(int(v), *self.geometry[s][1:]) for v, s in zip(lengths, plan.speed)]

    def output_width(self, Lmax: int, plan: WavePlan) -> int:
        """ld, the columns of wave': the longest a row of Lmax samples can become under the factors the plan uses."""
        return max(1, max(output_length(int(Lmax), *self.geometry[s][1:]) for s in set(plan.speed)))

    # ---- device ----------------------------------------------------------------------------------------------------------------
    def _resampler(self, s: int):
        if s not in self._resamplers:
            from .resample import Resampler
            self._resamplers[s] = Resampler(*self.speeds[s], device=self.device)
        return self._resamplers[s]

    @staticmethod
    def _copy_rows(x: torch.Tensor, y: torch.Tensor, W: int, rows_map: torch.Tensor) -> None:
        _lib.call("cfm3_wave_copy_rows_f32", x.data_ptr(), _pitch(x), x.shape[0], y.data_ptr(), _pitch(y), W, y.shape[0],
                  rows_map.data_ptr(), rows_map.shape[0], ops._stream())

    @torch.no_grad()
    def apply(self, wave: torch.Tensor, lengths: Sequence[int], plan: WavePlan,
              out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, List[int]]:
        """(wave' (B, ld) fp32 with zeros behind lengths'[b], lengths' as a host list).  out: a (B, ld) fp32 device tensor to
        write (unit column stride, any row pitch; ld = output_width(Lmax, plan)); nothing outside it is written."""
        if not isinstance(wave, torch.Tensor) or wave.dim() != 2:
            raise ValueError(f"wave: expected a (B, Lmax) tensor, got {tuple(getattr(wave, 'shape', ()))}")
        x = ops._req(wave, "wave")
        if x.device != self.device and not (self.device.index is None and x.device.type == self.device.type):
            raise _lib.ConformerHipError(f"wave: on {x.device}, the augmentation is on {self.device}")
        B, Lmax = x.shape
        if Lmax < 1 or Lmax >= 2 ** 30:
            raise ValueError(f"wave: {Lmax} columns, expected 1 to 2^30 - 1")
        lengths = self.check(lengths, Lmax, plan)
        if len(lengths) != B:
            raise ValueError(f"lengths: expected {B} lengths, got {len(lengths)}")
        dev = x.device
        out_lengths, ld = self.output_lengths(lengths, plan), self.output_width(Lmax, plan)
        if ld >= 2 ** 30:
            raise ValueError(f"wave: rows of {Lmax} samples become {ld}, the kernels index 2^30 - 1 at most")
        if out is not None and not (isinstance(out, torch.Tensor) and out.device == dev and out.dtype == torch.float32
                                    and out.shape == (B, ld) and out.stride(1) == 1 and _pitch(out) >= ld):
            raise ValueError(f"out: expected a ({B}, {ld}) fp32 tensor on {dev} with unit column stride")
        moved = [s for s in sorted(set(plan.speed)) if self.geometry[s][1:] != (1, 1)]
        reverb = any(r >= 0 for r in plan.rir)
        noisy = any(c >= 0 for c in plan.clip)
        mixed = [int(c >= 0 or g != 0.0) for c, g in zip(plan.clip, plan.gain_db)]

        # ---- every table in one pinned buffer: coef (B, 2) float64 | rows (B, 8) | maps and resampler tables, int32
        order = [b for s in moved for b in range(B) if plan.speed[b] == s]            # the rows to resample, grouped by factor
        stay = [b for b in range(B) if self.geometry[plan.speed[b]][1:] == (1, 1)]
        ints = np.zeros((B * ROW_COLS // 4 + 4 * len(order) + len(stay), 4), np.int32)
        rows = ints[:B * ROW_COLS // 4].reshape(B, ROW_COLS)
        rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = out_lengths, plan.rir, plan.clip, plan.offset, mixed
        at = B * ROW_COLS // 4
        for k, b in enumerate(order):
            width = self.geometry[plan.speed[b]][0]
            ints[at + k] = (b, k, lengths[b], 0)                                                  # gather: wave row b -> row k
            ints[at + len(order) + k] = (k, b, out_lengths[b], 0)                                 # scatter: row k -> row b
            ints[at + 2 * len(order) + 2 * k:at + 2 * len(order) + 2 * k + 2] = ((0, lengths[b], width, out_lengths[b]),
                                                                                 (1, 0, 0, 0))    # the resampler's table
        for k, b in enumerate(stay):
            ints[at + 4 * len(order) + k] = (b, b, lengths[b], 0)
        host = torch.empty(16 * B + ints.nbytes, dtype=torch.uint8, pin_memory=True)
        host[:16 * B].view(torch.float64).view(B, 2).numpy()[:] = [(10.0 ** (s / 10.0), 10.0 ** (g / 20.0))
                                                                   for s, g in zip(plan.snr_db, plan.gain_db)]
        host[16 * B:].view(torch.int32).numpy()[:] = ints.reshape(-1)
        table = host.to(dev, non_blocking=True)
        coef = table[:16 * B].view(torch.float64)
        tint = table[16 * B:].view(torch.int32).view(-1, 4)
        d_rows = tint[:at]
        n_o = len(order)

        def new() -> torch.Tensor:
            return torch.empty(B, ld, device=dev, dtype=torch.float32)

        cur = x
        # ---- 1. speed
        if moved:
            dst = new() if reverb or out is None else out                            # (the FIR is out of place)
            xg = torch.empty(n_o, Lmax, device=dev, dtype=torch.float32)
            self._copy_rows(x, xg, Lmax, tint[at:at + n_o])
            ld_g = max(4, (max(out_lengths[b] for b in order) + 3) // 4 * 4)
            yg = torch.empty(n_o, ld_g, device=dev, dtype=torch.float32)
            k0 = 0
            for s in moved:
                k1 = k0 + sum(1 for b in order if plan.speed[b] == s)
                rs_table = tint[at + 2 * n_o + 2 * k0:at + 2 * n_o + 2 * k1].view(-1, 8)
                self._resampler(s).launch(xg[k0:k1], 1, Lmax, None, rs_table, yg[k0:k1])
                k0 = k1
            self._copy_rows(yg, dst, ld, tint[at + n_o:at + 2 * n_o])
            if stay:
                self._copy_rows(x, dst, ld, tint[at + 4 * n_o:])
            cur = dst
        # ---- 2. reverb
        if reverb:
            taps, offsets, delays = self.rirs.on(dev)
            dst = new() if out is None else out
            _lib.call("cfm3_wave_fir_f32", cur.data_ptr(), _pitch(cur), d_rows.data_ptr(), taps.data_ptr(), offsets.data_ptr(),
                      delays.data_ptr(), len(self.rirs), taps.shape[0], self.rirs.k_max, dst.data_ptr(), _pitch(dst), ld, B,
                      ops._stream())
            cur = dst
        # ---- 3. mix
        if any(mixed):
            l_max = max(1, max(out_lengths))
            noise, clip_offsets, partial = None, None, None
            if noisy:
                noise, clip_offsets = self.noise.on(dev)
                partial = torch.empty(B * (-(-l_max // POWER_CHUNK)) * 2, device=dev, dtype=torch.float64)
                _lib.call("cfm3_wave_power_f64", cur.data_ptr(), _pitch(cur), d_rows.data_ptr(), noise.data_ptr(),
                          clip_offsets.data_ptr(), len(self.noise), noise.shape[0], l_max, partial.data_ptr(), B, ops._stream())
            dst = cur if cur is not x else (new() if out is None else out)           # in place on a buffer of our own
            _lib.call("cfm3_wave_mix_f32", cur.data_ptr(), _pitch(cur), d_rows.data_ptr(), coef.data_ptr(), ops._p(noise),
                      ops._p(clip_offsets), len(self.noise) if noisy else 0, noise.shape[0] if noisy else 0, ops._p(partial),
                      l_max, dst.data_ptr(), _pitch(dst), ld, B, ops._stream())
            cur = dst
        if cur is x:                                                                # no stage ran: the zeros behind the lengths
            cur = new() if out is None else out
            self._copy_rows(x, cur, ld, tint[at + 4 * n_o:])                        # (every row is in `stay`)
        return cur, out_lengths

    def __call__(self, wave: torch.Tensor, lengths: Sequence[int]) -> Tuple[torch.Tensor, List[int]]:
        if isinstance(lengths, torch.Tensor):
            lengths = lengths.tolist()
        return self.apply(wave, lengths, self.draw(lengths))
