"""The definition of the voice activity detector (conformer_amd/csrc/conformer_hip3_vad.h) in float64 numpy, frame by frame.
The only thing the GPU tests compare against.  No torch, no library."""
import math

import numpy as np


class Stream:
    """One stream.  push(x) takes x (n_mel, k) and returns (energies (k) float64, +inf where not finite; flags (k) bool;
    margins (k, 2): |e_t - f_t - snr| and |e_t - min_energy|, inf where the frame's energy is not finite).  words() is the
    kernel's state row, `segments` every segment closed so far, `stored` every stored energy."""

    def __init__(self, smooth, noise_window, snr, min_energy, onset, hangover, band=None):
        self.smooth, self.Wn, self.snr, self.min_energy = smooth, noise_window, float(snr), float(min_energy)
        self.onset, self.hangover, self.band = onset, hangover, band
        self.stored, self.s = [], []
        self.frames = self.run_speech = self.run_silence = self.in_speech = self.start = 0
        self.segments = []

    def push(self, x):
        x = np.asarray(x, dtype=np.float64)
        lo, hi = (0, x.shape[0]) if self.band is None else self.band
        es, flags, margins = [], [], []
        for c in range(x.shape[1]):
            t = self.frames
            with np.errstate(all="ignore"):
                col = x[lo:hi, c]
                m = np.max(col) if not np.isnan(col).any() else math.nan
                e = float(m + np.log(np.sum(np.exp(col - m))))
            finite = math.isfinite(e)
            self.stored.append(e if finite else math.inf)
            n = min(self.smooth, t + 1)
            total = 0.0
            for v in self.stored[-n:]:                       # oldest first
                total += v
            self.s.append(total / n)
            f = min(self.s[-min(self.Wn, t + 1):])
            raw = finite and (e - f >= self.snr) and (e >= self.min_energy)
            margins.append((abs(e - f - self.snr), abs(e - self.min_energy)) if finite else (math.inf, math.inf))
            if raw:
                self.run_speech, self.run_silence = self.run_speech + 1, 0
            else:
                self.run_speech, self.run_silence = 0, self.run_silence + 1
            if not self.in_speech and self.run_speech >= self.onset:
                self.in_speech, self.start = 1, t - self.run_speech + 1
            elif self.in_speech and self.run_silence >= self.hangover:
                self.segments.append((self.start, t - self.run_silence + 1))
                self.in_speech = 0
            self.frames += 1
            es.append(self.stored[-1])
            flags.append(raw)
        return np.array(es, dtype=np.float64), np.array(flags, dtype=bool), np.array(margins, dtype=np.float64).reshape(-1, 2)

    def words(self):
        """(frames, run_speech, run_silence, in_speech, start, segments closed so far)"""
        return (self.frames, self.run_speech, self.run_silence, self.in_speech, self.start, len(self.segments))

    def ring(self, initial=0.0):
        """the kernel's ring: the stored energy of frame u at u mod (noise_window + smooth - 1), `initial` where none was"""
        R = self.Wn + self.smooth - 1
        out = np.full(R, initial, dtype=np.float64)
        for u in range(max(0, self.frames - R), self.frames):
            out[u % R] = self.stored[u]
        return out

    def finish(self):
        """every segment, the open one closed at frames - run_silence"""
        return self.segments + ([(self.start, self.frames - self.run_silence)] if self.in_speech else [])


def run(x, chunks=None, **kw):
    """A fresh Stream over x (n_mel, T) cut into `chunks` (a list of lengths, None: whole): (stream, energies, flags, margins)"""
    st = Stream(**kw)
    x = np.asarray(x, dtype=np.float64)
    parts, at = [], 0
    for n in ([x.shape[1]] if chunks is None else chunks):
        parts.append(st.push(x[:, at:at + n]))
        at += n
    assert at == x.shape[1]
    return st, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])


def margin_levels(seed, n_mel, T, snr, longest=40):
    """`levels` with a pattern drawn from the seed: runs of 1 .. longest frames at noise, loud, just above snr and just below
    it.  Whether every frame keeps its margin depends on the seed and the parameters: the callers assert it."""
    rng = np.random.default_rng(seed)
    pattern, left = [], T
    while left > 0:
        n = min(left, int(rng.integers(1, longest + 1)))
        pattern.append((n, (0.0, 3.137, snr + 0.06, snr - 0.06)[int(rng.integers(0, 4))]))
        left -= n
    return levels(seed + 1, n_mel, pattern)


def levels(seed, n_mel, pattern, noise=-6.0, jitter=0.02, tilt=0.5):
    """Piecewise-level log-mel frames: `pattern` is a list of (frames, offset in nats above the noise level); every bin of a
    frame sits at noise + offset + a fixed per-bin tilt + a small jitter.  float32, as the front end emits."""
    rng = np.random.default_rng(seed)
    T = sum(n for n, _ in pattern)
    base = np.concatenate([np.zeros(0)] + [np.full(n, noise + off) for n, off in pattern])
    bins = tilt * np.sin(np.arange(n_mel) * 0.7)[:, None]
    return (base[None, :] + bins + jitter * rng.standard_normal((n_mel, T))).astype(np.float32)
