"""A numpy restatement of the waveform augmentation's definition (INTEGRATION.md "Waveform augmentation") in float64, written
from the definition and independent of conformer_amd.wave_augment; the speed stage is the resampler's own restatement
(tests/resample_restatement.py).

    bank:    d = the first index of max |h|;  normalised: h / ||h||_2
    reverb:  y[t] = sum_{k<K} h[k] x[t + d - k],  0 <= t < L,  x = 0 outside [0, L)
    mix:     n[t] = clip[(s + t) mod N_c],  Px = sum x^2,  Pn = sum n^2,  g = sqrt(Px / (Pn 10^(snr_db / 10))) if Px > 0 and
             Pn > 0 else 0,  a = 10^(gain_db / 20),  y[t] = a x[t] + a g n[t]
"""
import math

import numpy as np

from tests import resample_restatement as R


def direct_path(h):
    h = np.abs(np.asarray(h, np.float64))
    return next(i for i in range(len(h)) if h[i] == h.max())


def unit_norm(h):
    h = np.asarray(h, np.float64)
    return h / math.sqrt(float((h * h).sum()))


def reverb64(x, h, d):
    """(y, sum_k |h[k]| |x[t + d - k]|), both float64 of length len(x)."""
    x, h = np.asarray(x, np.float64), np.asarray(h, np.float64)
    L, K = len(x), len(h)
    xp = np.zeros(L + K - 1, np.float64)                    # x[j] lies at j + K - 1 - d: y[t] = sum_k h[k] xp[t + K - 1 - k]
    lo = K - 1 - d
    xp[lo:lo + L] = x
    y, mass = np.empty(L, np.float64), np.empty(L, np.float64)
    hr, step = h[::-1].copy(), max(1, (1 << 22) // K)
    for t0 in range(0, L, step):
        rows = min(step, L - t0)
        w = np.lib.stride_tricks.as_strided(xp[t0:], (rows, K), (xp.strides[0], xp.strides[0]))
        y[t0:t0 + rows] = w @ hr
        mass[t0:t0 + rows] = np.abs(w) @ np.abs(hr)
    return y, mass


def noise_of(clip, s, L):
    clip = np.asarray(clip)
    return clip[(s + np.arange(L)) % len(clip)]


def mix_terms(x, clip, s, snr_db, gain_db):
    """(a x, a g n, a, g) in float64; clip None = no noise (a g n = 0)."""
    x = np.asarray(x, np.float64)
    a = 10.0 ** (gain_db / 20.0)
    if clip is None:
        return a * x, np.zeros(len(x)), a, 0.0
    n = noise_of(clip, s, len(x)).astype(np.float64)
    px, pn = float((x * x).sum()), float((n * n).sum())
    g = math.sqrt(px / (pn * 10.0 ** (snr_db / 10.0))) if px > 0 and pn > 0 else 0.0
    return a * x, a * g * n, a, g


def mix64(x, clip, s, snr_db, gain_db):
    ax, agn, _, _ = mix_terms(x, clip, s, snr_db, gain_db)
    return ax + agn


def speed64(x, num, den):
    """(y, sum of |terms|, K) of Resampler(orig_rate=num, new_rate=den); (1, 1): x itself."""
    x = np.asarray(x, np.float64)
    if num == den:
        return x.copy(), np.abs(x), 1
    k, o, n, width = R.bank(num, den)
    y, mass = R.resample64(x, k, o, width)
    return y, mass, k.shape[1]
