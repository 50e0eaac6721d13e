"""A numpy restatement of the resampler's definition (INTEGRATION.md "Input sample rates"), independent of
conformer_amd.resample: the Hann-windowed-sinc bank and the resampled utterance in float64, the streaming rule as a small Stream
class that only copies samples (exact in any dtype) and sums the same K terms in float64, and the conversion and downmix in
float32 exactly as the contract writes them.

Rates R_in -> R_out: g = gcd, o = R_in / g, n = R_out / g, base = min(o, n) rolloff, width = ceil(lpw o / base), K = 2 width + o,
    t = clip(((m - width) / o - j / n) base, -lpw, lpw),   k[j, m] = sinc(t) cos(pi t / (2 lpw))^2 base / o
    y[i n + j] = sum_m k[j, m] x[i o - width + m]   (x = 0 outside [0, L)),   ceil(n L / o) outputs.
"""
import math

import numpy as np

TAIL_LD, TABLE_COLS = 1024, 8
LPW, ROLLOFF = 6, 0.99


def geometry(r_in, r_out, lpw=LPW, rolloff=ROLLOFF):
    """(o, n, width, K, base)"""
    g = math.gcd(r_in, r_out)
    o, n = r_in // g, r_out // g
    base = min(o, n) * rolloff
    width = int(math.ceil(lpw * o / base))
    return o, n, width, 2 * width + o, base


def kernel_f(u, o, base, lpw=LPW):
    """The continuous prototype at u input samples from its centre: f(u) = sinc(t) cos^2(pi t / (2 lpw)) base / o, t = clip(u
    base / o)."""
    t = np.clip(np.asarray(u, np.float64) * base / o, -lpw, lpw)
    return np.sinc(t) * np.cos(np.pi * t / (2 * lpw)) ** 2 * base / o


def bank(r_in, r_out, lpw=LPW, rolloff=ROLLOFF):
    """(k (n, K) float64, o, n, width)"""
    o, n, width, K, base = geometry(r_in, r_out, lpw, rolloff)
    k = np.empty((n, K), np.float64)
    for j in range(n):
        for m in range(K):
            t = min(max(((m - width) / o - j / n) * base, -lpw), lpw)
            k[j, m] = (1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)) * math.cos(math.pi * t / (2 * lpw)) ** 2 * base / o
    return k, o, n, width


def out_len(L, o, n):
    return -(-n * L // o)


def windows(xz, lead, blocks, o, K):
    """(blocks, K): row i = xz'[i o + m - lead], xz' = xz with zeros in front and behind."""
    need = (blocks - 1) * o + K if blocks else 0
    pad = np.zeros(lead + len(xz) + max(0, need - lead - len(xz)), np.float64)
    pad[lead:lead + len(xz)] = xz
    return np.lib.stride_tricks.as_strided(pad, (blocks, K), (o * pad.strides[0], pad.strides[0])) if blocks else np.zeros((0, K))


def apply_bank(k, xz, lead, count, o):
    """The first `count` outputs r = i n + j of sum_m k[j, m] xz'[i o + m - lead] and, for the rounding bound, of
    sum_m |k[j, m] xz'[.]|, both float64."""
    n, K = k.shape
    blocks = -(-count // n)
    w = windows(np.asarray(xz, np.float64), lead, blocks, o, K)
    return (w @ k.T).reshape(-1)[:count], (np.abs(w) @ np.abs(k).T).reshape(-1)[:count]


def resample64(x, k, o, width):
    """(y, sum of |terms|) of the whole utterance x: the definition."""
    return apply_bank(k, x, width, out_len(len(x), o, k.shape[0]), o)


def blocks_emitted(N, width, o):
    """Eb(N)"""
    return max(0, (N - width) // o)


class Stream:
    """One stream: step(new, flush) -> a dict with the step's outputs `y` (float64, of the samples as given), the table `row`
    the device takes for it, and the tail before (`tail_in`) and after (`tail_out`) the step, in `dtype` (copied, never
    computed with)."""

    def __init__(self, k, o, width, dtype=np.float64):
        self.k, self.o, self.n, self.width, self.dtype = k, o, k.shape[0], width, dtype
        self.tail = np.zeros(0, dtype)
        self.N = 0                      # samples received
        self.out = 0                    # outputs emitted
        self.p0 = 0                     # stream position of tail[0]

    def step(self, new, flush=False):
        o, n, width = self.o, self.n, self.width
        new = np.asarray(new, dtype=self.dtype)
        cat = np.concatenate([self.tail, new])
        N = self.N + len(new)
        assert self.p0 + len(cat) == N and self.out % n == 0
        eb0 = self.out // n
        if flush:
            total, p1 = out_len(N, o, n), N
        else:
            eb1 = blocks_emitted(N, width, o)
            total, p1 = n * eb1, max(0, eb1 * o - width)
            # every tap of every block emitted mid-stream has arrived
            assert eb1 == 0 or (eb1 - 1) * o + width + o - 1 < N
        count = total - self.out
        first = eb0 * o - width                                           # stream position of the first tap of block eb0
        assert count >= 0 and self.p0 == max(0, first), "the tail no longer holds a sample the next block needs"
        lead = max(0, -first)
        y, _ = apply_bank(self.k, cat, lead, count, o)
        tail_out = cat[p1 - self.p0:]
        assert len(tail_out) < max(1, self.k.shape[1]) or flush
        row = (len(self.tail), len(new), lead, count, int(flush), p1 - self.p0, len(tail_out), 0)
        out = dict(y=y, row=row, tail_in=self.tail, tail_out=tail_out)
        self.tail, self.N, self.out, self.p0 = tail_out, N, total, p1
        return out


def run_stream(x, chunks, flush_with_last, k, o, width, dtype=np.float64):
    """Feed x in `chunks` (they sum to len(x)); the flush comes with the last chunk or in a step of its own with no samples.
    Returns (all outputs concatenated, the steps' dicts)."""
    st, steps, t0 = Stream(k, o, width, dtype), [], 0
    for i, c in enumerate(chunks):
        steps.append(st.step(x[t0:t0 + c], flush=flush_with_last and i == len(chunks) - 1))
        t0 += c
    assert t0 == len(x)
    if not flush_with_last:
        steps.append(st.step(x[:0], flush=True))
    return np.concatenate([s["y"] for s in steps]), steps


def from_int16(v):
    """float(v) * 2^-15 in float32 (exact)."""
    return np.asarray(v, np.int16).astype(np.float32) * np.float32(2.0 ** -15)


def downmix(x):
    """(..., C) float32 -> (...): (x_0 + x_1 + ... + x_{C-1}) * fp32(1 / C), summed left to right, every step rounded to fp32."""
    x = np.asarray(x, np.float32)
    s = x[..., 0].copy()
    for c in range(1, x.shape[-1]):
        s = (s + x[..., c]).astype(np.float32)
    return (s * (np.float32(1.0) / np.float32(x.shape[-1]))).astype(np.float32)
