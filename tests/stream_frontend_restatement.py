"""A numpy restatement of the streaming audio front end's bookkeeping (INTEGRATION.md "Streaming audio front end"), independent
of conformer_amd.stream_frontend: per step it assembles the slot's segment from [tail | new samples] as the contract states it and
cuts the segment into frames.  Values are only copied, never computed with, so the results are exact in any dtype: float64
streams serve as the reference of the whole pipeline, float32 ones as the bit-exact expectation of the staging kernel.

pad = n_fft // 2.  Frame t covers virtual samples [t hop - pad, t hop - pad + n_fft) of the reflect-padded utterance; a virtual
position v < 0 is sample -v, a position v >= L (known at the flush alone) is sample 2 (L - 1) - v.
"""
import numpy as np

TAIL_LD, TABLE_COLS = 512, 8


def emitted_mid_stream(n, hop, n_fft):
    """E(n)"""
    pad = n_fft // 2
    return 0 if n <= pad else (n - pad) // hop + 1


def offline_frames(x, hop, n_fft):
    """(L // hop + 1, n_fft): the frames of the whole reflect-padded utterance x (L > pad)."""
    pad = n_fft // 2
    xp = np.pad(np.asarray(x), (pad, pad), mode="reflect")
    T = len(x) // hop + 1
    return np.stack([xp[t * hop:t * hop + n_fft] for t in range(T)])


class Stream:
    """One stream: step(new, flush) -> a dict with the step's `segment`, its `frames` (k, n_fft), the table `row` the device
    takes for it, the tail before (`tail_in`) and after (`tail_out`) the step."""

    def __init__(self, hop=160, n_fft=400, dtype=np.float64):
        self.hop, self.n_fft, self.pad, self.dtype = hop, n_fft, n_fft // 2, dtype
        self.tail = np.zeros(0, dtype)
        self.n = 0                      # samples received
        self.emitted = 0                # frames emitted
        self.p0 = 0                     # stream position of tail[0]

    def step(self, new, flush=False):
        hop, n_fft, pad = self.hop, self.n_fft, self.pad
        new = np.asarray(new, dtype=self.dtype)
        cat = np.concatenate([self.tail, new])
        p0, n = self.p0, self.n + len(new)
        assert p0 + len(cat) == n
        if flush:
            if n <= pad:
                raise ValueError(f"a stream of {n} samples is not longer than the reflect padding")
            total = n // hop + 1
        else:
            total = emitted_mid_stream(n, hop, n_fft)
        k = total - self.emitted
        assert k >= 0
        v0 = self.emitted * hop - pad                                     # virtual position of the segment's first sample
        v = v0 + np.arange((k - 1) * hop + n_fft if k > 0 else 0)
        v = np.abs(v)                                                     # the opening reflected
        if not flush:
            assert (v < n).all(), "a mid-stream frame needs a sample that has not arrived"
        v = np.where(v >= n, 2 * (n - 1) - v, v)                          # the end reflected
        c = v - p0
        assert ((c >= 0) & (c < len(cat))).all(), "a frame needs a sample the tail no longer holds"
        segment = cat[c]
        frames = np.stack([segment[t * hop:t * hop + n_fft] for t in range(k)]) if k else np.zeros((0, n_fft), self.dtype)
        p1 = n if flush else max(0, min(total * hop - pad, n - (pad + 1)))
        assert p1 >= p0
        tail_out = cat[p1 - p0:]
        row = (len(self.tail), len(new), max(0, -v0), k, int(flush), max(0, v0 - p0), p1 - p0, len(tail_out))
        out = dict(segment=segment, frames=frames, row=row, tail_in=self.tail, tail_out=tail_out)
        self.tail, self.n, self.emitted, self.p0 = tail_out, n, total, p1
        return out


def run_stream(x, chunks, flush_with_last, hop=160, n_fft=400, dtype=np.float64):
    """Feed x in `chunks` (they sum to len(x)); the flush comes with the last chunk or in a step of its own with no samples.
    Returns (all frames concatenated, the steps' dicts)."""
    st, steps, t0 = Stream(hop, n_fft, dtype), [], 0
    for i, c in enumerate(chunks):
        steps.append(st.step(x[t0:t0 + c], flush=flush_with_last and i == len(chunks) - 1))
        t0 += c
    assert t0 == len(x)
    if not flush_with_last:
        steps.append(st.step(x[:0], flush=True))
    return np.concatenate([s["frames"] for s in steps]), steps


def chunkings(L, seed, n_random=3):
    """The chunkings the contract was checked over: random draws from the sizes that matter (0, 1, around the hop, around the
    padding, a whole 64-frame step, more than everything) and, for short streams, one sample per step."""
    sizes = [0, 1, 7, 159, 160, 161, 200, 201, 640, 5000]
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_random):
        chunks, left = [], L
        while left:
            c = min(int(rng.choice(sizes)), left)
            chunks.append(c)
            left -= c
        out.append(chunks)
    if L <= 1000:
        out.append([1] * L)
    return out


def staged(steps_rows, f_max, hop, n_fft):
    """What cfm_stream_stage_f32 writes for one step of S slots: steps_rows = per slot a step dict of Stream.step, or None for
    a free slot.  Returns (xp (S * rpu * hop + n_fft,), tails (S, 512), table (S, 8) int32), float32."""
    S = len(steps_rows)
    pitch = (f_max + (n_fft + hop - 1) // hop) * hop
    xp = np.zeros(S * pitch + n_fft, np.float32)
    tails = np.zeros((S, TAIL_LD), np.float32)
    table = np.zeros((S, TABLE_COLS), np.int32)
    for b, st in enumerate(steps_rows):
        if st is None:
            continue
        seg = st["segment"]
        xp[b * pitch:b * pitch + len(seg)] = seg
        tails[b, :len(st["tail_out"])] = st["tail_out"]
        table[b] = st["row"]
    return xp, tails, table
