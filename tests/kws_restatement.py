"""The definition of CTC keyword spotting (conformer_amd/csrc/conformer_hip3_kws.h) in numpy float32, frame by frame and state by
state, written from the definition and not from the kernel.  The arithmetic is one max chain, one subtraction and one add per
state, so the GPU tests compare with it EXACTLY.  No torch, no library."""
import numpy as np

NEG = np.float32(-np.inf)


def row_max(row):
    """m_t: the maximum over the row with NaNs ignored; NaN when that is not finite (a BREAK)"""
    m = NEG
    for v in np.asarray(row, dtype=np.float32):
        m = np.fmax(m, v)
    return m if np.isfinite(m) else np.float32(np.nan)


class Keyword:
    """One keyword of one stream: its 2 L - 1 states (a, start), its detector and what it emitted."""

    def __init__(self, tokens, blank, threshold):
        self.tokens, self.blank, self.thr = [int(t) for t in tokens], int(blank), np.float32(threshold)
        self.n = 2 * len(self.tokens) - 1
        self.a = np.full(self.n, NEG, dtype=np.float32)
        self.start = np.zeros(self.n, dtype=np.int32)
        self.held = None                       # (start, end, score)
        self.last = (0, 0, np.float32(0.0))    # the last detection held: the state words keep it after it is dropped
        self.emitted = []

    def label(self, i):
        return self.tokens[i // 2] if i % 2 == 0 else self.blank

    def frame(self, t, row, m):
        """frame t with logits `row` and m_t = m; returns the detection it emits, or None"""
        a, start = self.a.copy(), self.start.copy()
        for i in range(self.n):
            best, frm = a[i], start[i]                                             # 1. stay
            if i >= 1 and a[i - 1] > best:                                         # 2. advance
                best, frm = a[i - 1], start[i - 1]
            if i >= 2 and i % 2 == 0 and self.tokens[i // 2] != self.tokens[i // 2 - 1] and a[i - 2] > best:   # 3. skip
                best, frm = a[i - 2], start[i - 2]
            if i == 0 and np.float32(0.0) > best:                                  # 4. a fresh start
                best, frm = np.float32(0.0), t
            if np.isnan(m):
                r = NEG
            else:
                with np.errstate(all="ignore"):
                    r = np.float32(row[self.label(i)]) - m
                if np.isnan(r):
                    r = NEG
            self.a[i], self.start[i] = np.float32(best + r), frm
        e, s = self.a[-1], int(self.start[-1])
        out = None
        if e >= self.thr:
            if self.held is not None and s > self.held[1]:
                out, self.held = self.held, None
            if self.held is None or e >= self.held[2]:
                self.held = self.last = (s, t, e)
        elif self.held is not None:
            out, self.held = self.held, None
        if out is not None:
            self.emitted.append(out)
        return out


class Stream:
    """One stream and K keywords.  keywords: token-id lists; thresholds: thr_q per keyword (<= 0).  `emissions` lists
    (keyword, start, end, score) in the order of the frames and, within a frame, of the keywords."""

    def __init__(self, keywords, blank, thresholds):
        self.kw = [Keyword(k, blank, th) for k, th in zip(keywords, thresholds)]
        self.frames = 0
        self.emissions = []
        self.rowmax = []

    def push(self, x):
        x = np.asarray(x, dtype=np.float32)
        for row in x:
            m = row_max(row)
            self.rowmax.append(m)
            for q, k in enumerate(self.kw):
                d = k.frame(self.frames, row, m)
                if d is not None:
                    self.emissions.append((q, d[0], d[1], d[2]))
            self.frames += 1
        return self

    def held(self):
        return [(q, *k.held) for q, k in enumerate(self.kw) if k.held is not None]

    def finish(self):
        """every detection, the held ones included, sorted by (end, keyword)"""
        return sorted(self.emissions + self.held(), key=lambda d: (d[2], d[0]))


def run(x, keywords, blank, thresholds, chunks=None):
    """A fresh Stream over x (T, V) cut into `chunks` (a list of lengths, None: whole)"""
    st = Stream(keywords, blank, thresholds)
    at = 0
    for n in ([len(x)] if chunks is None else chunks):
        st.push(x[at:at + n])
        at += n
    assert at == len(x)
    return st


def state_words(stream, packing, group):
    """The kernel's (8, 64) state words of `group` as int32, from the restatement's keywords: packing is the list of
    (keyword, group, first lane) the host packed."""
    out = np.zeros((8, 64), dtype=np.int32)
    out[0] = NEG.view(np.int32)
    for q, g, lane0 in packing:
        if g != group:
            continue
        k = stream.kw[q]
        out[0, lane0:lane0 + k.n] = k.a.view(np.int32)
        out[1, lane0:lane0 + k.n] = k.start
        out[2:6, lane0 + k.n - 1] = [k.held is not None, k.last[0], k.last[1], np.float32(k.last[2]).view(np.int32)]
    out[6, 0] = stream.frames
    return out


def peaky(seed, T, V, blank, plants, peak=8.0, noise=1.0):
    """CTC-like logits (T, V) float32: Gaussian noise, the blank the argmax of every frame but the planted ones.  plants: a list
    of (first frame, [symbol per frame]): on those frames the symbol (a token id, or the blank) is the argmax.  No entry is a
    zero of either sign."""
    rng = np.random.default_rng(seed)
    x = (noise * rng.standard_normal((T, V))).astype(np.float32)
    x[x == 0] = np.float32(0.25)
    top = np.full(T, blank)
    for t0, symbols in plants:
        top[t0:t0 + len(symbols)] = symbols
    x[np.arange(T), top] = np.float32(peak) + np.abs(x[np.arange(T), top])
    return x


def spell(tokens, blank, repeat=1):
    """the frames of one occurrence: every token `repeat` times, a blank between equal neighbours"""
    out = []
    for i, t in enumerate(tokens):
        if i and tokens[i - 1] == t:
            out.append(blank)
        out += [t] * repeat
    return out
