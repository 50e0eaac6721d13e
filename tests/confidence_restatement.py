"""Confidence, restated in plain numpy float64 (include/conformer_hip_confidence.h is the statement the kernels follow): the
frame measure, the lowest-index argmax, the span rule and the greedy decoder's spans.  No torch, no device."""
import math

import numpy as np

METHODS = ("max_prob", "entropy", "tsallis", "renyi")
AGGREGATIONS = ("mean", "min", "max", "prod")


def frame_confidence(x, method, alpha=None):
    """One frame of V logits -> its confidence in [0, 1] (NaN if a logit is NaN)."""
    x = np.asarray(x, dtype=np.float64)
    V = x.shape[0]
    if np.isnan(x).any():
        return math.nan
    m = x.max()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        lse = m + np.log(np.exp(x - m).sum())
        lp = x - lse
        p = np.exp(lp)
        if method == "max_prob":
            c = (V * math.exp(m - lse) - 1.0) / (V - 1.0)
        elif method == "entropy":
            terms = np.where(p == 0.0, 0.0, p * np.where(p == 0.0, 0.0, lp))        # a term with p = 0 is 0
            c = 1.0 + terms.sum() / math.log(V)
        elif method == "tsallis":
            c = 1.0 - (np.exp(alpha * lp).sum() - 1.0) / (V ** (1.0 - alpha) - 1.0)
        elif method == "renyi":
            c = 1.0 + math.log(np.exp(alpha * lp).sum()) / ((alpha - 1.0) * math.log(V))
        else:
            raise ValueError(method)
    if c < 0.0:
        c = 0.0
    if c > 1.0:
        c = 1.0
    return float(c)


def frame_id(x):
    """The lowest index that attains the maximum."""
    return int(np.argmax(np.asarray(x, dtype=np.float64)))


def frames(x, method, alpha=None):
    """(T, V) logits -> (conf (T) float64, ids (T) int64)"""
    x = np.asarray(x, dtype=np.float64)
    return (np.array([frame_confidence(r, method, alpha) for r in x], dtype=np.float64).reshape(-1),
            np.array([frame_id(r) for r in x], dtype=np.int64).reshape(-1))


def span(conf, ids, total, R, start, end, aggregation, exclude_ids=()):
    """The span [start, end) of absolute frames over a ring of R columns that has taken `total` frames (frame t at t mod R).
    NaN: an empty span (after the clamp to [0, total]), a start that has rolled out of the ring, a NaN frame in the span."""
    start, end = min(max(start, 0), total), min(max(end, 0), total)
    if end <= start or start < total - R:
        return math.nan
    c = np.array([conf[t % R] for t in range(start, end)], dtype=np.float64)
    counts = np.array([ids[t % R] not in exclude_ids for t in range(start, end)])
    if np.isnan(c).any():
        return math.nan
    if counts.any():                        # none left: all frames of the span count
        c = c[counts]
    return float({"mean": np.mean, "min": np.min, "max": np.max, "prod": np.prod}[aggregation](c))


def spans(conf, ids, total, R, starts, ends, n_spans, aggregation, exclude_ids=()):
    """One slot's row of the span entry: L values, NaN from n_spans (clamped to [0, L]) on."""
    L = len(starts)
    n = min(max(n_spans, 0), L)
    return [span(conf, ids, total, R, int(starts[j]), int(ends[j]), aggregation, exclude_ids) if j < n else math.nan
            for j in range(L)]


def greedy_spans(frame_ids, pad_id, unk_id, length=None):
    """One row of frame ids -> (token_start, token_end), both T long and padded with -1: the greedy decoder's collapse (pad and
    unk frames dropped, a token where the id differs from the previous kept one) with the frame of each emission."""
    T = len(frame_ids)
    n = T if length is None else min(max(int(length), 0), T)
    starts, prev = [], None
    for t in range(n):
        i = int(frame_ids[t])
        if i == pad_id or i == unk_id:
            continue
        if i != prev:
            starts.append(t)
        prev = i
    ends = starts[1:] + [n] if starts else []
    pad = [-1] * (T - len(starts))
    return starts + pad, ends + pad


def greedy_tokens(frame_ids, pad_id, unk_id, length=None):
    starts, _ = greedy_spans(frame_ids, pad_id, unk_id, length)
    return [int(frame_ids[t]) for t in starts if t >= 0]


def ranking_frames(seed=5, V=67, T=40):
    """The ranking fixture: (peaked, flat), each (T, V) float32: N(0, 1) logits with one logit per frame raised by 8 / by 1."""
    rng = np.random.default_rng(seed)
    out = []
    for raise_by in (8.0, 1.0):
        x = rng.standard_normal((T, V))
        x[np.arange(T), rng.integers(0, V, T)] += raise_by
        out.append(x.astype(np.float32))
    return out
