"""Float64 restatement of CTC forced alignment (`conformer_amd.align.ctc_forced_align`, INTEGRATION.md "Forced alignment"),
plus a brute-force scorer.  Test helper only: not collected by pytest, imported by the ctc_align tests.

States are s = 0..2L: an even s is blank, an odd s = 2i+1 is label y[i]; e[t,s] is the RAW logit of the state's symbol.
  v[0,0] = e[0,0]; v[0,1] = e[0,1] if L > 0; every other v[0,s] = -inf
  v[t,s] = e[t,s] + max(v[t-1,s], v[t-1,s-1], v[t-1,s-2]), the last only for odd s >= 3 with y[i] != y[i-1]
  the path ends in state 2L or (L > 0) 2L-1, whichever has the larger v[T-1,.]
Ties resolve to the smaller move (stay, advance, skip) and at the end to state 2L: of all maximum-score paths the one whose
state sequence read from the last frame backwards is lexicographically greatest.  `viterbi` is vectorised over the states
(T = 16384 runs in seconds); `brute_force` enumerates every frame labelling and applies the global rule.
"""
from __future__ import annotations

import itertools
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

NEG = -math.inf


def log_softmax64(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def repeats(y: Sequence[int]) -> int:
    return sum(1 for i in range(1, len(y)) if y[i] == y[i - 1])


def feasible(T: int, y: Sequence[int]) -> bool:
    return T > 0 and T >= len(y) + repeats(y)


def state_symbols(y: Sequence[int], blank: int) -> np.ndarray:
    sym = np.full(2 * len(y) + 1, blank, dtype=np.int64)
    sym[1::2] = np.asarray(y, dtype=np.int64)
    return sym


def viterbi(logits: np.ndarray, y: Sequence[int], blank: int, dtype=np.float64) -> Optional[np.ndarray]:
    """logits (T,V) -> the state of every frame (T,) int64, or None when infeasible.  dtype: the arithmetic of the
    recursion (float64: the restatement; float32: what an un-centred device lattice computes)."""
    x = np.asarray(logits)
    T, L = x.shape[0], len(y)
    if not feasible(T, y):
        return None
    sym = state_symbols(y, blank)
    S = 2 * L + 1
    skip = np.zeros(S, dtype=bool)
    if L > 1:
        ya = np.asarray(y)
        skip[3::2] = ya[1:] != ya[:-1]
    v = np.full(S, NEG, dtype=dtype)
    e0 = x[0, sym].astype(dtype)
    v[0] = e0[0]
    if L > 0:
        v[1] = e0[1]
    move = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        c1 = np.full(S, NEG, dtype=dtype)
        c1[1:] = v[:-1]
        c2 = np.full(S, NEG, dtype=dtype)
        c2[2:] = v[:-2]
        c2[~skip] = NEG
        best, mv = v.copy(), np.zeros(S, dtype=np.int8)
        better = c1 > best                                        # a larger move wins only when strictly greater
        best[better], mv[better] = c1[better], 1
        better = c2 > best
        best[better], mv[better] = c2[better], 2
        v = best + x[t, sym].astype(dtype)
        move[t] = mv
    s = 2 * L - 1 if L > 0 and v[2 * L - 1] > v[2 * L] else 2 * L
    states = np.empty(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        states[t] = s
        if t > 0:
            s -= int(move[t, s])
    return states


class Result(NamedTuple):
    ok: bool
    states: Optional[np.ndarray]       # (T,)
    frame_tokens: np.ndarray           # (T,) -1 when not ok
    frame_index: np.ndarray            # (T,)
    token_start: np.ndarray            # (L,)
    token_end: np.ndarray
    token_score: np.ndarray            # (L,) float64
    score: float


def outputs_of(logits: np.ndarray, y: Sequence[int], blank: int, states: Optional[np.ndarray]) -> Result:
    """The tabulated outputs of one utterance from its state sequence (None: infeasible)."""
    T, L = np.asarray(logits).shape[0], len(y)
    if states is None:
        neg1 = np.full(T, -1, dtype=np.int64)
        return Result(False, None, neg1, neg1.copy(), np.full(L, -1, dtype=np.int64), np.full(L, -1, dtype=np.int64),
                      np.full(L, NEG), NEG)
    sym = state_symbols(y, blank)
    tok = sym[states]
    idx = np.where(states % 2 == 1, states // 2, -1)
    lp = log_softmax64(logits)[np.arange(T), tok]
    start, end, sc = np.full(L, -1, dtype=np.int64), np.full(L, -1, dtype=np.int64), np.full(L, NEG)
    for i in range(L):
        fr = np.nonzero(idx == i)[0]
        start[i], end[i], sc[i] = fr[0], fr[-1] + 1, lp[fr].mean()
    return Result(True, states, tok, idx, start, end, sc, float(lp.sum()))


def align(logits: np.ndarray, y: Sequence[int], blank: int, length: Optional[int] = None) -> Result:
    x = np.asarray(logits)
    n = x.shape[0] if length is None else max(0, min(x.shape[0], int(length)))
    return outputs_of(x[:n], y, blank, viterbi(x[:n], y, blank))


def path_score(logits: np.ndarray, y: Sequence[int], blank: int, states: np.ndarray) -> float:
    """Sum of the raw logits along a state sequence, float64."""
    x = np.asarray(logits, dtype=np.float64)
    return float(x[np.arange(len(states)), state_symbols(y, blank)[states]].sum())


def valid_path(y: Sequence[int], states: np.ndarray) -> bool:
    """Starts in state 0 or 1, ends in 2L or 2L-1, moves of 0, 1 or 2, skips only into a label that differs from the last."""
    L = len(y)
    s = [int(v) for v in states]
    if not s or s[0] not in ((0, 1) if L > 0 else (0,)) or s[-1] not in ((2 * L, 2 * L - 1) if L > 0 else (0,)):
        return False
    for a, b in zip(s, s[1:]):
        d = b - a
        if d not in (0, 1, 2):
            return False
        if d == 2 and not (b % 2 == 1 and b >= 3 and y[b // 2] != y[b // 2 - 1]):
            return False
    return True


def collapse(tokens: Sequence[int], blank: int) -> List[int]:
    """Standard CTC collapse: merge repeats, then drop blanks."""
    out, prev = [], None
    for t in tokens:
        if t != prev and t != blank:
            out.append(int(t))
        prev = t
    return out


def states_of_labelling(labelling: Sequence[int], blank: int) -> Tuple[int, ...]:
    """The lattice state of every frame of a labelling: a blank after i labels is state 2i, label number i is 2i+1."""
    out, n, prev = [], 0, None
    for sym in labelling:
        if sym != blank and sym != prev:
            n += 1
        out.append(2 * n if sym == blank else 2 * n - 1)
        prev = sym
    return tuple(out)


def brute_force(logits: np.ndarray, y: Sequence[int], blank: int) -> Optional[np.ndarray]:
    """Every frame labelling over {blank} + the symbols of y that collapses to y, scored in float64; of the maximum-score
    ones the labelling whose state sequence is lexicographically greatest read from the last frame backwards.  Returns
    the states, None when no labelling collapses to y.  For T <= 6, L <= 3."""
    x = np.asarray(logits, dtype=np.float64)
    T, L = x.shape[0], len(y)
    assert T <= 6 and L <= 3
    if T == 0:
        return None
    alphabet = sorted({int(blank)} | {int(v) for v in y})
    best: Optional[Tuple[float, Tuple[int, ...]]] = None
    for lab in itertools.product(alphabet, repeat=T):
        if collapse(lab, blank) != [int(v) for v in y]:
            continue
        states = states_of_labelling(lab, blank)
        key = (float(x[np.arange(T), list(lab)].sum()), tuple(reversed(states)))
        if best is None or key > best:
            best = key
    return None if best is None else np.asarray(tuple(reversed(best[1])), dtype=np.int64)
