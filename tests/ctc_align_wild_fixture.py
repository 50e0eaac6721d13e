"""Shared by the wildcard alignment tests (test_ctc_align_wild_cpu / _gpu).  Test helper only: not collected by pytest.

`extended` states the definition of INTEGRATION.md "Wildcards" in numpy: the logits with w = fl32(row maximum - penalty)
appended as column V, the target with every wildcard replaced by the id V (other ids clamped to [0,V) as the device clamps
them).  The float64 restatement (tests/ctc_align_restatement.py) on that pair IS the expected path.  `reference` tabulates
the outputs from a state path: the scores over the V real columns, a wildcard frame at max_v log_softmax(x[t])[v].

`planted` is the construction the feature exists for: three words at known frames, other speech around them.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from tests import ctc_align_restatement as R

W = -2                                              # align.WILDCARD; test_ctc_align_wild_cpu pins the two together


def extended(x: np.ndarray, y: Sequence[int], penalty: float):
    """x (T,V) fp32, y the target inside its length -> (x' (T,V+1) fp32, y' list)"""
    x = np.asarray(x, dtype=np.float32)
    V = x.shape[1]
    w = x.max(axis=-1) - np.float32(penalty)                              # ONE fp32 subtraction
    assert w.dtype == np.float32
    yp = [V if int(v) == W else int(min(max(int(v), 0), V - 1)) for v in y]
    return np.concatenate([x, w[:, None]], axis=1), yp


def reference(x: np.ndarray, y: Sequence[int], blank: int, states: Optional[np.ndarray]) -> R.Result:
    """The tabulated outputs of one utterance (x (T,V) cut to its frames, y with W inside) from a state path of the extended
    lattice; None: infeasible."""
    T, V = x.shape
    if states is None:
        return R.outputs_of(x, list(y), blank, None)
    yp = [V if int(v) == W else int(min(max(int(v), 0), V - 1)) for v in y]
    sym = R.state_symbols(yp, blank)[states]
    lsm = R.log_softmax64(x)
    lp = np.where(sym == V, lsm.max(axis=-1), lsm[np.arange(T), np.minimum(sym, V - 1)])
    idx = np.where(states % 2 == 1, states // 2, -1)
    L = len(yp)
    start, end, sc = np.full(L, -1, dtype=np.int64), np.full(L, -1, dtype=np.int64), np.full(L, R.NEG)
    for i in range(L):
        fr = np.nonzero(idx == i)[0]
        start[i], end[i], sc[i] = fr[0], fr[-1] + 1, lp[fr].mean()
    return R.Result(True, states, np.where(sym == V, W, sym), idx, start, end, sc, float(lp.sum()))


def expected(x: np.ndarray, y: Sequence[int], blank: int, penalty: float, length: Optional[int] = None) -> R.Result:
    """The definition, end to end: restatement on the extended pair, outputs over the real columns."""
    n = x.shape[0] if length is None else max(0, min(x.shape[0], int(length)))
    xp, yp = extended(x[:n], y, penalty)
    return reference(np.asarray(x[:n], dtype=np.float32), y, blank, R.viterbi(xp, yp, blank))


# ---- the planted construction -----------------------------------------------------------------------------------------------

PLANT_T, PLANT_V, PLANT_BLANK = 64, 12, 0
PLANT_WORDS = ([1, 2], [3, 3, 4], [5, 6, 7])        # the second holds a repeat: a blank frame is planted between its two 3s
PLANT_PENALTY = 0.5


class Planted(NamedTuple):
    x: np.ndarray                   # (T,V) fp32 on the 1/8 grid
    spans: List[List[tuple]]        # per word, per token: (first frame, one past the last)


def planted(seed: int) -> Planted:
    """Logits on the 1/8 grid in [-2,2].  Each word's tokens stand at known frames at logit 6.0 (a token lasts 1..3 frames,
    a blank frame at 6.0 between the two tokens of a repeat); every other frame carries 5.0 on one of the symbols 8..11,
    which occur in no word: speech the transcript does not have.  With a wildcard around every word and a penalty of 0.5 a
    wildcard scores 4.5 on the other speech and 5.5 on a planted frame, every label and the blank at most 2 off their
    frames: each frame has ONE best assignment, at least 0.5 above the next."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-16, 17, size=(PLANT_T, PLANT_V)) / 8.0).astype(np.float32)
    taken = np.zeros(PLANT_T, dtype=bool)
    spans = []
    for k, word in enumerate(PLANT_WORDS):
        t = 3 + 20 * k + int(rng.integers(0, 6))
        word_spans = []
        for j, tok in enumerate(word):
            if j > 0 and word[j - 1] == tok:
                x[t, PLANT_BLANK], taken[t] = 6.0, True
                t += 1
            n = int(rng.integers(1, 4))
            x[t:t + n, tok], taken[t:t + n] = 6.0, True
            word_spans.append((t, t + n))
            t += n
        assert t <= 3 + 20 * k + 5 + 12 < 20 * (k + 1) + 3
        spans.append(word_spans)
    for t in np.nonzero(~taken)[0]:
        x[t, 8 + int(rng.integers(0, 4))] = 5.0
    return Planted(x, spans)


def planted_target(wildcards: bool) -> List[int]:
    out: List[int] = [W] if wildcards else []
    for word in PLANT_WORDS:
        out += list(word) + ([W] if wildcards else [])
    return out


def planted_token_spans(p: Planted) -> List[tuple]:
    return [s for word in p.spans for s in word]


def recovered(result: R.Result, y: Sequence[int], p: Planted) -> bool:
    """every planted token span is the span of that token in the result"""
    real = [i for i, v in enumerate(y) if v != W]
    got = [(int(result.token_start[i]), int(result.token_end[i])) for i in real]
    return got == planted_token_spans(p)
