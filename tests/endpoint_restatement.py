"""Endpointing restated frame by frame in float64 (INTEGRATION.md "Endpointing").  Plain loops; shares no code with the
product."""
import numpy as np


def log_p_silence(frame, silence_ids):
    """log of the probability mass of `silence_ids` under softmax(frame), float64.  A NaN in the frame gives NaN."""
    x = np.asarray(frame, dtype=np.float64)
    with np.errstate(all="ignore"):
        m = np.max(x)                                      # (np.max keeps a NaN)
        lse = m + np.log(np.sum(np.exp(x - m)))
        return float(np.log(sum(np.exp(x[i] - lse) for i in silence_ids)))


def is_silent(frame, silence_ids, threshold):
    lp = log_p_silence(frame, silence_ids)
    return bool(lp >= np.log(np.float64(threshold)))       # False for a NaN


def new_state():
    return [0, 0, 0, -1, 0, 0, 0, 0]


def absorb(state, silent, rules):
    """One frame into one slot's state, in place.  rules: rows (min_trailing, min_frames, min_speech[, 0])."""
    state[0] += 1
    if silent:
        state[1] += 1
    else:
        state[1] = 0
        state[2] += 1
    if state[3] < 0:
        for r, rule in enumerate(rules):
            if state[1] >= rule[0] and state[0] >= rule[1] and state[2] >= rule[2]:
                state[3], state[4], state[5] = r, state[0] - 1, state[1]
                break
    return state


def run_flags(flags, rules, state=None):
    state = new_state() if state is None else state
    for f in flags:
        absorb(state, bool(f), rules)
    return state


def run_frames(frames, silence_ids, threshold, rules, state=None):
    """frames: (T, V) logits of one slot."""
    return run_flags([is_silent(x, silence_ids, threshold) for x in frames], rules, state)
