"""The shared inputs of tests/test_hotword_rows_gpu.py: four utterances with the SAME peaky logits (so that any mixing of the
rows' hotword tables shows), four lists and four weights, and the float64 restatement of every row, computed once.

The logits spell   A | B | C | D | E | ÉA | THE | B | C | D   one token per frame; in one frame of every word but the last a letter
that belongs to no list leads the spelled one by AHEAD, so the unboosted search reads another word there and each list pulls back
its own words only.  SEED was chosen on the CPU: with it the restatement alone keeps every decision margin >= 1e-8 for every row,
with and without the small LM, at both beam widths."""
import functools

import numpy as np

from tests import ctc_beam_hotword_restatement as HR
from tests import ctc_beam_lm_restatement as LR
from tests import ctc_beam_restatement as R
from tests.test_ctc_beam_hotword_gpu import G_UNK, GVOCAB, PHRASES

ID = {t: i for i, t in enumerate(GVOCAB)}
L1 = ["A B", "C D E", "D"]
L2 = ["ÉA", "THE", "B C"]
DEC = ["D", "A", "ßAB"]                      # the decoder's own list: what a None entry means
assert all(" ".join(p.split()) in [" ".join(q.split()) for q in PHRASES] for p in L1 + L2 + DEC)
DEC_WEIGHT = 7.0
ENTRIES = [L1, L2, (), None]
WEIGHTS = [9.0, 5.0, 0.0, -4.0]
LISTS = [L1, L2, [], DEC]                    # what each row's search boosts
SPELL = ["A", "|", "B", "|", "C", "|", "D", "|", "E", "|", "É", "A", "|", "TH", "E", "|", "B", "|", "C", "|", "D"]
RIVAL = {0: "F", 2: "G", 4: "H", 8: "I", 11: "J", 14: "F", 16: "G", 18: "H"}     # frame -> the letter that leads there
AHEAD = 0.6
SEED = 1
BEAMS = [(16, 8), (100, 1)]                  # (beam_width, n_best)
KNOBS = dict(beam_prune_logp=-12.0)
LMKW = dict(alpha=0.5, beta=1.5)


def logits(seed: int = SEED) -> np.ndarray:
    """(T, V) fp32, T = 23: a blank frame in front and behind"""
    rng = np.random.default_rng(seed)
    frames = ["<pad>"] + SPELL + ["<pad>"]
    x = (rng.standard_normal((len(frames), len(GVOCAB))) * 0.4).astype(np.float32)
    for t, tok in enumerate(frames):
        x[t, ID[tok]] += 7.0
        if t - 1 in RIVAL:
            x[t, ID[RIVAL[t - 1]]] += 7.0 + AHEAD
    return x


def batch(seed: int = SEED) -> np.ndarray:
    return np.stack([logits(seed)] * len(ENTRIES))


def fusion(phrases, weight, ref_lm=None):
    lm = None if ref_lm is None else LR.Fusion(ref_lm, GVOCAB, skip_ids=(G_UNK,), **LMKW)
    return HR.Fusion(phrases, GVOCAB, skip_ids=(G_UNK,), weight=weight, lm=lm)


def restate(x: np.ndarray, phrases, weight, ref_lm, W: int, N: int):
    """(hyps, margins) of one utterance x (T, V) under one list"""
    return HR.restate_batch(x[None], 0, fusion(phrases, weight, ref_lm), None, beam_width=W, n_best=N, **KNOBS)[0]


@functools.lru_cache(maxsize=None)
def _restated(lm_path, W: int, N: int):
    ref_lm = None if lm_path is None else LR.Arpa.read(lm_path)
    x = logits()
    rows = [restate(x, LISTS[b], WEIGHTS[b], ref_lm, W, N) for b in range(len(LISTS))]
    plain = restate(x, [], 0.0, ref_lm, W, N)
    return rows, plain


def restated(lm_path, W: int, N: int):
    """per row (hyps, margins) under its own list and weight, and the same without hotwords; computed once per case"""
    return _restated(lm_path, W, N)


def distinct(results) -> bool:
    """the best hypotheses (tokens, score) of `results` are pairwise different in tokens or score"""
    best = [(tuple(r[0]), float(r[1])) for r in results]
    return all(a[0] != b[0] or a[1] != b[1] for i, a in enumerate(best) for b in best[i + 1:])


def lists_matter(rows, plain) -> bool:
    """The condition on the reference: every row with a non-empty list differs from the unboosted result and from every other
    row (the logits are the same, so the other rows ARE this row under their lists); the empty row is the unboosted result."""
    best = [r[0][0] for r in rows]
    return distinct([best[0], best[1], best[3], plain[0][0]]) and best[2][0] == plain[0][0][0] and best[2][1] == plain[0][0][1]


def margins_ok(rows, plain, least: float) -> bool:
    return all(R.min_margin(m) >= least for _, m in list(rows) + [plain])
