"""Two independent statements of the beam search's token timestamps (INTEGRATION.md "Beam-search timestamps").  Test helper
only: not collected by pytest, imported by the ctc_beam_times tests.

Every token i of a live hypothesis y has (frame[i], logp[i]): the frame at which y[:i+1] entered the live set on the lineage
that survived, and log_softmax(logits[frame[i]])[y[i]].

1. `times_from_live_sets`: the lineage rule as a recurrence over the live SETS alone.  The live set after frame t is what the
   existing, unmodified restatement returns for length = t + 1 and n_best = W (`live_sets`), so this statement knows nothing of
   how a search is carried from frame to frame: it serves the plain, LM, hotword and LM + hotword searches alike.  O(T^2).
2. `TimedCommitSearch`: ctc_beam_commit_restatement.CommitSearch with `_frame` and `_commit` wrapped.  It carries one tuple of
   (frame, logp) per live hypothesis through the search itself, told apart by the canonical node ids (a hypothesis that keeps its
   node stayed; a new node appends to the tuple of the hypothesis that owns its parent node), filters the tuples as the commit
   filters the hypotheses, and logs the (token, frame, logp) of what every step committed.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests.ctc_beam_commit_restatement import CommitSearch, chunk_ends
from tests.ctc_beam_restatement import log_softmax64

Seq = Tuple[int, ...]
Times = Tuple[Tuple[int, float], ...]


def live_sets(search: Callable[..., tuple], logits: np.ndarray, length: int, W: int) -> List[List[Seq]]:
    """[L_0 .. L_{length-1}]: `search(logits, length=t + 1, n_best=W)` is the restatement with everything but those two bound
    (ctc_beam_restatement.beam_search, or the LM / hotword beam_search with its Fusion); its hypotheses' first entries are the
    token tuples.  A search keeps at most W hypotheses, so n_best = W returns the whole live set."""
    return [[tuple(h[0]) for h in search(logits, length=t + 1, n_best=W)[0]] for t in range(length)]


def times_from_live_sets(sets: Sequence[Sequence[Seq]], lp: np.ndarray) -> List[Dict[Seq, Times]]:
    """Per frame t the values of every y in L_t.  lp (T, V): the float64 log-softmax of the logits.
    Stay: y in L_{t-1} and in L_t keeps its values.  Entry (and re-entry): y in L_t, not in L_{t-1}: then y[:-1] is in L_{t-1}
    and y takes its values followed by (t, lp[t, y[-1]])."""
    prev: Dict[Seq, Times] = {(): ()}
    out = []
    for t, live in enumerate(sets):
        cur: Dict[Seq, Times] = {}
        for y in live:
            if y in prev:
                cur[y] = prev[y]
            else:
                assert len(y) > 0 and y[:-1] in prev, (t, y)
                cur[y] = prev[y[:-1]] + ((t, float(lp[t, y[-1]])),)
        out.append(cur)
        prev = cur
    return out


def reentries(sets: Sequence[Sequence[Seq]]) -> List[Tuple[int, Seq]]:
    """(t, y): y enters L_t having been live at some frame before t - 1 and not at t - 1 (pruned and found again)."""
    seen, prev, out = set(), set(), []
    for t, live in enumerate(sets):
        cur = set(live)
        out += [(t, y) for y in live if y not in prev and y in seen]
        seen |= cur
        prev = cur
    return out


def reentry_logits(T: int = 10, V: int = 7, seed: int = 0) -> np.ndarray:
    """(T, V) logits, blank 0, built for beam_width = 4, max_candidates = 4 and the default pruning: (1, 2) enters at frame 1,
    is cut at frame 2 (the stay of (1,) and its extensions by 3, 4 and 5 all outrank its stay) and enters again at frame 3,
    where token 2 dominates.  Frames 4.. are 3 * N(0, 1)."""
    x = np.full((T, V), -6.0, dtype=np.float32)
    x[0, 1], x[0, 0] = 5.0, 0.0
    x[1, 0], x[1, 2] = 3.0, 0.0
    x[2, 0], x[2, 3], x[2, 4], x[2, 5] = 3.0, 2.5, 2.3, 2.1
    x[3, 2], x[3, 0] = 5.0, 0.0
    x[4:] = (3 * np.random.default_rng(seed).normal(size=(T - 4, V))).astype(np.float32)
    return x


class TimedCommitSearch(CommitSearch):
    """CommitSearch carrying `vals[r]`, the (frame, logp) tuple of live hypothesis r over its ABSOLUTE token sequence (CommitSearch
    keeps absolute sequences), and `log_steps`: per step the list of (token, frame, logp) it committed."""

    def __init__(self, *a, **kw) -> None:
        super().__init__(*a, **kw)
        self.vals: List[Times] = [()]
        self.t = 0                             # frames consumed
        self.log_steps: List[List[Tuple[int, int, float]]] = []

    def _frame(self, row: np.ndarray) -> None:
        old = {int(n): v for n, v in zip(self.node, self.vals)}            # canonical ids: one live hypothesis per node
        lp = log_softmax64(row)
        super()._frame(row)
        vals = []
        for n, p, c in zip(self.node, self.pnode, self.last):
            if int(n) in old:                                              # stay (merged extensions included)
                vals.append(old[int(n)])
            else:                                                          # unmerged extension of the hypothesis at node p
                vals.append(old[int(p)] + ((self.t, float(lp[int(c)])),))
        self.vals = vals
        self.t += 1

    def _commit(self) -> None:
        before, y0, nodes = len(self.C), self.vals[0], [int(n) for n in self.node]
        y0_seq = self.sequence(0)
        super()._commit()
        kept = {int(n) for n in self.node}
        self.vals = [v for n, v in zip(nodes, self.vals) if n in kept]
        assert len(self.vals) == self.node.shape[0] and self.C == y0_seq[:len(self.C)]
        self.log_steps.append([(y0_seq[p], y0[p][0], y0[p][1]) for p in range(before, len(self.C))])

    def final_times(self, n_best: int = 1) -> List[Times]:
        return self.vals[:min(n_best, len(self.vals))]


def timed_commit_search(logits: np.ndarray, chunks: Sequence[int], blank: int, max_pending: Optional[int], n_best: int = 1, **kw):
    """logits (T, V) stepped in `chunks` (cycled).  Returns (final hypotheses [(absolute tokens, score)], their value tuples, the
    TimedCommitSearch)."""
    logits = np.asarray(logits)
    cs = TimedCommitSearch(blank, max_pending=max_pending, **kw)
    for a, b in chunk_ends(logits.shape[0], chunks):
        cs.step(logits[a:b])
    return cs.finish(n_best), cs.final_times(n_best), cs
