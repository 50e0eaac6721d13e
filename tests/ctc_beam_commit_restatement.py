"""Float64 restatement of the committed-prefix streaming search (INTEGRATION.md "Committed-prefix streaming (max_pending)").
Test helper only: not collected by pytest, imported by the ctc_beam_commit tests.

`CommitSearch` is the search of tests/ctc_beam_restatement.py (`beam_search`: the same per-frame rules, the same canonical prefix
tree, `candidates` and `log_softmax64` reused) run chunk by chunk, with the commit rules 1-5 after each chunk:
  lcp = longest common prefix of the live hypotheses; nb = max(lcp, |y_0| - M); y_r survives iff it starts with y_0[:nb] and
  |y_r| - nb <= M; survivors keep their order and their values; C = y_0[:nb].
It keeps absolute token sequences (C is a length into them), so nothing here shares the device's relative bookkeeping.

The margins are the ones `beam_search` reports, recomputed on THIS trajectory: after a hypothesis was dropped the search is no
longer the one-shot search, and the one-shot margins say nothing about it.  'order' also takes the gap between the two best
hypotheses at every step end, because y_0 decides what a forced commit commits.  Counters: commits that forced (nb > lcp),
commits that did not but moved C (natural), hypotheses dropped.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests.ctc_beam_restatement import NEG, candidates, log_softmax64


class CommitSearch:
    def __init__(self, blank: int, beam_width: int, max_candidates: int = 16, token_min_logp: float = -5.0,
                 beam_prune_logp: float = -10.0, max_pending: Optional[int] = None) -> None:
        self.blank, self.W, self.K = int(blank), int(beam_width), int(max_candidates)
        self.token_min_logp, self.beam_prune_logp = token_min_logp, beam_prune_logp
        self.M = None if max_pending is None else int(max_pending)
        self.margins = {"cut": math.inf, "prune": math.inf, "cand": math.inf, "order": math.inf}
        self.intern: Dict[Tuple[int, int], int] = {}
        self.parent, self.token = [-1], [-1]
        self.pb, self.pnb = np.array([0.0]), np.array([NEG])
        self.node = np.array([0], dtype=np.int64)
        self.pnode = np.array([-1], dtype=np.int64)
        self.last = np.array([-1], dtype=np.int64)
        self.C: Tuple[int, ...] = ()
        self.forced = self.natural = self.dropped = 0
        self.last_commit = 0                   # tokens the latest step committed

    # ---- one frame: beam_search's loop body on the carried state
    def _frame(self, row: np.ndarray) -> None:
        V = row.shape[0]
        W, margins = self.W, self.margins
        pb, pnb, node, pnode, last = self.pb, self.pnb, self.node, self.pnode, self.last
        lp = log_softmax64(row)
        C, cm = candidates(lp, self.blank, self.K, self.token_min_logp)
        margins["cand"] = min(margins["cand"], cm)
        H = pb.shape[0]
        s = np.logaddexp(pb, pnb)
        rank = np.arange(H)
        st_pb = s + lp[self.blank]
        st_pnb = np.where(last >= 0, pnb + lp[np.maximum(last, 0)], NEG)
        st_key = np.stack([rank, np.full(H, -1)], axis=1)
        ei = np.repeat(rank, C.shape[0])
        ec = np.tile(C, H)
        ev = np.where(ec == last[ei], pb[ei], s[ei]) + lp[ec]
        # merge: extension (i, c) is live hypothesis j iff j's prefix id is node[i] and last(j) == c (ids are canonical).  A
        # hypothesis whose whole sequence was committed keeps its node, so this holds across commits unchanged.
        js = np.nonzero(last >= 0)[0]
        jkey = pnode[js] * (V + 1) + last[js]
        ekey = node[ei] * (V + 1) + ec
        o = np.argsort(jkey)
        pos = np.minimum(np.searchsorted(jkey[o], ekey), max(js.shape[0] - 1, 0))
        merged = (js.shape[0] > 0) & (jkey[o][pos] == ekey) if js.shape[0] else np.zeros(ekey.shape[0], dtype=bool)
        for e in np.nonzero(merged)[0]:
            j = js[o[pos[e]]]
            st_pnb[j] = np.logaddexp(st_pnb[j], ev[e])
            if (ei[e], ec[e]) < tuple(st_key[j]):
                st_key[j] = (ei[e], ec[e])
        keep_e = ~merged
        ei, ec, ev = ei[keep_e], ec[keep_e], ev[keep_e]
        c_pb = np.concatenate([st_pb, np.full(ei.shape[0], NEG)])
        c_pnb = np.concatenate([st_pnb, ev])
        c_score = np.logaddexp(c_pb, c_pnb)
        c_k0 = np.concatenate([st_key[:, 0], ei])
        c_k1 = np.concatenate([st_key[:, 1], ec])
        c_src = np.concatenate([rank, ei])
        c_tok = np.concatenate([np.full(H, -1), ec])
        best = c_score.max()
        thr = best + self.beam_prune_logp
        if math.isfinite(thr):
            margins["prune"] = min(margins["prune"], float(np.min(np.abs(c_score - thr))))
        idx = np.nonzero(c_score >= thr)[0]
        order = idx[np.lexsort((c_k1[idx], c_k0[idx], -c_score[idx]))]
        if order.shape[0] > W:
            margins["cut"] = min(margins["cut"], float(c_score[order[W - 1]] - c_score[order[W]]))
            order = order[:W]
        n = order.shape[0]
        new_node, new_last, new_pnode = (np.empty(n, dtype=np.int64) for _ in range(3))
        for r, o in enumerate(order):
            src = int(c_src[o])
            if c_tok[o] < 0:
                new_node[r], new_last[r], new_pnode[r] = node[src], last[src], pnode[src]
            else:
                key = (int(node[src]), int(c_tok[o]))
                nid = self.intern.get(key)
                if nid is None:
                    nid = self.intern[key] = len(self.parent)
                    self.parent.append(key[0])
                    self.token.append(key[1])
                new_node[r], new_last[r], new_pnode[r] = nid, c_tok[o], node[src]
        self.pb, self.pnb, self.node, self.last, self.pnode = c_pb[order], c_pnb[order], new_node, new_last, new_pnode

    def sequence(self, r: int) -> Tuple[int, ...]:
        seq, x = [], int(self.node[r])
        while x > 0:
            seq.append(self.token[x])
            x = self.parent[x]
        return tuple(reversed(seq))

    def scores(self) -> np.ndarray:
        return np.logaddexp(self.pb, self.pnb)

    # ---- rules 1-5
    def _commit(self) -> None:
        ys = [self.sequence(r) for r in range(self.pb.shape[0])]
        y0 = ys[0]
        lcp = len(y0)
        for y in ys[1:]:
            k = 0
            while k < min(lcp, len(y)) and y[k] == y0[k]:
                k += 1
            lcp = k
        assert lcp >= len(self.C)
        nb = max(lcp, len(y0) - self.M)
        keep = np.array([len(y) >= nb and y[:nb] == y0[:nb] and len(y) - nb <= self.M for y in ys])
        assert keep[0]
        self.dropped += int((~keep).sum())
        if nb > lcp:
            self.forced += 1
        elif nb > len(self.C):
            self.natural += 1
        self.pb, self.pnb, self.node, self.last, self.pnode = (a[keep] for a in (self.pb, self.pnb, self.node, self.last,
                                                                                  self.pnode))
        self.last_commit = nb - len(self.C)
        self.C = y0[:nb]

    def step(self, chunk: np.ndarray) -> None:
        """chunk (k, V), k >= 1 frames: the search over them, then the commit."""
        for row in np.asarray(chunk):
            self._frame(row)
        sc = self.scores()
        if sc.shape[0] > 1 and math.isfinite(sc[1]):
            self.margins["order"] = min(self.margins["order"], float(sc[0] - sc[1]))
        if self.M is not None:
            self._commit()

    def survivors(self, n_best: Optional[int] = None) -> List[Tuple[Tuple[int, ...], float]]:
        """The live hypotheses in rank order: (tokens after C, score)."""
        sc = self.scores()
        n = sc.shape[0] if n_best is None else min(n_best, sc.shape[0])
        return [(self.sequence(r)[len(self.C):], float(sc[r])) for r in range(n)]

    def finish(self, n_best: int = 1) -> List[Tuple[Tuple[int, ...], float]]:
        """The plain search's end of utterance (the traceback): (C + pending tokens, score), best first; the 'order' margin
        takes the gaps between the returned hypotheses and the first one not returned, as beam_search does."""
        sc = self.scores()
        for r in range(min(n_best + 1, sc.shape[0]) - 1):
            if math.isfinite(sc[r + 1]):
                self.margins["order"] = min(self.margins["order"], float(sc[r] - sc[r + 1]))
        return [(self.sequence(r), float(sc[r])) for r in range(min(n_best, sc.shape[0]))]


def chunk_ends(T: int, chunks: Sequence[int]) -> List[Tuple[int, int]]:
    """(begin, end) of the steps that cover T frames with the chunk sizes `chunks`, cycled; the last one is cut at T."""
    out, t, i = [], 0, 0
    while t < T:
        k = min(chunks[i % len(chunks)], T - t)
        out.append((t, t + k))
        t += k
        i += 1
    return out


def commit_search(logits: np.ndarray, chunks: Sequence[int], blank: int, max_pending: Optional[int], n_best: int = 1, **kw):
    """logits (T, V) stepped in `chunks` (cycled).  Returns (final hypotheses as beam_search returns them, the CommitSearch:
    its C before the finish, margins and counters, and the per-step list of (C, survivors))."""
    logits = np.asarray(logits)
    cs = CommitSearch(blank, max_pending=max_pending, **kw)
    steps = []
    for a, b in chunk_ends(logits.shape[0], chunks):
        cs.step(logits[a:b])
        steps.append((cs.C, cs.survivors()))
    return cs.finish(n_best), cs, steps
