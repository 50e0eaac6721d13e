"""Float64 restatement of the CTC prefix beam search of `conformer_amd.decode.beam_ctc_decode` ("CTC prefix
beam search"), plus a brute-force scorer.  Test helper only: not collected by pytest, imported by the ctc_beam tests.

`beam_search` follows the written semantics step by step; prefixes are interned in a prefix tree whose node ids are
canonical (one id per token sequence), so merging is exact.  Besides the hypotheses it reports the smallest gap between a
decision value and its threshold, over every decision the search made:
  - cut:   the score gap between the W-th kept and the best dropped hypothesis of a keep-W cut,
  - prune: the distance of any candidate score from best + beam_prune_logp,
  - cand:  the distance of any non-blank log probability from token_min_logp, and the log-probability gap at the K cap,
  - order: the gaps between consecutive returned hypotheses (and the first one not returned).
A device result computed in another floating-point order can only differ from this one where such a gap is below its
rounding error, so the tests require the gaps to be clear of it.
"""
from __future__ import annotations

import itertools
import math
from typing import Dict, List, Tuple

import numpy as np

NEG = -math.inf


def log_softmax64(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def candidates(lp: np.ndarray, blank: int, k: int, token_min_logp: float) -> Tuple[np.ndarray, float]:
    """C_t: up to k non-blank ids with the highest lp among those with lp >= token_min_logp, ties to the lower id.
    Returns (ids in order, margin)."""
    V = lp.shape[0]
    ids = np.arange(V)
    nb = ids != blank
    margin = math.inf
    if math.isfinite(token_min_logp):
        margin = float(np.min(np.abs(lp[nb] - token_min_logp)))
    ok = nb & (lp >= token_min_logp)
    sel = ids[ok]
    order = np.lexsort((sel, -lp[sel]))
    sel = sel[order]
    if sel.shape[0] > k:
        margin = min(margin, float(lp[sel[k - 1]] - lp[sel[k]]))
        sel = sel[:k]
    return sel, margin


def beam_search(logits: np.ndarray, blank: int, beam_width: int, max_candidates: int = 16, token_min_logp: float = -5.0,
                beam_prune_logp: float = -10.0, n_best: int = 1, length: int | None = None):
    """logits (T,V) -> (list of (tokens tuple, score)) of at most n_best hypotheses, best first, and a dict of the smallest
    margins {'cut', 'prune', 'cand', 'order'} (inf where that decision never arose)."""
    logits = np.asarray(logits)
    T, V = logits.shape
    n = T if length is None else max(0, min(T, int(length)))
    W, K = int(beam_width), int(max_candidates)
    margins = {"cut": math.inf, "prune": math.inf, "cand": math.inf, "order": math.inf}
    # prefix tree with canonical ids: node 0 = empty prefix
    intern: Dict[Tuple[int, int], int] = {}
    parent, token = [-1], [-1]
    # hypotheses in rank order
    pb = np.array([0.0])
    pnb = np.array([NEG])
    node = np.array([0], dtype=np.int64)
    pnode = np.array([-1], dtype=np.int64)       # id of the prefix without the last token
    last = np.array([-1], dtype=np.int64)
    for t in range(n):
        lp = log_softmax64(logits[t])
        C, cm = candidates(lp, blank, K, token_min_logp)
        margins["cand"] = min(margins["cand"], cm)
        H = pb.shape[0]
        s = np.logaddexp(pb, pnb)
        rank = np.arange(H)
        # stays
        st_pb = s + lp[blank]
        st_pnb = np.where(last >= 0, pnb + lp[np.maximum(last, 0)], NEG)
        st_key = np.stack([rank, np.full(H, -1)], axis=1)
        # extensions (i, c)
        ei = np.repeat(rank, C.shape[0])
        ec = np.tile(C, H)
        ev = np.where(ec == last[ei], pb[ei], s[ei]) + lp[ec]
        # merge: extension (i, c) is live hypothesis j iff j's prefix id is node[i] and last(j) == c (ids are canonical)
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
        # all candidates: stays first, then extensions
        c_pb = np.concatenate([st_pb, np.full(ei.shape[0], NEG)])
        c_pnb = np.concatenate([st_pnb, ev])
        c_score = np.logaddexp(c_pb, c_pnb)
        c_k0 = np.concatenate([st_key[:, 0], ei])
        c_k1 = np.concatenate([st_key[:, 1], ec])
        c_src = np.concatenate([rank, ei])
        c_tok = np.concatenate([np.full(H, -1), ec])           # -1: the stay of c_src
        best = c_score.max()
        thr = best + beam_prune_logp
        if math.isfinite(thr):
            margins["prune"] = min(margins["prune"], float(np.min(np.abs(c_score - thr))))
        ok = c_score >= thr
        idx = np.nonzero(ok)[0]
        order = idx[np.lexsort((c_k1[idx], c_k0[idx], -c_score[idx]))]
        if order.shape[0] > W:
            margins["cut"] = min(margins["cut"], float(c_score[order[W - 1]] - c_score[order[W]]))
            order = order[:W]
        new_node = np.empty(order.shape[0], dtype=np.int64)
        new_last = np.empty(order.shape[0], dtype=np.int64)
        new_pnode = np.empty(order.shape[0], dtype=np.int64)
        for r, o in enumerate(order):
            src = int(c_src[o])
            if c_tok[o] < 0:
                new_node[r], new_last[r], new_pnode[r] = node[src], last[src], pnode[src]
            else:
                key = (int(node[src]), int(c_tok[o]))
                nid = intern.get(key)
                if nid is None:
                    nid = intern[key] = len(parent)
                    parent.append(key[0])
                    token.append(key[1])
                new_node[r], new_last[r], new_pnode[r] = nid, c_tok[o], node[src]
        pb, pnb, node, last, pnode = c_pb[order], c_pnb[order], new_node, new_last, new_pnode
    scores = np.logaddexp(pb, pnb)
    out = []
    for r in range(min(n_best, scores.shape[0])):
        seq, x = [], int(node[r])
        while x > 0:
            seq.append(token[x])
            x = parent[x]
        out.append((tuple(reversed(seq)), float(scores[r])))
    for r in range(min(n_best + 1, scores.shape[0]) - 1):
        if math.isfinite(scores[r + 1]):
            margins["order"] = min(margins["order"], float(scores[r] - scores[r + 1]))
    return out, margins


def min_margin(margins: dict) -> float:
    return min(margins.values())


def collapse(path, blank: int) -> Tuple[int, ...]:
    """Standard CTC: merge repeats, then drop blanks (a blank separates repeats)."""
    out, prev = [], None
    for p in path:
        if p != prev and p != blank:
            out.append(p)
        prev = p
    return tuple(out)


def brute_force(logits: np.ndarray, blank: int, length: int | None = None) -> Dict[Tuple[int, ...], float]:
    """Every one of the V^T alignments, collapsed by the CTC rule; log of the summed probability per prefix."""
    logits = np.asarray(logits)
    T, V = logits.shape
    n = T if length is None else max(0, min(T, int(length)))
    lp = log_softmax64(logits[:n]) if n else np.zeros((0, V))
    acc: Dict[Tuple[int, ...], List[float]] = {}
    for path in itertools.product(range(V), repeat=n):
        acc.setdefault(collapse(path, blank), []).append(float(sum(lp[t, p] for t, p in enumerate(path))))
    return {k: float(np.logaddexp.reduce(np.array(v))) for k, v in acc.items()}


def restate_batch(logits, blank: int, lengths=None, **kw) -> List[Tuple[list, dict]]:
    """beam_search for every utterance of a (B,T,V) array."""
    logits = np.asarray(logits)
    return [beam_search(logits[b], blank, length=None if lengths is None else int(lengths[b]), **kw)
            for b in range(logits.shape[0])]
