"""Float64 restatement of the CTC prefix beam search fused with a word n-gram model (`conformer_amd.decode.beam_ctc_lm_decode`,
INTEGRATION.md "Language-model fusion"), its own ARPA reader and backoff scorer, and a brute-force scorer.  Test helper only:
not collected by pytest.  It shares nothing with conformer_amd/lm.py; from tests/ctc_beam_restatement.py it takes the
log-softmax, the candidate rule and the brute-force acoustic scorer.

`beam_search` follows the written semantics with the fused score F = logaddexp(pb, pnb) + (lm + P) in place of the acoustic
score, and reports the smallest gap of every decision as tests/ctc_beam_restatement.py does (cut, prune and cand, here on F;
order: the gaps between consecutive returned hypotheses by their final F).
"""
from __future__ import annotations

import gzip
import math
from typing import Dict, List, Sequence, Tuple

import numpy as np

from tests import ctc_beam_restatement as R

NEG = -math.inf
LN10 = math.log(10.0)
SPECIAL = ("<s>", "</s>", "<unk>")


class Arpa:
    """An ARPA model as {word tuple: (log10 p, log10 backoff)}, values rounded to float32."""

    def __init__(self, text: str) -> None:
        self.table: Dict[Tuple[str, ...], Tuple[float, float]] = {}
        self.order = 0
        section = 0
        for line in text.splitlines():
            line = line.strip()
            if not line or line == "\\data\\" or line.startswith("ngram "):
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                section = int(line[1:line.index("-")])
                self.order = max(self.order, section)
                continue
            f = line.split()
            words = tuple(f[1:1 + section])
            bo = float(np.float32(f[1 + section])) if len(f) > 1 + section else 0.0
            self.table[words] = (float(np.float32(f[0])), bo)
        if ("<unk>",) not in self.table:
            self.table[("<unk>",)] = (float(np.float32(-100.0)), 0.0)
        self.unigrams = {w[0] for w in self.table if len(w) == 1}
        self.spellings = {w for w in self.unigrams if w not in SPECIAL}
        self.prefixes = {w[:i] for w in self.spellings for i in range(len(w) + 1)}

    @classmethod
    def read(cls, path: str) -> "Arpa":
        op = gzip.open if str(path).endswith(".gz") else open
        with op(path, "rt", encoding="utf-8") as f:
            return cls(f.read())

    def known(self, w: str) -> bool:
        return w in self.spellings

    def cond(self, w: str, h: Sequence[str]) -> float:
        """log10 P(w | h), standard backoff; h is cut to its last order-1 words, an unknown w is <unk>."""
        if w not in self.unigrams:
            w = "<unk>"
        h = tuple(h)[max(0, len(h) - (self.order - 1)):] if self.order > 1 else ()
        return self._cond(w, h)

    def _cond(self, w: str, h: Tuple[str, ...]) -> float:
        hit = self.table.get(h + (w,))
        if hit is not None:
            return hit[0]
        bo = self.table[h][1] if h in self.table else 0.0
        return bo + self._cond(w, h[1:])

    def sentence(self, words: Sequence[str], boundary: bool = True) -> float:
        h: List[str] = ["<s>"] if boundary else []
        total = 0.0
        for w in words:
            total += self.cond(w, h)
            h.append(w if w in self.unigrams else "<unk>")
        if boundary:
            total += self.cond("</s>", h)
        return total


class Fusion:
    """The LM state of a token sequence and its terms: (lm, partial word, context) with lm the sum of the word terms."""

    def __init__(self, lm: Arpa, vocab: Sequence[str], delim_token: str = "|", skip_ids: Sequence[int] = (),
                 alpha: float = 2.1, beta: float = 9.2, unk_score_offset: float = -10.0, score_boundary: bool = True):
        self.lm, self.vocab = lm, list(vocab)
        self.delim = {i for i, t in enumerate(vocab) if t in (delim_token, " ")}
        self.skip = set(int(i) for i in skip_ids)
        self.alpha, self.beta, self.unk = float(alpha), float(beta), float(unk_score_offset)
        self.boundary = score_boundary

    def root(self):
        return (0.0, "", ("<s>",) if self.boundary else ())

    def word_term(self, w: str, h) -> float:
        oov = not self.lm.known(w)
        return self.alpha * LN10 * (self.lm.cond(w, h) + (self.unk if oov else 0.0)) + self.beta

    def push(self, h, w: str):
        h = h + (w if self.lm.known(w) else "<unk>",)
        return h[max(0, len(h) - max(self.lm.order - 1, 0)):] if self.lm.order > 1 else ()

    def extend(self, state, c: int):
        lm, p, h = state
        if c in self.skip:
            return state
        if c in self.delim:
            if not p:
                return state
            return (lm + self.word_term(p, h), "", self.push(h, p))
        return (lm, p + self.vocab[c], h)

    def penalty(self, p: str) -> float:
        if not p or p in self.lm.prefixes:
            return 0.0
        return self.unk * max(1.0, len(p) / 6)

    def lmp(self, state) -> float:
        return state[0] + self.penalty(state[1])

    def final(self, state) -> float:
        lm, p, h = state
        if p:
            lm = lm + self.word_term(p, h)
            h = self.push(h, p)
        if self.boundary:
            lm = lm + self.alpha * LN10 * self.lm.cond("</s>", h)
        return lm

    def of_sequence(self, seq):
        st = self.root()
        for c in seq:
            st = self.extend(st, c)
        return st


def beam_search(logits: np.ndarray, blank: int, fusion: Fusion, beam_width: int, max_candidates: int = 16,
                token_min_logp: float = -5.0, beam_prune_logp: float = -10.0, n_best: int = 1, length: int | None = None):
    """logits (T,V) -> (list of (tokens tuple, fused score, acoustic score)) of at most n_best hypotheses, best first by the
    final fused score, and a dict of the smallest margins {'cut', 'prune', 'cand', 'order'}."""
    logits = np.asarray(logits)
    T, V = logits.shape
    n = T if length is None else max(0, min(T, int(length)))
    W, K = int(beam_width), int(max_candidates)
    margins = {"cut": math.inf, "prune": math.inf, "cand": math.inf, "order": math.inf}
    intern: Dict[Tuple[int, int], int] = {}
    parent, token, state = [-1], [-1], [fusion.root()]
    pb = np.array([0.0])
    pnb = np.array([NEG])
    node = np.array([0], dtype=np.int64)
    pnode = np.array([-1], dtype=np.int64)
    last = np.array([-1], dtype=np.int64)

    def child(src_node: int, c: int) -> int:
        key = (src_node, c)
        nid = intern.get(key)
        if nid is None:
            nid = intern[key] = len(parent)
            parent.append(src_node)
            token.append(c)
            state.append(fusion.extend(state[src_node], c))
        return nid

    for t in range(n):
        lp = R.log_softmax64(logits[t])
        C, cm = R.candidates(lp, blank, K, token_min_logp)
        margins["cand"] = min(margins["cand"], cm)
        H = pb.shape[0]
        s = np.logaddexp(pb, pnb)
        rank = np.arange(H)
        own = np.array([fusion.lmp(state[x]) for x in node])
        st_pb = s + lp[blank]
        st_pnb = np.where(last >= 0, pnb + lp[np.maximum(last, 0)], NEG)
        st_key = np.stack([rank, np.full(H, -1)], axis=1)
        ei = np.repeat(rank, C.shape[0])
        ec = np.tile(C, H)
        ev = np.where(ec == last[ei], pb[ei], s[ei]) + lp[ec]
        live = {(int(pnode[j]), int(last[j])): j for j in range(H) if last[j] >= 0}
        keep_e = np.ones(ei.shape[0], dtype=bool)
        for e in range(ei.shape[0]):
            j = live.get((int(node[ei[e]]), int(ec[e])))
            if j is not None:
                keep_e[e] = False
                st_pnb[j] = np.logaddexp(st_pnb[j], ev[e])
                if (ei[e], ec[e]) < tuple(st_key[j]):
                    st_key[j] = (ei[e], ec[e])
        ei, ec, ev = ei[keep_e], ec[keep_e], ev[keep_e]
        ext_nodes = [child(int(node[i]), int(c)) for i, c in zip(ei, ec)]
        ext_lmp = np.array([fusion.lmp(state[x]) for x in ext_nodes], dtype=np.float64)
        c_pb = np.concatenate([st_pb, np.full(ei.shape[0], NEG)])
        c_pnb = np.concatenate([st_pnb, ev])
        c_f = np.concatenate([np.logaddexp(st_pb, st_pnb) + own, ev + ext_lmp])
        c_k0 = np.concatenate([st_key[:, 0], ei])
        c_k1 = np.concatenate([st_key[:, 1], ec])
        c_node = np.concatenate([node, np.array(ext_nodes, dtype=np.int64)])
        c_pnode = np.concatenate([pnode, node[ei]])
        c_last = np.concatenate([last, ec])
        best = c_f.max()
        thr = best + beam_prune_logp
        if math.isfinite(thr):
            margins["prune"] = min(margins["prune"], float(np.min(np.abs(c_f - thr))))
        idx = np.nonzero(c_f >= thr)[0]
        order = idx[np.lexsort((c_k1[idx], c_k0[idx], -c_f[idx]))]
        if order.shape[0] > W:
            margins["cut"] = min(margins["cut"], float(c_f[order[W - 1]] - c_f[order[W]]))
            order = order[:W]
        pb, pnb = c_pb[order], c_pnb[order]
        node, pnode, last = c_node[order], c_pnode[order], c_last[order]
    am = np.logaddexp(pb, pnb)
    fin = np.array([am[r] + fusion.final(state[x]) for r, x in enumerate(node)])
    order = sorted(range(fin.shape[0]), key=lambda r: (-fin[r], r))
    out = []
    for r in order[:n_best]:
        seq, x = [], int(node[r])
        while x > 0:
            seq.append(token[x])
            x = parent[x]
        out.append((tuple(reversed(seq)), float(fin[r]), float(am[r])))
    for a, b in zip(order[:n_best], order[1:n_best + 1]):
        if math.isfinite(fin[b]):
            margins["order"] = min(margins["order"], float(fin[a] - fin[b]))
    return out, margins


def brute_force(logits: np.ndarray, blank: int, fusion: Fusion, length: int | None = None) -> Dict[Tuple[int, ...], float]:
    """Every prefix the alignments of the first `length` frames collapse to, scored am(y) + LM(y): the exact acoustic prefix
    probability plus every word term and the end-of-utterance terms."""
    return {seq: am + fusion.final(fusion.of_sequence(seq)) for seq, am in R.brute_force(logits, blank, length).items()}


def restate_batch(logits, blank: int, fusion: Fusion, lengths=None, **kw):
    logits = np.asarray(logits)
    return [beam_search(logits[b], blank, fusion, length=None if lengths is None else int(lengths[b]), **kw)
            for b in range(logits.shape[0])]
