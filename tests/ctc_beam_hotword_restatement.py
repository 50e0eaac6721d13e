"""Float64 restatement of the CTC prefix beam search with hotword boosting (`conformer_amd.decode.beam_ctc_hotword_decode`,
INTEGRATION.md "Hotword boosting").  Test helper only: not collected by pytest.  It shares nothing with
conformer_amd/hotwords.py: its own normalisation, and count(words) by the literal `re.findall` definition, not by the
device's window rule.  The search itself is `tests/ctc_beam_lm_restatement.beam_search` / `brute_force`, unchanged: `Fusion`
here has the `root` / `extend` / `lmp` / `final` interface of `ctc_beam_lm_restatement.Fusion` and wraps one (with the LM)
or a null model (without it).
"""
from __future__ import annotations

import re
from typing import List, Optional, Sequence

from tests import ctc_beam_lm_restatement as LR


def normalise(phrases: Sequence[str]) -> List[str]:
    """whitespace split and re-joined, empty entries and duplicates dropped (first kept), in the given order"""
    out: List[str] = []
    for p in phrases:
        n = " ".join(p.split())
        if n and n not in out:
            out.append(n)
    return out


def priority(phrases: Sequence[str]) -> List[str]:
    return sorted(normalise(phrases), key=len, reverse=True)


class Matcher:
    def __init__(self, phrases: Sequence[str]) -> None:
        self.order = priority(phrases)
        self.unigrams = {w for p in self.order for w in p.split(" ")}
        self.regex = re.compile("|".join(r"(?<!\S)" + re.escape(h) + r"(?!\S)" for h in self.order)) if self.order else None

    def count(self, words: Sequence[str]) -> int:
        if self.regex is None or not words:
            return 0
        return len(self.regex.findall(" ".join(words)))

    def is_prefix(self, p: str) -> bool:
        return bool(p) and any(u.startswith(p) for u in self.unigrams)

    def bonus(self, p: str, weight: float) -> float:
        """Q(p), 0 where p is empty or no hotword prefix"""
        if not self.is_prefix(p):
            return 0.0
        return weight * len(p) / min(len(u) for u in self.unigrams if u.startswith(p))


class NullLM:
    """the word formation of ctc_beam_lm_restatement.Fusion without a model: state (0.0, partial word, ())"""

    def __init__(self, vocab: Sequence[str], delim_token: str = "|", skip_ids: Sequence[int] = ()) -> None:
        self.vocab = list(vocab)
        self.delim = {i for i, t in enumerate(vocab) if t in (delim_token, " ")}
        self.skip = set(int(i) for i in skip_ids)

    def root(self):
        return (0.0, "", ())

    def extend(self, state, c: int):
        lm, p, h = state
        if c in self.skip:
            return state
        if c in self.delim:
            return (lm, "", h) if p else state
        return (lm, p + self.vocab[c], h)

    def final(self, state) -> float:
        return 0.0


class Fusion:
    """State (inner state, completed words, count of the completed words).  lmp = lm + weight * count + R(p), with R(p) =
    Q(p) where p is a hotword prefix and otherwise the LM's penalty (0 without an LM); final = the LM's end terms + weight *
    count(words + [p])."""

    def __init__(self, phrases: Sequence[str], vocab: Sequence[str], delim_token: str = "|", skip_ids: Sequence[int] = (),
                 weight: float = 9.0, lm: Optional[LR.Fusion] = None) -> None:
        self.m = Matcher(phrases)
        self.weight = float(weight)
        self.lm = lm
        self.inner = lm if lm is not None else NullLM(vocab, delim_token, skip_ids)

    def root(self):
        return (self.inner.root(), (), 0)

    def extend(self, state, c: int):
        inner, words, cnt = state
        nxt = self.inner.extend(inner, c)
        p = inner[1]
        if p and not nxt[1]:                                  # a delimiter completed p
            words = words + (p,)
            cnt = self.m.count(words)
        return (nxt, words, cnt)

    def r(self, p: str) -> float:
        if self.m.is_prefix(p):
            return self.m.bonus(p, self.weight)
        return self.lm.penalty(p) if self.lm is not None else 0.0

    def lmp(self, state) -> float:
        inner, _, cnt = state
        return inner[0] + self.weight * cnt + self.r(inner[1])

    def final(self, state) -> float:
        inner, words, cnt = state
        p = inner[1]
        if p:
            cnt = self.m.count(words + (p,))
        return self.inner.final(inner) + self.weight * cnt

    def of_sequence(self, seq):
        st = self.root()
        for c in seq:
            st = self.extend(st, c)
        return st

    def words(self, seq):
        st = self.of_sequence(seq)
        return list(st[1]), st[0][1]


def beam_search(logits, blank: int, fusion: Fusion, beam_width: int, **kw):
    return LR.beam_search(logits, blank, fusion, beam_width, **kw)


def brute_force(logits, blank: int, fusion: Fusion, length: Optional[int] = None):
    return LR.brute_force(logits, blank, fusion, length)


def restate_batch(logits, blank: int, fusion: Fusion, lengths=None, **kw):
    return LR.restate_batch(logits, blank, fusion, lengths, **kw)
