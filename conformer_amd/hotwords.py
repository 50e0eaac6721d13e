"""Hotword boosting for the CTC beam search ("Hotword boosting").

The reference's `KenLanguageModel` passes a list of domain phrases and `hotword_weight` to every pyctcdecode `decode` call.
`Hotwords` normalises such a list (whitespace, duplicates, empty entries), orders it by priority (code-point length,
descending, ties in the given order) and packs it into the device tables of `csrc/hotword.hip`: a character trie over the
hotword unigrams, a word-level phrase trie, and the vocabulary tokens' code points.  The boosted search is
`conformer_amd.decode.beam_ctc_hotword_decode`.

Per-request hotwords (INTEGRATION.md "Per-request hotwords"): `HotwordRows` turns one entry per utterance (None: the decoder's
own list, a Hotwords, or phrases) and the weights into one buffer of tables, a pointer per utterance and a weight per utterance;
`reserved_bytes` is the largest table a list within given bounds can need (the region a stream reserves per utterance).
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from .lm import TOK_CHARS, TOK_DELIM, TOK_SKIP, PackedTables, token_code_points

MAX_WORDS = 8            # words per phrase
MAX_PHRASES = 1024


class Hotwords(PackedTables):
    """A hotword list: `phrases` normalised in the given order (split on whitespace and re-joined with single spaces, empty
    entries and duplicates dropped, the first kept), `priority` the same phrases by code-point length descending (stable),
    `unigrams` every word of every phrase (first seen in priority order).  Matching is by exact code points."""

    def __init__(self, phrases: Iterable[str]) -> None:
        super().__init__()
        if isinstance(phrases, (str, bytes)):
            raise ValueError("hotwords: expected a sequence of str, got a single string")
        out: List[str] = []
        seen = set()
        for i, p in enumerate(phrases):
            if not isinstance(p, str):
                raise ValueError(f"hotwords: every entry must be a str, entry {i} is {type(p).__name__}")
            words = p.split()
            if len(words) > MAX_WORDS:
                raise ValueError(f"hotwords: at most {MAX_WORDS} words per phrase, entry {i} has {len(words)}")
            norm = " ".join(words)
            if norm and norm not in seen:
                seen.add(norm)
                out.append(norm)
        if len(out) > MAX_PHRASES:
            raise ValueError(f"hotwords: at most {MAX_PHRASES} phrases, got {len(out)}")
        self.phrases: List[str] = out
        self.priority: List[str] = sorted(out, key=len, reverse=True)
        self.unigrams: List[str] = []
        uid: Dict[str, int] = {}
        self.phrase_ids: List[List[int]] = []
        for p in self.priority:
            ids = []
            for w in p.split(" "):
                if w not in uid:
                    uid[w] = len(self.unigrams)
                    self.unigrams.append(w)
                ids.append(uid[w])
            self.phrase_ids.append(ids)

    def __len__(self) -> int:
        return len(self.phrases)

    @property
    def code_points(self) -> int:
        """The characters of every word of every phrase (spaces not counted): what `reserved_bytes` bounds."""
        return sum(len(p) - p.count(" ") for p in self.phrases)

    def __repr__(self) -> str:
        return f"Hotwords({self.phrases!r})"

    @staticmethod
    def token_kinds(vocab: Sequence[str], delim_token: str = "|", skip_ids: Iterable[int] = ()) -> np.ndarray:
        """tok_kind of each token (as the LM packer assigns it); a non-delimiter token with whitespace raises ValueError"""
        skip = frozenset(int(i) for i in skip_ids)
        kinds = np.array([TOK_SKIP if i in skip else TOK_DELIM if t in (delim_token, " ") else TOK_CHARS
                          for i, t in enumerate(vocab)], dtype=np.int32)
        for i, (t, k) in enumerate(zip(vocab, kinds)):
            if k != TOK_DELIM and any(ch.isspace() for ch in t):
                raise ValueError(f"hotwords: vocabulary token {i} ({t!r}) contains whitespace but is not the delimiter")
        return kinds

    # ---- device tables
    def _pack(self, vocab: Sequence[str], delim_token: str, skip: frozenset) -> np.ndarray:
        kinds = self.token_kinds(vocab, delim_token, skip)
        tok_off, tok_cp = token_code_points(vocab, kinds)
        uni_off = np.zeros(len(self.unigrams) + 1, dtype=np.int64)
        uni_off[1:] = np.cumsum([len(w) for w in self.unigrams])
        uni_cp = np.array([ord(ch) for w in self.unigrams for ch in w], dtype=np.int32)
        ph_off = np.zeros(len(self.phrase_ids) + 1, dtype=np.int64)
        ph_off[1:] = np.cumsum([len(p) for p in self.phrase_ids])
        ph_words = np.array([i for p in self.phrase_ids for i in p], dtype=np.int32)
        lib = _lib.load()
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None     # noqa: E731
        nbytes = lib.cfm_hotword_pack_bytes(len(self.unigrams), int(uni_off[-1]), len(self.phrase_ids), int(ph_off[-1]),
                                            len(vocab), int(tok_off[-1]))
        if not nbytes:
            raise ValueError("the hotwords or the vocabulary are out of the packer's range")
        blob = np.empty(int(nbytes), dtype=np.uint8)
        _lib.call("cfm_hotword_pack", len(self.unigrams), uni_off.ctypes.data_as(ctypes.c_void_p), p(uni_cp), len(self.phrase_ids),
                  ph_off.ctypes.data_as(ctypes.c_void_p), p(ph_words), len(vocab), tok_off.ctypes.data_as(ctypes.c_void_p),
                  p(tok_cp), kinds.ctypes.data_as(ctypes.c_void_p), blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes)
        return blob

    def count(self, sequences: Sequence[Sequence[int]], vocab: Sequence[str], delim_token: str = "|",
              skip_ids: Iterable[int] = (), weight: float = 9.0) -> List[Tuple[List[int], List[float], int]]:
        """The device's window step and bonus run on the host (cfm_hotword_count) over token sequences: per sequence the
        count after each token, Q after each token, and the final count (the last partial word taken as a word)."""
        if not math.isfinite(weight):
            raise ValueError(f"hotword_weight must be finite, got {weight}")
        blob = self.pack(vocab, delim_token, skip_ids)
        flat = np.array([int(c) for s in sequences for c in s], dtype=np.int32)
        off = np.zeros(len(sequences) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(s) for s in sequences])
        counts = np.zeros(max(flat.size, 1), dtype=np.int32)
        bonus = np.zeros(max(flat.size, 1), dtype=np.float64)
        final = np.zeros(len(sequences), dtype=np.int32)
        _lib.call("cfm_hotword_count", blob.ctypes.data_as(ctypes.c_void_p),
                  flat.ctypes.data_as(ctypes.c_void_p) if flat.size else None, off.ctypes.data_as(ctypes.c_void_p), len(sequences),
                  float(weight), counts.ctypes.data_as(ctypes.c_void_p), bonus.ctypes.data_as(ctypes.c_void_p),
                  final.ctypes.data_as(ctypes.c_void_p))
        return [(counts[off[s]:off[s + 1]].tolist(), bonus[off[s]:off[s + 1]].tolist(), int(final[s]))
                for s in range(len(sequences))]


def as_hotwords(hotwords: Union[Hotwords, Iterable[str], None]) -> Optional[Hotwords]:
    """None for None or a list without phrases (after normalisation), else a Hotwords."""
    if hotwords is None:
        return None
    h = hotwords if isinstance(hotwords, Hotwords) else Hotwords(hotwords)
    return h if len(h) else None


# ---- per-request hotwords ---------------------------------------------------------------------------------------------------

ROW_ALIGN = 256          # every table of a HotwordRows buffer, and every reserved region, starts at a multiple of this


def _align(n: int) -> int:
    return (int(n) + ROW_ALIGN - 1) // ROW_ALIGN * ROW_ALIGN


def check_bounds(bounds) -> Tuple[int, int]:
    """(max_phrases, max_code_points) of a reservation, checked."""
    try:
        P, C = (int(x) for x in bounds)
    except (TypeError, ValueError):
        raise ValueError(f"hotwords: expected (max_phrases, max_code_points), got {bounds!r}") from None
    if not 0 <= P <= MAX_PHRASES or not 0 <= C < 1 << 30:
        raise ValueError(f"hotwords: (max_phrases, max_code_points) = ({P}, {C}) outside [0, {MAX_PHRASES}] x [0, 2^30)")
    return P, C


def reserved_bytes(max_phrases: int, max_code_points: int, vocab: Sequence[str], delim_token: str = "|",
                   skip_ids: Iterable[int] = ()) -> int:
    """An upper bound of len(Hotwords(L).pack(vocab, ...)) over every list L of at most max_phrases phrases whose words have at
    most max_code_points characters in all (Hotwords.code_points).  The packer's size grows with the code points of the
    distinct words and with the words of the phrases and depends on nothing else of the list, so the size at the largest of
    both is the bound: at most min(8 P, C) words, at most C code points."""
    P, C = check_bounds((max_phrases, max_code_points))
    P = min(P, C)
    n = min(MAX_WORDS * P, C)
    kinds = Hotwords.token_kinds(vocab, delim_token, skip_ids)
    tok_off, _ = token_code_points(vocab, kinds)
    nbytes = int(_lib.load().cfm_hotword_pack_bytes(n, C, P, n, len(vocab), int(tok_off[-1])))
    if not nbytes:
        raise ValueError("the hotword bounds or the vocabulary are out of the packer's range")
    return nbytes


def fits(hw: Hotwords, bounds: Tuple[int, int], who: str = "hotwords") -> None:
    """ValueError naming the limit if the list `hw` is over the reserved (max_phrases, max_code_points)."""
    P, C = bounds
    if len(hw) > P:
        raise ValueError(f"{who}: {len(hw)} phrases, the reservation is for max_phrases={P}")
    if hw.code_points > C:
        raise ValueError(f"{who}: {hw.code_points} code points, the reservation is for max_code_points={C}")


def row_weight(weight, default: float) -> float:
    """A hotword weight of one utterance (None: the decoder's own), finite."""
    w = float(default if weight is None else weight)
    if not math.isfinite(w):
        raise ValueError(f"hotword_weight must be finite, got {weight}")
    return w


class HotwordRows:
    """One hotword list and one weight per utterance, laid out for the search with per-row tables
    (csrc/conformer_hip3_hotword_rows.h).  `entries`: B entries, each None (the list `default`, the decoder's own; no list when
    that is None too), a Hotwords, or an iterable of phrases (() or []: no hotwords).  `weights`: None, one float, or B entries
    of float or None; None is `default_weight`.  A list replaces the default for its utterance, it is not merged with it.
    Every distinct list is packed once; `blob` is one uint8 array with each table at a multiple of 256 bytes, `offsets[b]` where
    utterance b's table starts, `weights` (B) float64.  `bounds`: (max_phrases, max_code_points) no list may pass.
    Lists given as phrases are packed without touching any cache; a Hotwords entry (and `default`) packs through its own."""

    def __init__(self, entries, weights, vocab: Sequence[str], delim_token: str = "|", skip_ids: Iterable[int] = (), *,
                 batch: Optional[int] = None, default: Optional[Hotwords] = None, default_weight: float = 9.0,
                 bounds: Optional[Tuple[int, int]] = None) -> None:
        if isinstance(entries, (str, bytes, Hotwords)):
            raise ValueError("hotwords: expected one entry per utterance (None, a Hotwords or a sequence of str)")
        entries = list(entries)
        B = len(entries) if batch is None else int(batch)
        if len(entries) != B:
            raise ValueError(f"hotwords: expected {B} entries, one per utterance, got {len(entries)}")
        if weights is None or isinstance(weights, (int, float)):
            weights = [weights] * B
        weights = list(weights)
        if len(weights) != B:
            raise ValueError(f"hotword_weight: expected one float or {B} of them, got {len(weights)}")
        self.weights = np.array([row_weight(w, default_weight) for w in weights], dtype=np.float64)
        if bounds is not None:
            bounds = check_bounds(bounds)
        skip = frozenset(int(i) for i in skip_ids)
        tables: Dict[tuple, np.ndarray] = {}
        keys = []
        for b, e in enumerate(entries):
            own = e is not None and not isinstance(e, Hotwords)
            hw = (default if default is not None else _EMPTY) if e is None else e if isinstance(e, Hotwords) else Hotwords(e)
            if bounds is not None:
                fits(hw, bounds, f"hotwords[{b}]")
            key = tuple(hw.phrases)
            if key not in tables:
                tables[key] = hw._pack(vocab, delim_token, skip) if own else hw.pack(vocab, delim_token, skip)
            keys.append(key)
        at, total = {}, 0
        for key, t in tables.items():
            at[key] = total
            total += _align(t.nbytes)
        self.blob = np.zeros(total, dtype=np.uint8)
        for key, t in tables.items():
            self.blob[at[key]:at[key] + t.nbytes] = t
        self.offsets = [at[k] for k in keys]
        self.distinct = len(tables)

    def __len__(self) -> int:
        return len(self.offsets)

    def to_device(self, device):
        """(buffer, pointers, weights) on `device`: the tables, the (B) int64 device pointers to each utterance's table and the
        (B) float64 weights, all three views of ONE uint8 tensor filled by one copy from pinned memory."""
        import torch
        device = torch.device(device)
        B, n = len(self.offsets), self.blob.nbytes
        buf = torch.empty(n + 16 * B, dtype=torch.uint8, device=device)
        host = torch.empty(n + 16 * B, dtype=torch.uint8, pin_memory=device.type == "cuda")
        h = host.numpy()
        h[:n] = self.blob
        h[n:n + 8 * B].view(np.int64)[:] = buf.data_ptr() + np.asarray(self.offsets, dtype=np.int64)
        h[n + 8 * B:].view(np.float64)[:] = self.weights
        buf.copy_(host, non_blocking=True)
        return buf, buf[n:n + 8 * B].view(torch.int64), buf[n + 8 * B:].view(torch.float64)


_EMPTY = Hotwords(())
