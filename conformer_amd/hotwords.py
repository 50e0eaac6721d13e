"""Hotword boosting for the CTC beam search ("Hotword boosting").

The reference's `KenLanguageModel` passes a list of domain phrases and `hotword_weight` to every pyctcdecode `decode` call.
`Hotwords` normalises such a list (whitespace, duplicates, empty entries), orders it by priority (code-point length,
descending, ties in the given order) and packs it into the device tables of `csrc/hotword.hip`: a character trie over the
hotword unigrams, a word-level phrase trie, and the vocabulary tokens' code points.  The boosted search is
`conformer_amd.decode.beam_ctc_hotword_decode`.
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
