"""Word n-gram language model for CTC beam-search fusion ("Language-model fusion").

The reference decodes through pyctcdecode with a KenLM model built by `create_lm.py` (`lmplz -o 5 --arpa`).  This module
reads that model's ARPA text (plain or gzip) into word ids and float32 log10 values, as KenLM stores them, and packs it into
the device tables of `csrc/ngram_lm.hip` (n-gram hash tables, the character trie of the unigrams' spellings and the
vocabulary tokens' code points).  The fused search is `conformer_amd.decode.beam_ctc_lm_decode`.
"""
from __future__ import annotations

import ctypes
import gzip
import os
from typing import Dict, Iterable, List, Sequence, Tuple, Union

import numpy as np

from . import _lib

MAX_ORDER = 6
UNK_LOGP = -100.0            # log10 p(<unk>) when the file has no <unk>, as KenLM does
TOK_CHARS, TOK_DELIM, TOK_SKIP = 0, 1, 2
_KENLM_MAGIC = b"mmap lm http://kheafield.com/code"


def _open_arpa(path: str):
    with open(path, "rb") as f:
        head = f.read(64)
    if head.startswith(_KENLM_MAGIC) or path.endswith((".bin", ".klm", ".binary")):
        raise ValueError(f"{path}: a KenLM binary model; only ARPA text is supported (.arpa or .arpa.gz: write it with "
                         "`lmplz --arpa`, or convert the binary back to ARPA with KenLM's tools)")
    if head[:2] == b"\x1f\x8b":
        return gzip.open(path, "rt", encoding="utf-8")
    return open(path, "r", encoding="utf-8")


class PackedTables:
    """What NgramLanguageModel and Hotwords share: the tables `_pack` writes for a vocabulary, cached per (vocab, delimiter,
    skip ids) on the host and per device."""

    def __init__(self) -> None:
        self._packed: Dict[tuple, np.ndarray] = {}
        self._device: Dict[tuple, object] = {}

    def _pack(self, vocab: Sequence[str], delim_token: str, skip: frozenset) -> np.ndarray:
        raise NotImplementedError

    def pack(self, vocab: Sequence[str], delim_token: str = "|", skip_ids: Iterable[int] = ()) -> np.ndarray:
        """The device tables (uint8) for this vocabulary: a token equal to `delim_token` or " " is a word delimiter, tokens in
        `skip_ids` have no characters, every other token spells its code points."""
        skip = frozenset(int(i) for i in skip_ids)
        key = (tuple(vocab), delim_token, skip)
        blob = self._packed.get(key)
        if blob is None:
            blob = self._packed[key] = self._pack(vocab, delim_token, skip)
        return blob

    def device_tables(self, vocab: Sequence[str], delim_token: str = "|", skip_ids: Iterable[int] = (), device=None):
        """The packed tables as a uint8 tensor on `device`, packed and copied once per (vocab, delimiter, skip ids, device)."""
        import torch
        device = torch.device(device if device is not None else "cuda")
        skip = frozenset(int(i) for i in skip_ids)
        key = (tuple(vocab), delim_token, skip, str(device))
        t = self._device.get(key)
        if t is None:
            t = torch.from_numpy(self.pack(vocab, delim_token, skip)).to(device)
            self._device[key] = t
        return t


def token_code_points(vocab: Sequence[str], kinds: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """CSR code points of the vocabulary tokens of kind TOK_CHARS (the others spell nothing): (offsets (V+1), code points)."""
    tok_cps = [[ord(ch) for ch in t] if k == TOK_CHARS else [] for t, k in zip(vocab, kinds)]
    tok_off = np.zeros(len(vocab) + 1, dtype=np.int64)
    tok_off[1:] = np.cumsum([len(c) for c in tok_cps])
    return tok_off, np.array([c for cs in tok_cps for c in cs], dtype=np.int32)


class NgramLanguageModel(PackedTables):
    """An ARPA word n-gram model: `words[i]` is the word with id i (the order of the 1-gram section; `<unk>` appended with
    log10 p = -100 when the file has none); `ngrams[n-1] = (ids (count, n) int32, logp (count,) float32, backoff (count,)
    float32)` for n = 1..order, backoff 0 where the file gives none."""

    def __init__(self, words: List[str], ngrams: List[Tuple[np.ndarray, np.ndarray, np.ndarray]]) -> None:
        super().__init__()
        self.words = list(words)
        self.word_id: Dict[str, int] = {w: i for i, w in enumerate(self.words)}
        if len(self.word_id) != len(self.words):
            raise ValueError("duplicate words")
        self.ngrams = ngrams
        self.order = len(ngrams)
        if not 1 <= self.order <= MAX_ORDER:
            raise ValueError(f"orders 1 to {MAX_ORDER} are supported, got {self.order}")
        for name in ("<s>", "</s>", "<unk>"):
            if name not in self.word_id:
                raise ValueError(f"the model has no {name}")
        self.bos, self.eos, self.unk = self.word_id["<s>"], self.word_id["</s>"], self.word_id["<unk>"]

    @property
    def counts(self) -> List[int]:
        return [int(g[0].shape[0]) for g in self.ngrams]

    @classmethod
    def from_arpa(cls, path: Union[str, os.PathLike]) -> "NgramLanguageModel":
        """Read an .arpa or .arpa.gz file.  The \\data\\ counts must match the sections that follow, and \\end\\ must close
        the file; a malformed line raises ValueError naming it."""
        path = os.fspath(path)
        words: List[str] = []
        word_id: Dict[str, int] = {}
        declared: Dict[int, int] = {}
        grams: List[Tuple[list, list, list]] = []
        state, n, lineno = "start", 0, 0

        def fail(msg: str):
            raise ValueError(f"{path}:{lineno}: {msg}")

        with _open_arpa(path) as f:
            try:
                for lineno, raw in enumerate(f, 1):
                    line = raw.strip()
                    if state == "start":
                        if line == "\\data\\":
                            state = "data"
                        elif line:
                            fail(f"expected \\data\\, got {line[:40]!r}")
                        continue
                    if state == "end":
                        if line:
                            fail("text after \\end\\")
                        continue
                    if not line:
                        continue
                    if line == "\\end\\":
                        if state != "grams" or len(grams[-1][1]) != declared[n]:
                            fail("\\end\\ before every declared n-gram was read")
                        if len(grams) != len(declared):
                            fail(f"\\end\\ after {len(grams)} of {len(declared)} declared orders")
                        state = "end"
                        continue
                    if line.startswith("\\") and line.endswith("-grams:"):
                        try:
                            m = int(line[1:-len("-grams:")])
                        except ValueError:
                            fail(f"bad section header {line!r}")
                        if state == "data":
                            if not declared or sorted(declared) != list(range(1, len(declared) + 1)):
                                fail("the \\data\\ counts must declare orders 1..N")
                            if len(declared) > MAX_ORDER:
                                fail(f"orders 1 to {MAX_ORDER} are supported, the file declares {len(declared)}")
                        elif len(grams[-1][1]) != declared[n]:
                            fail(f"the {n}-gram section holds {len(grams[-1][1])} entries, \\data\\ declares {declared[n]}")
                        if m != n + 1 or m not in declared:
                            fail(f"unexpected section {line!r}")
                        n, state = m, "grams"
                        grams.append(([], [], []))
                        continue
                    if state == "data":
                        key, _, val = line.partition("=")
                        kw = key.split()
                        if len(kw) != 2 or kw[0] != "ngram" or not val.strip():
                            fail(f"expected 'ngram N=count', got {line[:40]!r}")
                        try:
                            order, count = int(kw[1]), int(val)
                        except ValueError:
                            fail(f"expected 'ngram N=count', got {line[:40]!r}")
                        if order < 1 or count < 0 or order in declared:
                            fail(f"bad count line {line!r}")
                        declared[order] = count
                        continue
                    # an n-gram line: log10 p, n words, optional log10 backoff
                    parts = line.split()
                    if len(parts) not in (n + 1, n + 2):
                        fail(f"expected log10 p, {n} words and an optional backoff, got {len(parts)} fields")
                    try:
                        lp = float(parts[0])
                        bo = float(parts[n + 1]) if len(parts) == n + 2 else 0.0
                    except ValueError:
                        fail("a log10 value is not a number")
                    if lp != lp or bo != bo:
                        fail("a log10 value is NaN")
                    ids, lps, bos = grams[-1]
                    if n == 1:
                        w = parts[1]
                        if w in word_id:
                            fail(f"the unigram {w!r} appears twice")
                        word_id[w] = len(words)
                        words.append(w)
                        ids.append(word_id[w])
                    else:
                        try:
                            ids.extend(word_id[w] for w in parts[1:n + 1])
                        except KeyError as e:
                            fail(f"the word {e.args[0]!r} has no unigram")
                    lps.append(lp)
                    bos.append(bo)
                    if len(lps) > declared[n]:
                        fail(f"more {n}-grams than \\data\\ declares ({declared[n]})")
            except UnicodeDecodeError as e:
                raise ValueError(f"{path}:{lineno + 1}: not UTF-8 ({e})") from None
        if state != "end":
            raise ValueError(f"{path}: no \\end\\" if state == "grams" else f"{path}: no \\data\\ section")
        ngrams = []
        for m, (ids, lps, bos) in enumerate(grams, 1):
            ngrams.append((np.asarray(ids, dtype=np.int32).reshape(-1, m), np.asarray(lps, dtype=np.float32),
                           np.asarray(bos, dtype=np.float32)))
        if "<unk>" not in word_id:
            words.append("<unk>")
            i, lp, bo = ngrams[0]
            ngrams[0] = (np.concatenate([i, np.array([[len(words) - 1]], dtype=np.int32)]),
                         np.concatenate([lp, np.array([UNK_LOGP], dtype=np.float32)]),
                         np.concatenate([bo, np.zeros(1, dtype=np.float32)]))
        return cls(words, ngrams)

    # ---- device tables
    def _pack(self, vocab: Sequence[str], delim_token: str, skip: frozenset) -> np.ndarray:
        kinds = np.array([TOK_SKIP if i in skip else TOK_DELIM if t in (delim_token, " ") else TOK_CHARS
                          for i, t in enumerate(vocab)], dtype=np.int32)
        tok_off, tok_cp = token_code_points(vocab, kinds)
        word_off = np.zeros(len(self.words) + 1, dtype=np.int64)
        word_off[1:] = np.cumsum([len(w) for w in self.words])
        word_cp = np.array([ord(ch) for w in self.words for ch in w], dtype=np.int32)
        counts = np.array(self.counts, dtype=np.int64)
        ids = np.ascontiguousarray(np.concatenate([g[0].reshape(-1) for g in self.ngrams]).astype(np.int32))
        logp = np.ascontiguousarray(np.concatenate([g[1] for g in self.ngrams]).astype(np.float32))
        backoff = np.ascontiguousarray(np.concatenate([g[2] for g in self.ngrams]).astype(np.float32))
        lib = _lib.load()
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None     # noqa: E731
        nbytes = lib.cfm_ngram_lm_pack_bytes(self.order, counts.ctypes.data_as(ctypes.c_void_p), len(self.words),
                                             int(word_off[-1]), len(vocab), int(tok_off[-1]))
        if not nbytes:
            raise ValueError("the language model or the vocabulary is out of the packer's range")
        blob = np.empty(int(nbytes), dtype=np.uint8)
        _lib.call("cfm_ngram_lm_pack", self.order, counts.ctypes.data_as(ctypes.c_void_p), p(ids), p(logp), p(backoff),
                  len(self.words), word_off.ctypes.data_as(ctypes.c_void_p), p(word_cp), self.bos, self.eos, self.unk, len(vocab),
                  tok_off.ctypes.data_as(ctypes.c_void_p), p(tok_cp), kinds.ctypes.data_as(ctypes.c_void_p),
                  blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes)
        return blob

    def score_sentences(self, sentences: Sequence[Sequence[Union[str, int]]], boundary: bool = True, device=None):
        """log10 probability of each sentence (a list of words or word ids; unknown words score as <unk>) on the device,
        fp64, with <s> / </s> when `boundary`.  The sums run in cfm_ngram_lm_score_f64."""
        import torch
        from . import ops
        tables = self.device_tables(("",), device=device)
        flat = [w if isinstance(w, (int, np.integer)) else self.word_id.get(w, -1) for s in sentences for w in s]
        off = np.zeros(len(sentences) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(s) for s in sentences])
        words = torch.tensor(flat if flat else [0], dtype=torch.int32).to(tables.device)
        offsets = torch.from_numpy(off).to(tables.device)
        out = torch.empty(len(sentences), dtype=torch.float64, device=tables.device)
        _lib.call("cfm_ngram_lm_score_f64", tables.data_ptr(), words.data_ptr(), offsets.data_ptr(), len(sentences),
                  1 if boundary else 0, out.data_ptr(), ops._stream())
        return out


def as_language_model(lm: Union[NgramLanguageModel, str, os.PathLike]) -> NgramLanguageModel:
    return lm if isinstance(lm, NgramLanguageModel) else NgramLanguageModel.from_arpa(lm)


def write_synthetic_arpa(path: Union[str, os.PathLike], tokens: Sequence[str], n_words: int, counts: Sequence[int],
                         seed: int = 0, max_tokens_per_word: int = 4) -> List[str]:
    """Write a deterministic synthetic ARPA model for tests and benchmarks: `n_words` distinct words spelled by 1 to
    `max_tokens_per_word` of `tokens`, plus <s>, </s>, <unk>; counts[n-1] n-grams of order n (counts[0] is ignored: every
    word is a unigram), each an existing (n-1)-gram extended by a random word, with random log10 probabilities and backoffs.
    Returns the words (without <s>, </s>, <unk>).  Written as gzip when the path ends in .gz."""
    rng = np.random.default_rng(seed)
    vocab: List[str] = []
    seen = set()
    while len(vocab) < n_words:
        k = int(rng.integers(1, max_tokens_per_word + 1))
        w = "".join(tokens[i] for i in rng.integers(0, len(tokens), size=k))
        if w not in seen:
            seen.add(w)
            vocab.append(w)
    words = ["<s>", "</s>", "<unk>"] + vocab
    W = len(words)
    order = len(counts)
    levels = [np.arange(W, dtype=np.int64).reshape(-1, 1)]
    for n in range(2, order + 1):
        prev, want = levels[-1], int(counts[n - 1])
        rows = np.zeros((0, n), dtype=np.int64)
        for _ in range(50):
            need = want - rows.shape[0]
            if need <= 0:
                break
            src = prev[rng.integers(0, prev.shape[0], size=2 * need + 16)]
            src = src[src[:, -1] != 1]                                    # nothing follows </s>
            nxt = rng.integers(1, W, size=(src.shape[0], 1))              # never <s> inside
            cand = np.concatenate([src, nxt], axis=1)
            rows = np.unique(np.concatenate([rows, cand]), axis=0)
        rows = rows[rng.permutation(rows.shape[0])[:want]]
        levels.append(rows[np.lexsort(rows.T[::-1])])
    lines = ["\\data\\"] + [f"ngram {n}={lv.shape[0]}" for n, lv in enumerate(levels, 1)] + [""]
    for n, lv in enumerate(levels, 1):
        lines.append(f"\\{n}-grams:")
        lp = rng.uniform(-6.0, -0.5, size=lv.shape[0])
        bo = rng.uniform(-1.5, 0.0, size=lv.shape[0])
        for r in range(lv.shape[0]):
            text = " ".join(words[i] for i in lv[r])
            if n < order:
                lines.append(f"{lp[r]:.6f}\t{text}\t{bo[r]:.6f}")
            else:
                lines.append(f"{lp[r]:.6f}\t{text}")
        lines.append("")
    lines.append("\\end\\")
    data = "\n".join(lines) + "\n"
    path = os.fspath(path)
    if path.endswith(".gz"):
        with gzip.open(path, "wt", encoding="utf-8") as f:
            f.write(data)
    else:
        with open(path, "w", encoding="utf-8") as f:
            f.write(data)
    return vocab
