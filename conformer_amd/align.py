"""CTC forced alignment on the device: token and word timestamps (INTEGRATION.md "Forced alignment").

`ctc_forced_align` (T <= 16384 frames, Lmax <= 4096; `ctc_forced_align_long` beyond that) aligns known targets to logits:
the best path of the CTC lattice (the one the loss sums over), its frames, the span and mean log-probability of every
target token and the path's log-probability.  `CTCAligner` puts words
on top: texts or token ids in, `Word(text, start_frame, end_frame, start, end, score)` out; `CTCAligner.hypotheses` does
the same for what a `BeamCTCDecoder` search returned.  Timestamps of a finished stream (`StreamingTranscriber`,
`SlotTranscriber`) come from aligning the final text against the collected logits.

A transcript that skips audio takes wildcards (INTEGRATION.md "Wildcards"): a target position of value WILDCARD absorbs any
stretch of frames at `wildcard_penalty` logit units per frame below the frame's best symbol; `CTCAligner.segments` locates
utterances in a recording that holds other audio around them.

There is no CPU path: the alignment runs as gfx950 kernels (conformer_amd/csrc/ctc_align.hip)."""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence, Union

import torch

from . import _lib, ops

MAX_FRAMES = _lib.CONSTANTS["CFM_CTC_ALIGN_MAX_FRAMES"]
MAX_TARGET = _lib.CONSTANTS["CFM_CTC_ALIGN_MAX_TARGET"]
LONG_MAX_FRAMES = _lib.EXTRA_CONSTANTS["conformer_hip2_align_long.h"]["CFM2_CTC_ALIGN_LONG_MAX_FRAMES"]
LONG_MAX_TARGET = _lib.EXTRA_CONSTANTS["conformer_hip2_align_long.h"]["CFM2_CTC_ALIGN_LONG_MAX_TARGET"]
WILDCARD = _lib.OPEN_CONSTANTS["conformer_hip3_align_wild.h"]["CFM3_CTC_ALIGN_WILDCARD"]      # a target position that absorbs audio


class Alignment(NamedTuple):
    """Device tensors; B utterances, T frames, Lmax target slots.  Padding: -1 (int64), -inf (scores), False (ok)."""
    frame_tokens: torch.Tensor     # (B,T) int64: symbol emitted at each frame (blank id or a label)
    frame_index: torch.Tensor      # (B,T) int64: index into the target for label frames, -1 for blank frames
    token_start: torch.Tensor      # (B,Lmax) int64: first frame of target token i
    token_end: torch.Tensor        # (B,Lmax) int64: one past its last frame
    token_score: torch.Tensor      # (B,Lmax) fp32: mean over the run of log_softmax(x[t])[y_i]
    score: torch.Tensor            # (B,) float64: sum over the frames of the log-probability of the emitted symbol
    ok: torch.Tensor               # (B,) bool: the target fits the frames


class Word(NamedTuple):
    text: str
    start_frame: int
    end_frame: int                 # exclusive
    start: float                   # seconds
    end: float
    score: float                   # frame-weighted mean of the tokens' scores


def _checked(who: str, logits, targets, blank_id, lengths, target_lengths, max_frames: int, max_target: int):
    """The argument checks both aligners share: (x, y, lengths, target_lengths, B, T, V, L), with one unused target slot
    where there is none at all (every target length 0 then)."""
    if isinstance(logits, torch.Tensor) and logits.dtype in (torch.bfloat16, torch.float16):
        logits = logits.float()
    x = ops._req(logits, "logits")
    if x.dim() != 3:
        raise ValueError(f"logits: expected (B,T,V), got {tuple(x.shape)}")
    B, T, V = x.shape
    y = ops._req(targets, "targets", torch.int64)
    if y.dim() != 2 or y.shape[0] != B:
        raise ValueError(f"targets: expected ({B},Lmax), got {tuple(y.shape)}")
    L = int(y.shape[1])
    if not 0 <= int(blank_id) < V:
        raise ValueError(f"blank_id {blank_id} outside [0,{V})")
    if B < 1 or T < 1 or V < 2:
        raise ValueError(f"logits: empty or degenerate shape {tuple(x.shape)}")
    if T > max_frames or L > max_target:
        raise ValueError(f"{who} supports T <= {max_frames} and Lmax <= {max_target}, got T={T}, Lmax={L}")
    for name, t in (("lengths", lengths), ("target_lengths", target_lengths)):
        if t is not None and tuple(ops._req(t, name, torch.int64).shape) != (B,):
            raise ValueError(f"{name}: expected ({B},), got {tuple(t.shape)}")
    lengths = None if lengths is None else ops._req(lengths, "lengths", torch.int64)
    target_lengths = None if target_lengths is None else ops._req(target_lengths, "target_lengths", torch.int64)
    if L == 0:                                    # no target slot at all: one unused slot, every target length 0
        y = torch.zeros(B, 1, dtype=torch.int64, device=x.device)
        target_lengths = torch.zeros(B, dtype=torch.int64, device=x.device)
    return x, y, lengths, target_lengths, B, T, V, L


def _outputs(B: int, T: int, lmax: int, dev):
    return (torch.empty(B, T, dtype=torch.int64, device=dev), torch.empty(B, T, dtype=torch.int64, device=dev),
            torch.empty(B, lmax, dtype=torch.int64, device=dev), torch.empty(B, lmax, dtype=torch.int64, device=dev),
            torch.empty(B, lmax, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float64, device=dev),
            torch.empty(B, dtype=torch.bool, device=dev))


def _penalty(who: str, wildcard_penalty) -> float:
    """wildcard_penalty as the C entries take it: a finite float32 >= 0"""
    if isinstance(wildcard_penalty, bool) or not isinstance(wildcard_penalty, (int, float)) or \
            not 0.0 <= float(wildcard_penalty) < math.inf or float(wildcard_penalty) > 3.4028234e38:
        raise ValueError(f"{who}: wildcard_penalty must be a finite number >= 0 (logit units per wildcard frame), got "
                         f"{wildcard_penalty!r}")
    return float(wildcard_penalty)


def ctc_forced_align(logits: torch.Tensor, targets: torch.Tensor, blank_id: int, lengths: Optional[torch.Tensor] = None,
                     target_lengths: Optional[torch.Tensor] = None, *, wildcard_penalty: Optional[float] = None) -> Alignment:
    """Align targets (B,Lmax) int64 (padded, as the CTC loss takes them) to logits (B,T,V) on the HIP device (fp32, or
    bf16 / fp16 cast to fp32).  `lengths` / `target_lengths` (B) int64 on the device: frames / labels per utterance
    (clamped to [0,T] / [0,Lmax]; None = all).  The path is the maximum of the sum of raw logits over the lattice's paths,
    ties resolved to the latest alignment.  An utterance with no frames, or fewer frames than labels plus adjacent
    repeats, is not an error: ok False, score -inf, padding elsewhere.

    Target ids are clamped to [0,V) on the device, as the loss does (checking them would synchronise with the host); a
    target equal to `blank_id` is not detected here and is aligned as a label that emits the blank symbol.  CTCAligner,
    which builds the targets on the host, refuses both.  Logits are expected to be finite.  Nothing synchronises with
    the host.

    wildcard_penalty (INTEGRATION.md "Wildcards"): None: as ever, a target value of WILDCARD is clamped like any id.  A
    float >= 0: a target position inside target_lengths that holds WILDCARD (-2) may absorb any stretch of one or more
    frames; at each it scores the row's largest logit minus the penalty.  frame_tokens is WILDCARD there, token_score /
    score take max_v log_softmax(x[t])[v].  A target without a wildcard gives the outputs of None, bit for bit."""
    x, y, lengths, target_lengths, B, T, V, L = _checked("ctc_forced_align", logits, targets, blank_id, lengths,
                                                         target_lengths, MAX_FRAMES, MAX_TARGET)
    wild = () if wildcard_penalty is None else (_penalty("ctc_forced_align", wildcard_penalty),)
    lmax = max(L, 1)
    lib = _lib.load()
    ws_bytes = int((lib.cfm3_ctc_align_wild_workspace_bytes if wild else lib.cfm_ctc_align_workspace_bytes)(B, T, lmax))
    if ws_bytes == 0:
        raise ValueError(f"ctc_forced_align: unsupported shape (B={B}, T={T}, Lmax={L})")
    workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    frame_tokens, frame_index, token_start, token_end, token_score, score, ok = _outputs(B, T, lmax, x.device)
    _lib.call("cfm3_ctc_align_wild_f32" if wild else "cfm_ctc_align_f32", x.data_ptr(), y.data_ptr(), ops._p(lengths),
              ops._p(target_lengths), B, T, V, lmax, int(blank_id), *wild, workspace.data_ptr(), ws_bytes,
              frame_tokens.data_ptr(), frame_index.data_ptr(),
              token_start.data_ptr(), token_end.data_ptr(), token_score.data_ptr(), score.data_ptr(), ok.data_ptr(), ops._stream())
    return Alignment(frame_tokens, frame_index, token_start[:, :L], token_end[:, :L], token_score[:, :L], score, ok)


def long_workspace_bytes(B: int, T: int, Lmax: int, tile_pairs: Optional[int] = None, chunk_frames: Optional[int] = None,
                         max_workspace_bytes: int = 16 << 30, *, wildcard_penalty: Optional[float] = None) -> int:
    """Bytes of device workspace ctc_forced_align_long takes for a shape (host arithmetic of the library, no device needed).
    ValueError for a tiling or shape it does not support and for one that needs more than `max_workspace_bytes`.
    wildcard_penalty other than None: the workspace of the wildcard entry (B * T floats more)."""
    tp, cf = (0 if v is None else int(v) for v in (tile_pairs, chunk_frames))
    if (tile_pairs is not None and not (512 <= tp <= 8192 and tp % 512 == 0)) or \
            (chunk_frames is not None and not (16 <= cf <= 65536 and cf % 16 == 0)):
        raise ValueError(f"ctc_forced_align_long: tile_pairs must be a multiple of 512 in [512,8192] and chunk_frames a "
                         f"multiple of 16 in [16,65536] (or None), got {tile_pairs!r}, {chunk_frames!r}")
    lib = _lib.load()
    if wildcard_penalty is not None:
        _penalty("ctc_forced_align_long", wildcard_penalty)
    sizer = lib.cfm2_ctc_align_long_workspace_bytes if wildcard_penalty is None else lib.cfm3_ctc_align_long_wild_workspace_bytes
    ws_bytes = int(sizer(int(B), int(T), int(Lmax), tp, cf))
    if ws_bytes == 0:
        raise ValueError(f"ctc_forced_align_long: unsupported shape (B={B}, T={T}, Lmax={Lmax})")
    if ws_bytes > int(max_workspace_bytes):
        raise ValueError(f"ctc_forced_align_long: (B={B}, T={T}, Lmax={Lmax}) needs a workspace of {ws_bytes} bytes, "
                         f"max_workspace_bytes is {int(max_workspace_bytes)}")
    return ws_bytes


def ctc_forced_align_long(logits: torch.Tensor, targets: torch.Tensor, blank_id: int, lengths: Optional[torch.Tensor] = None,
                          target_lengths: Optional[torch.Tensor] = None, *, tile_pairs: Optional[int] = None,
                          chunk_frames: Optional[int] = None, max_workspace_bytes: int = 16 << 30,
                          wildcard_penalty: Optional[float] = None) -> Alignment:
    """ctc_forced_align without its limits (INTEGRATION.md "Long form"): T <= LONG_MAX_FRAMES, Lmax <= LONG_MAX_TARGET, the
    same arguments, the same Alignment (dtypes, padding, infeasible rows).  The lattice is cut into cells of `tile_pairs`
    target positions (a multiple of 512 in [512,8192]) x `chunk_frames` frames (a multiple of 16 in [16,65536]); None: the
    measured defaults.  The tiling changes the time, never the result.  The recursion runs in float64 without re-centring,
    so for any finite logits the path is that of the float64 recursion on the raw logits, ties included.

    The workspace is dominated by the moves: B * T * ceil((Lmax+1)/tile_pairs) * tile_pairs / 2 bytes (1.4 GB for an hour
    of audio with 30 000 tokens).  A shape that needs more than `max_workspace_bytes` raises ValueError with the number of
    bytes it needs.  Nothing synchronises with the host.

    wildcard_penalty: as ctc_forced_align takes it; a wildcard's emission enters the float64 recursion as (double) of the
    fp32 value max - penalty, so the path is exact with wildcards too."""
    x, y, lengths, target_lengths, B, T, V, L = _checked("ctc_forced_align_long", logits, targets, blank_id, lengths,
                                                         target_lengths, LONG_MAX_FRAMES, LONG_MAX_TARGET)
    wild = () if wildcard_penalty is None else (_penalty("ctc_forced_align_long", wildcard_penalty),)
    lmax = max(L, 1)
    ws_bytes = long_workspace_bytes(B, T, lmax, tile_pairs, chunk_frames, max_workspace_bytes, wildcard_penalty=wildcard_penalty)
    tp, cf = int(tile_pairs or 0), int(chunk_frames or 0)
    workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    frame_tokens, frame_index, token_start, token_end, token_score, score, ok = _outputs(B, T, lmax, x.device)
    _lib.call("cfm3_ctc_align_long_wild_f32" if wild else "cfm2_ctc_align_long_f32", x.data_ptr(), y.data_ptr(),
              ops._p(lengths), ops._p(target_lengths), B, T, V, lmax, int(blank_id), *wild, tp, cf, workspace.data_ptr(), ws_bytes, frame_tokens.data_ptr(), frame_index.data_ptr(),
              token_start.data_ptr(), token_end.data_ptr(), token_score.data_ptr(), score.data_ptr(), ok.data_ptr(), ops._stream())
    return Alignment(frame_tokens, frame_index, token_start[:, :L], token_end[:, :L], token_score[:, :L], score, ok)


class Segment(NamedTuple):
    """One utterance located in a recording (CTCAligner.segments): `index` into the utterances given, its text, its frames
    [start_frame, end_frame) and seconds, the mean of its tokens' scores weighted by their frames, and its Words."""
    index: int
    text: str
    start_frame: int
    end_frame: int                 # exclusive
    start: float                   # seconds
    end: float
    score: float
    words: List[Word]


def group_words(ids: Sequence[int], starts: Sequence[int], ends: Sequence[int], scores: Sequence[float],
                vocab: Sequence[str], delim_id: Optional[int], frame_seconds: float, skip_ids=frozenset(),
                wildcard: Optional[int] = None) -> List[Word]:
    """Words are the runs of tokens between delimiter tokens (delimiters at the ends and doubled delimiters make no empty
    word).  A word spans the first start to the last end of its tokens; its score is the mean of its tokens' scores
    weighted by their frames.  Tokens in `skip_ids` take part in the span and the score but add no characters.
    `wildcard`: a token of this value (WILDCARD) closes the open word as a delimiter does and belongs to no word."""
    words: List[Word] = []
    text, first, last, acc, frames = [], -1, -1, 0.0, 0

    def close():
        nonlocal text, first, last, acc, frames
        if frames > 0 and text:
            words.append(Word("".join(text), first, last, first * frame_seconds, last * frame_seconds, acc / frames))
        text, first, last, acc, frames = [], -1, -1, 0.0, 0

    for tok, s, e, sc in zip(ids, starts, ends, scores):
        if (delim_id is not None and tok == delim_id) or (wildcard is not None and tok == wildcard):
            close()
            continue
        if tok not in skip_ids:
            text.append(vocab[tok])
        first = s if frames == 0 else first
        last = e
        acc += sc * (e - s)
        frames += e - s
    close()
    return words


class CTCAligner:
    """Word timestamps from a known transcript: `aligner(logits, texts_or_token_ids, lengths=None)` returns per utterance
    a list of Word.  `vocab` (V strings) spells the tokens, `delim_token` separates words, `blank_id` is the CTC blank.

    `frame_seconds` converts frames to seconds.  The default 0.04 is the encoder's subsampling of 4 times the front end's
    hop of 160 samples at 16 kHz.  Encoder frame t' is computed from the mel frames 4t' .. 4t'+6 (two 3-tap stride-2
    convolutions), so a word's `start` is the time of the first mel frame its first encoder frame sees.

    A text is tokenised greedily, longest vocabulary token first, with a space read as `delim_token`; token-id sequences
    are taken as they are.  An id outside [0,V), the blank id, or a character no token spells raises ValueError.

    Wildcards (INTEGRATION.md "Wildcards"), for transcripts that skip audio.  `wildcard_penalty` (logit units per wildcard
    frame, >= 0) has NO default: the useful value depends on a trained model's posteriors and no checkpoint was at hand;
    a target that holds a wildcard without it raises ValueError.  Id sequences may hold WILDCARD.  With `wildcard_token`
    (a string the vocabulary cannot spell) a text is split at it: the pieces are tokenised as ever, empty pieces vanish,
    word delimiters next to a wildcard are dropped and adjacent wildcards collapse to one.  A wildcard belongs to no Word.
    `segments` locates utterances, given in spoken order, in a recording that holds other audio around them."""

    def __init__(self, vocab: Sequence[str], blank_id: int, delim_token: str = "|", frame_seconds: float = 0.04,
                 skip_ids: Sequence[int] = (), wildcard_token: Optional[str] = None,
                 wildcard_penalty: Optional[float] = None) -> None:
        self.vocab = list(vocab)
        self.blank_id = int(blank_id)
        if not 0 <= self.blank_id < len(self.vocab):
            raise ValueError(f"blank_id {blank_id} outside the vocabulary of {len(self.vocab)} tokens")
        self.delim_token = delim_token
        self.delim_id = self.vocab.index(delim_token) if delim_token in self.vocab else None
        self.frame_seconds = float(frame_seconds)
        self.skip_ids = frozenset(int(i) for i in skip_ids)
        spell = {}
        for i, tok in enumerate(self.vocab):
            if tok and i != self.blank_id and i not in self.skip_ids:
                spell.setdefault(tok, i)
        self._spell = spell
        self._longest = max((len(t) for t in spell), default=1)
        self.wildcard_penalty = None if wildcard_penalty is None else _penalty("CTCAligner", wildcard_penalty)
        self.wildcard_token = None
        if wildcard_token is not None:
            if not isinstance(wildcard_token, str) or not wildcard_token.strip():
                raise ValueError(f"CTCAligner: wildcard_token must be a non-empty string, got {wildcard_token!r}")
            try:
                self._tokenize_piece(wildcard_token)
            except ValueError:
                self.wildcard_token = wildcard_token
            else:
                raise ValueError(f"CTCAligner: the vocabulary spells wildcard_token {wildcard_token!r}: a text could not tell "
                                 "the two apart")

    @classmethod
    def from_decoder(cls, decoder, frame_seconds: float = 0.04, wildcard_token: Optional[str] = None,
                     wildcard_penalty: Optional[float] = None) -> "CTCAligner":
        """Vocabulary, blank, delimiter and skipped ids of a BeamCTCDecoder."""
        return cls(decoder.vocab, decoder.blank_id, decoder.delim_token, frame_seconds, tuple(sorted(decoder.skip_ids)),
                   wildcard_token, wildcard_penalty)

    def tokenize(self, text: str) -> List[int]:
        if self.wildcard_token is None:
            return self._tokenize_piece(text)
        ids: List[int] = []
        pieces = text.split(self.wildcard_token)
        for k, piece in enumerate(pieces):
            if k > 0 and (not ids or ids[-1] != WILDCARD):               # adjacent wildcards collapse to one
                ids.append(WILDCARD)
            toks = self._tokenize_piece(piece)
            while k > 0 and toks and toks[0] == self.delim_id:           # delimiters next to a wildcard are dropped
                toks = toks[1:]
            while k < len(pieces) - 1 and toks and toks[-1] == self.delim_id:
                toks = toks[:-1]
            ids += toks
        return ids

    def _tokenize_piece(self, text: str) -> List[int]:
        s = text.replace(" ", self.delim_token) if self.delim_id is not None else text
        ids, i = [], 0
        while i < len(s):
            for n in range(min(self._longest, len(s) - i), 0, -1):
                tok = self._spell.get(s[i:i + n])
                if tok is not None:
                    ids.append(tok)
                    i += n
                    break
            else:
                raise ValueError(f"no vocabulary token spells {s[i]!r} (position {i} of {text!r})")
        return ids

    def _ids(self, item) -> List[int]:
        if isinstance(item, str):
            return self.tokenize(item)
        if isinstance(item, torch.Tensor):
            item = item.tolist()
        ids = [int(i) for i in item]
        for i in ids:
            if i != WILDCARD and (not 0 <= i < len(self.vocab) or i == self.blank_id):
                raise ValueError(f"target id {i} is outside [0,{len(self.vocab)}) or is the blank id {self.blank_id}")
        return ids

    def align(self, logits: torch.Tensor, targets: Sequence, lengths: Optional[torch.Tensor] = None, long: bool = False):
        """The targets as id lists and the Alignment of ctc_forced_align for them (long=True: of ctc_forced_align_long,
        for recordings beyond MAX_FRAMES / MAX_TARGET).  Targets that hold a wildcard go through the wildcard entry with
        this aligner's wildcard_penalty (ValueError without one); targets without any run exactly as ever."""
        ids = [self._ids(t) for t in targets]
        wild = any(WILDCARD in i for i in ids)
        if wild and self.wildcard_penalty is None:
            raise ValueError("CTCAligner: a target holds a wildcard but no wildcard_penalty was given (there is no default: "
                             "it depends on the model's posteriors)")
        if logits.dim() != 3 or logits.shape[0] != len(ids):
            raise ValueError(f"logits: expected ({len(ids)},T,V), got {tuple(logits.shape)}")
        if logits.shape[2] != len(self.vocab):
            raise ValueError(f"vocab has {len(self.vocab)} tokens, the logits {logits.shape[2]}")
        lmax = max((len(i) for i in ids), default=0)
        padded = torch.tensor([i + [0] * (lmax - len(i)) for i in ids], dtype=torch.int64).reshape(len(ids), lmax)
        tlen = torch.tensor([len(i) for i in ids], dtype=torch.int64)
        if lengths is not None and not (isinstance(lengths, torch.Tensor) and lengths.is_cuda):
            lengths = torch.as_tensor(lengths, dtype=torch.int64).reshape(-1).to(logits.device)
        fn = ctc_forced_align_long if long else ctc_forced_align
        kw = {"wildcard_penalty": self.wildcard_penalty} if wild else {}
        return ids, fn(logits, padded.to(logits.device), self.blank_id, lengths, tlen.to(logits.device), **kw)

    def words(self, ids: Sequence[Sequence[int]], al: Alignment) -> List[List[Word]]:
        """Words of every utterance from its Alignment (one device-to-host copy; an infeasible utterance gives [])."""
        ok = al.ok.cpu().tolist()
        starts, ends, scores = al.token_start.cpu().tolist(), al.token_end.cpu().tolist(), al.token_score.cpu().tolist()
        out = []
        for b, row in enumerate(ids):
            n = len(row)
            out.append(group_words(row, starts[b][:n], ends[b][:n], scores[b][:n], self.vocab, self.delim_id,
                                   self.frame_seconds, self.skip_ids, wildcard=WILDCARD) if ok[b] else [])
        return out

    def segment_targets(self, utterances: Sequence, ends: bool = True):
        """One recording's utterances (texts or id lists, in spoken order) as ONE target with a wildcard between them and,
        with `ends`, in front and behind: (ids, [(first, last + 1) token range of every utterance])."""
        ids: List[int] = [WILDCARD] if ends else []
        ranges = []
        for k, u in enumerate(utterances):
            toks = self._ids(u)
            while toks and toks[0] in (WILDCARD, self.delim_id):         # the wildcard between two utterances is put here
                toks = toks[1:]
            while toks and toks[-1] in (WILDCARD, self.delim_id):
                toks = toks[:-1]
            if not toks:
                raise ValueError(f"CTCAligner.segments: utterance {k} ({u!r}) has no token to locate")
            if k > 0:
                ids.append(WILDCARD)
            ranges.append((len(ids), len(ids) + len(toks)))
            ids += toks
        if ends and ranges:
            ids.append(WILDCARD)
        return ids, ranges

    def segments_of(self, utterances: Sequence[Sequence], targets: Sequence[Sequence[int]], ranges: Sequence, al: Alignment):
        """Segments of every recording from the Alignment of its segment_targets (one device-to-host copy; a recording whose
        target does not fit its frames gives [])."""
        ok = al.ok.cpu().tolist()
        starts, ends, scores = al.token_start.cpu().tolist(), al.token_end.cpu().tolist(), al.token_score.cpu().tolist()
        out: List[List[Segment]] = []
        for b, row in enumerate(targets):
            segs: List[Segment] = []
            for k, (lo, hi) in enumerate(ranges[b] if ok[b] else ()):
                s, e, sc = starts[b][lo:hi], ends[b][lo:hi], scores[b][lo:hi]
                words = group_words(row[lo:hi], s, e, sc, self.vocab, self.delim_id, self.frame_seconds, self.skip_ids,
                                    wildcard=WILDCARD)
                real = [j for j in range(hi - lo) if row[lo + j] != WILDCARD]
                frames = sum(e[j] - s[j] for j in real)
                score = sum(sc[j] * (e[j] - s[j]) for j in real) / frames if frames > 0 else -math.inf
                u = utterances[b][k]
                text = u if isinstance(u, str) else " ".join(w.text for w in words)
                segs.append(Segment(k, text, s[0], e[-1], s[0] * self.frame_seconds, e[-1] * self.frame_seconds, score, words))
            out.append(segs)
        return out

    def segments(self, logits: torch.Tensor, utterances: Sequence, lengths: Optional[torch.Tensor] = None, long: bool = False,
                 ends: bool = True) -> Union[List[Segment], List[List[Segment]]]:
        """Where is each utterance?  `utterances`: per recording a list of texts or id lists that the recording contains
        somewhere, in spoken order (logits (T,V): one such list).  Every recording is aligned ONCE against
        [W] u1 W u2 ... uN [W], W a wildcard (the outer two with `ends`; without them the recording starts and ends with
        the utterances), and every utterance comes back as a Segment.  Needs wildcard_penalty.  A recording whose
        utterances do not fit its frames gives []."""
        single = logits.dim() == 2
        if single:
            logits, utterances = logits.unsqueeze(0), [utterances]
        if any(isinstance(u, str) for u in utterances):
            raise ValueError("CTCAligner.segments: every recording takes a LIST of utterances, got a single string")
        if self.wildcard_penalty is None:
            raise ValueError("CTCAligner.segments: needs the aligner's wildcard_penalty (there is no default: it depends on the "
                             "model's posteriors)")
        built = [self.segment_targets(u, ends) for u in utterances]
        ids, al = self.align(logits, [t for t, _ in built], lengths, long)
        out = self.segments_of(utterances, ids, [r for _, r in built], al)
        return out[0] if single else out

    def __call__(self, logits: torch.Tensor, targets: Union[Sequence[str], Sequence[Sequence[int]]],
                 lengths: Optional[torch.Tensor] = None, long: bool = False) -> List[List[Word]]:
        single = logits.dim() == 2
        if single:
            logits, targets = logits.unsqueeze(0), [targets]
        ids, al = self.align(logits, targets, lengths, long)
        out = self.words(ids, al)
        return out[0] if single else out

    def hypotheses(self, logits: torch.Tensor, tokens: torch.Tensor, counts: torch.Tensor,
                   lengths: Optional[torch.Tensor] = None, n_best: int = 1) -> Union[List[List[Word]], List[List[List[Word]]]]:
        """Words of what a beam search returned: tokens (B,N,T) int64 padded with -1 and counts (B,N), as
        beam_ctc_decode / BeamCTCDecoder's searches give them.  The best row only by default (a list of Word per
        utterance); with n_best > 1 a list of up to n_best word lists per utterance.  The scores are acoustic: the mean
        log-probability of the words' frames, without the language-model or hotword terms of the search."""
        if tokens.dim() != 3 or counts.dim() != 2 or tokens.shape[:2] != counts.shape:
            raise ValueError(f"tokens / counts: expected (B,N,T) and (B,N), got {tuple(tokens.shape)}, {tuple(counts.shape)}")
        tk, ct = tokens.cpu().tolist(), counts.cpu().tolist()
        rows = min(int(n_best), tokens.shape[1])
        per_rank = []
        for r in range(rows):
            targets = [tk[b][r][:max(ct[b][r], 0)] for b in range(len(tk))]
            ids, al = self.align(logits, targets, lengths)
            per_rank.append(self.words(ids, al))
        if int(n_best) == 1:
            return per_rank[0]
        return [[per_rank[r][b] for r in range(rows)] for b in range(len(tk))]
