"""Word, character and token error counts on the device ("Error rates on the device").

The reference scores every validation batch with `metric.wer_score(processor.batch_greedy_decode(outputs),
processor.batch_decode_tokens(y))` on host strings.  Here the token ids that `greedy_ctc_decode` and the beam search leave on the
device go straight into `csrc/error_rate.hip`: one launch turns token rows into unit streams (the code points of
`BeamCTCDecoder.text(ids)`, its words as spans, and the ids without the skip ids), one launch takes the Levenshtein distance of
every (reference, hypothesis) pair.  `error_counts` returns the integer counts, `ErrorRateMeter` sums them over batches in int64
device accumulators and synchronises only in `compute()`.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Sequence, Tuple

import numpy as np

from . import _lib
from .hotwords import Hotwords
from .lm import TOK_CHARS, PackedTables, token_code_points

MAX_UNITS = 16384            # units per side and kind (include/conformer_hip_error_rate.h)
UNITS = {"word": 0, "char": 1, "token": 2}
_ALL = 3


class ErrorRateTables(PackedTables):
    """The vocabulary as the scoring kernels read it: a token in `skip_ids` spells nothing, a token equal to `delim_token` or " "
    is a delimiter, every other token spells its code points (`Hotwords.token_kinds`, which refuses a non-delimiter token with
    whitespace in it).  A non-delimiter token that contains `delim_token` is refused too: `BeamCTCDecoder.text` would split it.
    Packed once on the host and copied once per device (PackedTables)."""

    def __init__(self, vocab: Sequence[str], delim_token: str = "|", skip_ids: Iterable[int] = ()) -> None:
        super().__init__()
        if isinstance(vocab, (str, bytes)) or not all(isinstance(t, str) for t in vocab):
            raise ValueError("ErrorRateTables: vocab must be a sequence of str")
        if not isinstance(delim_token, str) or not delim_token:
            raise ValueError(f"ErrorRateTables: delim_token must be a non-empty str, got {delim_token!r}")
        self.vocab = list(vocab)
        if not self.vocab:
            raise ValueError("ErrorRateTables: the vocabulary is empty")
        self.delim_token = delim_token
        self.skip_ids = frozenset(int(i) for i in skip_ids)
        self.kinds = Hotwords.token_kinds(self.vocab, delim_token, self.skip_ids)
        for i, (t, k) in enumerate(zip(self.vocab, self.kinds)):
            if k == TOK_CHARS and delim_token in t:
                raise ValueError(f"ErrorRateTables: vocabulary token {i} ({t!r}) contains the delimiter {delim_token!r}")
        self.tok_off, self.tok_cp = token_code_points(self.vocab, self.kinds)
        self.max_token_cps = int(np.diff(self.tok_off).max())
        if int(self.tok_off[-1]) >= 2 ** 31:
            raise ValueError("ErrorRateTables: the vocabulary spells more than 2^31 code points")

    def _pack(self, vocab: Sequence[str], delim_token: str, skip: frozenset) -> np.ndarray:
        """int32 words: kinds (V), offsets (V + 1), code points"""
        blob = np.concatenate([self.kinds.astype(np.int32), self.tok_off.astype(np.int32), self.tok_cp.astype(np.int32)])
        return np.ascontiguousarray(blob).view(np.uint8)

    def on(self, device) -> Tuple[object, object, object]:
        """(tok_kind (V), tok_off (V + 1), tok_cp) int32 views of the tables on `device`"""
        t = self.device_tables(self.vocab, self.delim_token, self.skip_ids, device).view(_torch().int32)
        V = len(self.vocab)
        return t[:V], t[V:2 * V + 1], t[2 * V + 1:]


def _torch():
    import torch
    return torch


def _rows(pairs, who: str):
    """int64 device rows and counts of matching shape, contiguous; dtypes and shapes are checked before devices"""
    torch = _torch()
    for name, tokens, counts in pairs:
        _dtype_and_shape(torch, tokens, counts, who, name)
    out = []
    for name, tokens, counts in pairs:
        for t, n in ((tokens, f"{name}_tokens"), (counts, f"{name}_counts")):
            if not t.is_cuda:
                raise _lib.ConformerHipError(f"{who}: {n}: expected a tensor on a HIP device, got {t.device}; "
                                             "the scoring only exists as gfx950 kernels (no CPU fallback)")
        out += [tokens.contiguous(), counts.contiguous()]
    return out


def _dtype_and_shape(torch, tokens, counts, who: str, name: str) -> None:
    for t, n in ((tokens, f"{name}_tokens"), (counts, f"{name}_counts")):
        if not isinstance(t, torch.Tensor):
            raise _lib.ConformerHipError(f"{who}: {n}: expected a tensor on a HIP device, got {type(t).__name__}")
        if t.dtype != torch.int64:
            raise _lib.ConformerHipError(f"{who}: {n}: expected dtype torch.int64, got {t.dtype}")
    if tuple(counts.shape) != tuple(tokens.shape[:-1]):
        raise ValueError(f"{who}: {name}_counts has shape {tuple(counts.shape)}, {name}_tokens {tuple(tokens.shape)}")


class _Units:
    """The unit streams of R token rows, as cfm_error_rate_units writes them"""

    def __init__(self, tokens, counts, tables: ErrorRateTables, who: str) -> None:
        torch = _torch()
        R, L = tokens.shape
        mc = max(tables.max_token_cps, 1)
        dev = tokens.device
        self.ld_cps, self.ld = L * mc, L
        self.cps = torch.empty(R, self.ld_cps, dtype=torch.int32, device=dev)
        self.words = torch.empty(R, L, 4, dtype=torch.int32, device=dev)
        self.toks = torch.empty(R, L, dtype=torch.int32, device=dev)
        self.lens = torch.empty(R, 4, dtype=torch.int32, device=dev)
        kind, off, cp = tables.on(dev)
        _lib.call("cfm_error_rate_units", tokens.data_ptr(), L, counts.data_ptr(), R, L, kind.data_ptr(), off.data_ptr(),
                  cp.data_ptr() if cp.numel() else None, len(tables.vocab), tables.max_token_cps, self.cps.data_ptr(),
                  self.ld_cps, self.words.data_ptr(), L, self.toks.data_ptr(), L, self.lens.data_ptr(), _stream())


def _stream() -> int:
    return _torch().cuda.current_stream().cuda_stream


def _counts(hyp_tokens, hyp_counts, ref_tokens, ref_counts, tables: ErrorRateTables, unit: int, who: str):
    """The three outputs of cfm_error_rate_distance for `unit` (0..2: (B, N), (B, N), (B); 3: a leading axis of three kinds)"""
    torch = _torch()
    if not isinstance(tables, ErrorRateTables):
        raise ValueError(f"{who}: tables must be an ErrorRateTables, got {type(tables).__name__}")
    if not isinstance(hyp_tokens, torch.Tensor) or hyp_tokens.dim() not in (2, 3):
        raise ValueError(f"{who}: hyp_tokens must be (B, L) or (B, N, L), got "
                         f"{tuple(hyp_tokens.shape) if isinstance(hyp_tokens, torch.Tensor) else type(hyp_tokens).__name__}")
    if not isinstance(ref_tokens, torch.Tensor) or ref_tokens.dim() != 2:
        raise ValueError(f"{who}: ref_tokens must be (B, Lr), got "
                         f"{tuple(ref_tokens.shape) if isinstance(ref_tokens, torch.Tensor) else type(ref_tokens).__name__}")
    hyp_tokens, hyp_counts, ref_tokens, ref_counts = _rows((("hyp", hyp_tokens, hyp_counts), ("ref", ref_tokens, ref_counts)),
                                                           who)
    B = hyp_tokens.shape[0]
    N = hyp_tokens.shape[1] if hyp_tokens.dim() == 3 else 1
    if ref_tokens.shape[0] != B:
        raise ValueError(f"{who}: {B} hypothesis rows but {ref_tokens.shape[0]} references")
    if ref_tokens.device != hyp_tokens.device:
        raise ValueError(f"{who}: hypotheses on {hyp_tokens.device}, references on {ref_tokens.device}")
    if min(B, N, hyp_tokens.shape[-1], ref_tokens.shape[-1]) < 1:
        raise ValueError(f"{who}: empty shapes {tuple(hyp_tokens.shape)}, {tuple(ref_tokens.shape)}")
    mc = max(tables.max_token_cps, 1)
    for name, t in (("hyp_tokens", hyp_tokens), ("ref_tokens", ref_tokens)):      # the entries refuse this too; no launch at all
        if t.shape[-1] * mc > MAX_UNITS:
            raise _lib.ConformerHipError(f"{who}: {name}: rows of {t.shape[-1]} tokens of up to {mc} code points may hold "
                                         f"{t.shape[-1] * mc} units, more than the {MAX_UNITS} supported")
    dev = hyp_tokens.device
    hyp = _Units(hyp_tokens.reshape(B * N, -1), hyp_counts.reshape(B * N), tables, who)
    ref = _Units(ref_tokens, ref_counts, tables, who)
    lead = (3,) if unit == _ALL else ()
    errors = torch.empty(lead + (B, N), dtype=torch.int32, device=dev)
    hyp_units = torch.empty(lead + (B, N), dtype=torch.int32, device=dev)
    ref_units = torch.empty(lead + (B,), dtype=torch.int32, device=dev)
    _lib.call("cfm_error_rate_distance", ref.cps.data_ptr(), ref.ld_cps, ref.words.data_ptr(), ref.ld, ref.toks.data_ptr(),
              ref.ld, ref.lens.data_ptr(), hyp.cps.data_ptr(), hyp.ld_cps, hyp.words.data_ptr(), hyp.ld, hyp.toks.data_ptr(),
              hyp.ld, hyp.lens.data_ptr(), B, N, unit, errors.data_ptr(), hyp_units.data_ptr(), ref_units.data_ptr(), _stream())
    return errors, hyp_units, ref_units


def error_counts(hyp_tokens, hyp_counts, ref_tokens, ref_counts, tables: ErrorRateTables, unit: str = "word"):
    """Levenshtein distances between references and hypotheses in `unit`s ("word", "char" or "token"), on the device.
    hyp_tokens (B, L) int64 with hyp_counts (B) as greedy_ctc_decode returns them, or (B, N, L) with (B, N) as the beam search
    does; ref_tokens (B, Lr) int64 padded, ref_counts (B).  Positions at or behind a count are never read.  Returns (errors,
    hyp_units, ref_units): int32, shaped like hyp_counts, like hyp_counts, and (B).  An n-best row with count 0 scores as an
    empty hypothesis.  Nothing synchronises.  Rows of more than MAX_UNITS possible units (the row width times the longest
    token's code points) raise ConformerHipError before anything is launched."""
    if unit not in UNITS:
        raise ValueError(f"error_counts: unit must be one of {sorted(UNITS)}, got {unit!r}")
    errors, hyp_units, ref_units = _counts(hyp_tokens, hyp_counts, ref_tokens, ref_counts, tables, UNITS[unit], "error_counts")
    if hyp_tokens.dim() == 2:
        return errors[:, 0], hyp_units[:, 0], ref_units
    return errors, hyp_units, ref_units


_RATES = ("wer", "cer", "ter")          # the planes of unit = 3: words, characters, tokens


class ErrorRateMeter:
    """Running WER, CER and token error rate of the best hypothesis, and the oracle rates of the n-best list, in int64 device
    accumulators (on `device`, or on the device of the first batch).  update() enqueues only; compute() is the one call that
    synchronises."""

    def __init__(self, tables: ErrorRateTables, device=None) -> None:
        if not isinstance(tables, ErrorRateTables):
            raise ValueError(f"ErrorRateMeter: tables must be an ErrorRateTables, got {type(tables).__name__}")
        self.tables = tables
        # (10) int64: errors w c t, reference units w c t, oracle errors w c t, utterances.  Without `device` they appear with
        # the first batch; a rank that may see no batch before all_reduce() names its device here.
        self.totals = None if device is None else _torch().zeros(10, dtype=_torch().int64, device=device)

    def reset(self) -> None:
        if self.totals is not None:
            self.totals.zero_()

    def update(self, hyp_tokens, hyp_counts, ref_tokens, ref_counts) -> None:
        """Add a batch: (B, L) hypotheses, or (B, N, L) n-best lists, whose row 0 is the best hypothesis and whose oracle is
        the minimum over row 0 and every row with a count above 0."""
        torch = _torch()
        errors, _, ref_units = _counts(hyp_tokens, hyp_counts, ref_tokens, ref_counts, self.tables, _ALL, "ErrorRateMeter.update")
        used = (hyp_counts.reshape(errors.shape[1:]) > 0)
        used[:, 0] = True
        big = torch.iinfo(torch.int32).max
        oracle = torch.where(used.unsqueeze(0), errors, torch.full_like(errors, big)).amin(dim=2)
        batch = torch.cat([errors[:, :, 0].sum(dim=1, dtype=torch.int64), ref_units.sum(dim=1, dtype=torch.int64),
                           oracle.sum(dim=1, dtype=torch.int64),
                           torch.full((1,), errors.shape[1], dtype=torch.int64, device=errors.device)])
        if self.totals is None:
            self.totals = batch
        elif self.totals.device != batch.device:
            raise ValueError(f"ErrorRateMeter.update: the totals live on {self.totals.device}, this batch on {batch.device}")
        else:
            self.totals += batch

    def all_reduce(self) -> None:
        """Sum the accumulators across ranks when torch.distributed is initialised; nothing otherwise."""
        import torch.distributed as dist
        if self.totals is not None and dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.totals)

    def compute(self) -> Dict[str, float]:
        """{"wer", "cer", "ter", "oracle_wer", "oracle_cer", "oracle_ter"} as sum(errors) / sum(reference units) (NaN when the
        denominator is 0), with the integer totals beside them ("word_errors", "ref_words", ..., "utterances")."""
        t = [0] * 10 if self.totals is None else self.totals.cpu().tolist()
        out: Dict[str, float] = {}
        for i, rate in enumerate(_RATES):
            out[rate] = t[i] / t[3 + i] if t[3 + i] else math.nan
            out["oracle_" + rate] = t[6 + i] / t[3 + i] if t[3 + i] else math.nan
        for i, name in enumerate(("word", "char", "token")):
            out[f"{name}_errors"], out[f"ref_{name}s"], out[f"oracle_{name}_errors"] = t[i], t[3 + i], t[6 + i]
        out["utterances"] = t[9]
        return out


def rate_tokens(hyp_tokens, hyp_counts, ref_tokens, ref_counts, tables: ErrorRateTables, unit: str):
    """sum(errors of the best hypothesis) / sum(reference units) as a 0-dim float64 device tensor (NaN for 0 / 0)"""
    torch = _torch()
    errors, _, ref_units = error_counts(hyp_tokens, hyp_counts, ref_tokens, ref_counts, tables, unit)
    if errors.dim() == 2:
        errors = errors[:, 0]
    total = ref_units.sum(dtype=torch.int64).double()
    return torch.where(total > 0, errors.sum(dtype=torch.int64).double() / total, torch.full_like(total, math.nan))
