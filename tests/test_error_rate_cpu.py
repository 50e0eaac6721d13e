"""Error rates without a GPU: the plain-Python restatement against ConformerMetric on BeamCTCDecoder.text strings (the public
definition the device numbers are tied to), the binding of include/conformer_hip_error_rate.h, and the host refusals."""
import ctypes
import math
import os
import random
import re

import pytest
import torch

from conformer_amd import _lib, build
from conformer_amd.decode import BeamCTCDecoder
from conformer_amd.error_rate import MAX_UNITS, ErrorRateMeter, ErrorRateTables, error_counts
from conformer_amd.evaluation import ConformerMetric
from tests import error_rate_restatement as R

# multi-code-point tokens, both delimiters, two skip ids (blank and unk), an empty token and a non-BMP character
VOCAB = ["_", "a", "b", "ch", "sch", "|", " ", "\U0001F600", "é", "<unk>", "", "z"]
SKIP = (0, 9)


def _random_rows(rng, n, max_len):
    rows = []
    for _ in range(n):
        L = rng.randint(0, max_len)
        weights = [1, 4, 4, 2, 1, rng.choice([1, 6]), 1, 1, 1, 1, 1, 2]
        rows.append(rng.choices(range(len(VOCAB)), weights=weights, k=L))
    return rows


# ---- the restatement is the existing public definition ----------------------------------------------------------------------------
def test_the_restatement_equals_conformer_metric_on_the_decoders_text():
    rng = random.Random(5)
    dec = BeamCTCDecoder(VOCAB, blank_id=0, skip_ids=SKIP)
    kinds, cps = R.tables(VOCAB, "|", SKIP)
    metric = ConformerMetric()
    refs, hyps = _random_rows(rng, 300, 24), _random_rows(rng, 300, 24)
    hyps[:40] = [list(r) for r in refs[:40]]                                  # some exact and some near matches
    for h in hyps[20:40]:
        if h:
            h[rng.randrange(len(h))] = rng.randrange(len(VOCAB))
    tot = {"word": [0, 0], "char": [0, 0]}
    n_checked = 0
    for r, h in zip(refs, hyps):
        rt, ht = dec.text(r), dec.text(h)
        assert "".join(map(chr, R.units(r, len(r), kinds, cps, "char"))) == rt
        assert ["".join(map(chr, w)) for w in R.units(h, len(h), kinds, cps, "word")] == ht.split()
        for kind, score in (("word", metric.wer_score), ("char", metric.cer_score)):
            e, nh, nr = R.counts(h, len(h), r, len(r), kinds, cps, kind)
            tot[kind][0] += e
            tot[kind][1] += nr
            got = float(score(ht, rt))
            if nr:
                assert got == float(torch.tensor(e / nr)), (kind, r, h)
                n_checked += 1
            else:
                assert math.isnan(got)
    assert n_checked > 500
    texts_h, texts_r = [dec.text(h) for h in hyps], [dec.text(r) for r in refs]
    assert float(metric.wer_score(texts_h, texts_r)) == float(torch.tensor(R.rate(*tot["word"])))
    assert float(metric.cer_score(texts_h, texts_r)) == float(torch.tensor(R.rate(*tot["char"])))


def test_the_restatement_by_hand():
    kinds, cps = R.tables(VOCAB, "|", SKIP)
    row = [5, 0, 1, 9, 2, 5, 6, 3, 10, 7, 5, 99, -1]                          # |_a<unk>b| ch""😀| then two ids outside V
    assert R.units(row, len(row), kinds, cps, "token") == [5, 1, 2, 5, 6, 3, 10, 7, 5]
    assert R.units(row, len(row), kinds, cps, "char") == [ord(c) for c in "ab ch\U0001F600"]
    assert R.units(row, len(row), kinds, cps, "word") == [(97, 98), (99, 104, 0x1F600)]
    assert R.units(row, 3, kinds, cps, "char") == [97] and R.units(row, 0, kinds, cps, "word") == []
    assert R.units(row, 99, kinds, cps, "token") == R.units(row, 13, kinds, cps, "token")
    assert R.levenshtein("kitten", "sitting") == 3 and R.levenshtein("", "abc") == 3 and R.levenshtein("abc", "") == 3
    assert R.levenshtein([(1, 2), (3,)], [(1, 2), (4,)]) == 1
    assert math.isnan(R.rate(0, 0)) and R.rate(1, 4) == 0.25


# ---- the tables ---------------------------------------------------------------------------------------------------------------------
def test_the_tables_are_the_lm_packers_kinds_and_code_points():
    t = ErrorRateTables(VOCAB, "|", SKIP)
    kinds, cps = R.tables(VOCAB, "|", SKIP)
    assert t.kinds.tolist() == kinds
    assert [t.tok_cp[t.tok_off[i]:t.tok_off[i + 1]].tolist() for i in range(len(VOCAB))] == cps
    assert t.max_token_cps == 3
    blob = t.pack(t.vocab, t.delim_token, t.skip_ids)
    assert blob.dtype.name == "uint8" and blob.size == 4 * (len(VOCAB) + len(VOCAB) + 1 + sum(map(len, cps)))
    assert t.pack(t.vocab, t.delim_token, t.skip_ids) is blob                 # packed once (PackedTables)


def test_a_vocabulary_the_definition_cannot_spell_is_refused():
    with pytest.raises(ValueError, match="whitespace"):
        ErrorRateTables(["_", "a b", "|"])
    with pytest.raises(ValueError, match="whitespace"):
        ErrorRateTables(["_", "a\t", "|"])
    with pytest.raises(ValueError, match="contains the delimiter"):
        ErrorRateTables(["_", "a|b", "|"])
    with pytest.raises(ValueError, match="delim_token"):
        ErrorRateTables(["_", "a"], delim_token="")
    with pytest.raises(ValueError, match="empty"):
        ErrorRateTables([])
    with pytest.raises(ValueError, match="sequence of str"):
        ErrorRateTables("abc")
    ErrorRateTables(["_", " ", "|", "a"])                                     # both delimiters are fine


# ---- host refusals --------------------------------------------------------------------------------------------------------------
def _args(B=2, L=3, N=None):
    shape = (B, L) if N is None else (B, N, L)
    z = lambda *s: torch.zeros(*s, dtype=torch.int64)                       # noqa: E731
    return [z(*shape), z(*shape[:-1]), z(B, 4), z(B)]


def test_cpu_tensors_are_refused():
    t = ErrorRateTables(VOCAB, "|", SKIP)
    with pytest.raises(_lib.ConformerHipError, match="HIP device"):
        error_counts(*_args(), t)
    with pytest.raises(_lib.ConformerHipError, match="HIP device"):
        ErrorRateMeter(t).update(*_args(N=3))
    with pytest.raises(_lib.ConformerHipError, match="HIP device"):
        ConformerMetric().wer_tokens(*_args(), t)
    with pytest.raises(_lib.ConformerHipError, match="HIP device"):
        ConformerMetric().cer_tokens(*_args(), t)
    with pytest.raises(_lib.ConformerHipError, match="HIP device"):
        error_counts(*(_args()[:3] + [[0, 0]]), t)                            # a list is no tensor either


def test_wrong_ranks_dtypes_and_shapes_are_refused():
    t = ErrorRateTables(VOCAB, "|", SKIP)
    a = _args()
    with pytest.raises(ValueError, match="hyp_tokens must be"):
        error_counts(a[0][0], a[1], a[2], a[3], t)
    with pytest.raises(ValueError, match="hyp_tokens must be"):
        error_counts(a[0][None, None], a[1], a[2], a[3], t)
    with pytest.raises(ValueError, match="ref_tokens must be"):
        error_counts(a[0], a[1], a[2][:, None], a[3], t)
    with pytest.raises(_lib.ConformerHipError, match="int64"):
        error_counts(a[0].int(), a[1], a[2], a[3], t)
    with pytest.raises(_lib.ConformerHipError, match="ref_counts.*int64"):
        error_counts(a[0], a[1], a[2], a[3].float(), t)
    with pytest.raises(ValueError, match="hyp_counts has shape"):
        error_counts(a[0], a[1][:1], a[2], a[3], t)
    b = _args(N=3)
    with pytest.raises(ValueError, match="hyp_counts has shape"):
        error_counts(b[0], a[1], b[2], b[3], t)                               # (B) counts for (B, N, L) rows
    with pytest.raises(ValueError, match="ref_counts has shape"):
        error_counts(a[0], a[1], a[2], a[3][:, None], t)
    with pytest.raises(ValueError, match="unit"):
        error_counts(*a, t, unit="phoneme")
    with pytest.raises(ValueError, match="ErrorRateTables"):
        error_counts(*a, VOCAB)
    with pytest.raises(ValueError, match="ErrorRateTables"):
        ErrorRateMeter(VOCAB)


def test_an_empty_meter_computes_nan_and_all_reduce_does_nothing_alone():
    m = ErrorRateMeter(ErrorRateTables(VOCAB, "|", SKIP))
    m.all_reduce()
    m.reset()
    out = m.compute()
    for k in ("wer", "cer", "ter", "oracle_wer", "oracle_cer", "oracle_ter"):
        assert math.isnan(out[k]), k
    assert out["word_errors"] == out["ref_words"] == out["utterances"] == 0


def test_a_zero_denominator_gives_nan_with_errors_counted():
    m = ErrorRateMeter(ErrorRateTables(VOCAB, "|", SKIP))
    m.totals = torch.tensor([3, 4, 5, 0, 0, 0, 2, 3, 4, 2])                  # hypotheses against empty references
    out = m.compute()
    assert all(math.isnan(out[k]) for k in ("wer", "cer", "ter", "oracle_wer", "oracle_cer", "oracle_ter"))
    assert (out["word_errors"], out["char_errors"], out["token_errors"], out["utterances"]) == (3, 4, 5, 2)
    m.totals = torch.tensor([1, 4, 5, 4, 8, 10, 0, 2, 5, 2])
    out = m.compute()
    assert (out["wer"], out["cer"], out["ter"], out["oracle_wer"], out["oracle_cer"], out["oracle_ter"]) == (
        0.25, 0.5, 0.5, 0.0, 0.25, 0.5)
    m.reset()
    assert m.totals.tolist() == [0] * 10


# ---- the binding ----------------------------------------------------------------------------------------------------------------
def test_the_header_parses_into_its_own_table():
    """what every header shares (record, names, binding, rebuild message, build) is asserted in test_abi_binding_cpu"""
    header = _lib.HEADERS["conformer_hip_error_rate.h"]
    signatures = header.signatures
    assert list(signatures) == ["cfm_error_rate_units", "cfm_error_rate_distance"]
    p, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    res, args = signatures["cfm_error_rate_units"]
    assert res is i and args == [p, i64, p, i, i, p, p, p, i, i, p, i64, p, i64, p, i64, p, p]
    assert _lib.PARAMS["cfm_error_rate_units"] == ["ids", "ld_ids", "counts", "R", "L", "tok_kind", "tok_off", "tok_cp", "V",
                                                    "max_token_cps", "cps", "ld_cps", "words", "ld_words", "toks", "ld_toks",
                                                    "lens", "stream"]
    res, args = signatures["cfm_error_rate_distance"]
    assert res is i and args == [p, i64, p, i64, p, i64, p, p, i64, p, i64, p, i64, p, i, i, i, p, p, p, p]
    assert _lib.PARAMS["cfm_error_rate_distance"][-7:] == ["B", "N", "unit", "errors", "hyp_units", "ref_units", "stream"]
    with open(header.path) as fh:
        assert str(MAX_UNITS) in fh.read()                                    # the cap is stated in the header
    with open(_lib.HEADER_PATH) as fh:
        main = fh.read()
    assert "conformer_hip_error_rate.h" not in main and "cfm_error_rate" not in main   # the main header stays as it was
    assert os.path.exists(_lib.LIB_PATH), "build the library first (python -m conformer_amd.build)"
    with open(_lib.LIB_PATH, "rb") as fh:
        blob = fh.read()
    for name in signatures:
        assert re.search(name.encode() + b"\0", blob), f"{name} is not in the library's symbol strings"
    assert any(s.endswith("error_rate.hip") for s in build.sources())


def test_a_meter_with_a_device_has_its_totals_from_the_start():
    m = ErrorRateMeter(ErrorRateTables(VOCAB, "|", SKIP), device="cpu")
    assert m.totals.tolist() == [0] * 10 and m.totals.dtype == torch.int64
    m.all_reduce()
    assert math.isnan(m.compute()["wer"])
