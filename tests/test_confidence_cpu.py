"""Confidence without a GPU: the float64 restatement (tests/confidence_restatement.py) against values worked by hand, the host
checks and refusals of conformer_amd/confidence.py, and the binding of include/conformer_hip_confidence.h."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conformer_amd import _lib
from conformer_amd.align import Word
from conformer_amd.confidence import (AGGREGATIONS, METHODS, ConfidenceConfig, StreamingConfidence, frame_confidence,
                                      greedy_ctc_confidence, span_confidence, word_confidence)
from tests import confidence_restatement as R

# every method with the alphas the ranking asks for
MEASURES = [("max_prob", None), ("entropy", None), ("tsallis", 0.33), ("tsallis", 2.0), ("renyi", 0.33), ("renyi", 2.0)]


# ---- the frame measure, by hand ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,alpha", MEASURES + [("tsallis", 0.5), ("renyi", 8.0)])
@pytest.mark.parametrize("V", [2, 3, 67])
def test_uniform_is_0_and_one_hot_is_1(method, alpha, V):
    assert abs(R.frame_confidence(np.full(V, 1.7), method, alpha)) < 1e-12
    x = np.zeros(V)
    x[V // 2] = 60.0                                        # the rest hold exp(-60) = 9e-27 each
    assert abs(R.frame_confidence(x, method, alpha) - 1.0) < 1e-6


@pytest.mark.parametrize("method,alpha,want", [
    ("max_prob", None, 0.25),                               # (3 / 2 - 1) / 2
    ("entropy", None, 0.0536054),                           # 1 - (3/2) ln 2 / ln 3
    ("tsallis", 2.0, 0.0625),                               # 1 - (3/8 - 1) / (1/3 - 1)
    ("renyi", 2.0, 0.1072107),                              # 1 + ln(3/8) / ln 3
    ("tsallis", 0.5, 0.0340742),                            # 1 - (sqrt(1/2) + 1 - 1) / (sqrt 3 - 1)
    ("renyi", 0.5, 0.0264081)])                             # 1 + ln(sqrt(1/2) + 1) / (-ln 3 / 2)
def test_half_quarter_quarter(method, alpha, want):
    x = np.log([0.5, 0.25, 0.25]) + 3.0                     # (any shift of the logits is the same posterior)
    assert abs(R.frame_confidence(x, method, alpha) - want) < 5e-8


def test_the_hand_values_in_closed_form():
    assert abs(R.frame_confidence(np.log([0.5, 0.25, 0.25]), "entropy") - (1 - 1.5 * math.log(2) / math.log(3))) < 1e-15
    assert abs(R.frame_confidence(np.log([0.5, 0.25, 0.25]), "tsallis", 0.5)
               - (1 - math.sqrt(0.5) / (math.sqrt(3) - 1))) < 1e-15


def test_special_logits():
    inf, nan = math.inf, math.nan
    c = R.frame_confidence([0.0, -inf, 0.0, 0.0], "entropy")                      # uniform over three of four
    assert abs(c - (1 - math.log(3) / math.log(4))) < 1e-15
    assert R.frame_confidence([2.0, -inf, -inf], "entropy") == 1.0
    for method, alpha in MEASURES:
        assert math.isnan(R.frame_confidence([0.0, nan, 1.0], method, alpha))
        assert 0.0 <= R.frame_confidence([0.0, -inf, 1.0], method, alpha) <= 1.0


def test_the_lowest_index_attains_the_maximum():
    assert R.frame_id([0.0, 3.0, 3.0, 1.0]) == 1 and R.frame_id([5.0, 5.0]) == 0 and R.frame_id([-1.0, -2.0, -0.5]) == 2


# ---- ranking ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,alpha", MEASURES)
def test_peaked_frames_rank_above_flat_ones(method, alpha):
    peaked, flat = R.ranking_frames()
    assert peaked.shape == flat.shape == (40, 67)
    gap = R.frames(peaked, method, alpha)[0].mean() - R.frames(flat, method, alpha)[0].mean()
    assert gap >= 0.25, gap


# ---- the span rule ----------------------------------------------------------------------------------------------------------------
CONF = [0.9, 0.5, 0.1, 0.8, 0.25, 0.5]
IDS = [0, 4, 4, 0, 7, 0]


def test_the_four_aggregations_with_and_without_exclusion():
    a = dict(conf=CONF, ids=IDS, total=6, R=6, start=0, end=5)
    assert abs(R.span(aggregation="mean", **a) - 0.51) < 1e-15
    assert R.span(aggregation="min", **a) == 0.1 and R.span(aggregation="max", **a) == 0.9
    assert abs(R.span(aggregation="prod", **a) - 0.009) < 1e-15
    b = dict(a, exclude_ids=(0,))                           # frames 1, 2, 4 count
    assert abs(R.span(aggregation="mean", **b) - 0.85 / 3) < 1e-15
    assert R.span(aggregation="min", **b) == 0.1 and R.span(aggregation="max", **b) == 0.5
    assert abs(R.span(aggregation="prod", **b) - 0.0125) < 1e-15


def test_empty_all_excluded_and_rolled_out_spans():
    assert math.isnan(R.span(CONF, IDS, 6, 6, 3, 3, "mean"))                      # empty
    assert math.isnan(R.span(CONF, IDS, 6, 6, 4, 2, "mean"))
    assert math.isnan(R.span(CONF, IDS, 6, 6, 6, 9, "mean"))                      # clamped to [6, 6): empty
    assert math.isnan(R.span(CONF, IDS, 6, 6, -1, -1, "min"))                     # (padding)
    assert R.span(CONF, IDS, 6, 6, 4, 9, "min") == 0.25                           # clamped to [4, 6)
    assert R.span(CONF, IDS, 6, 6, 1, 3, "max", exclude_ids=(4,)) == 0.5          # all excluded: all count
    assert R.span(CONF, IDS, 6, 6, 1, 4, "max", exclude_ids=(4,)) == 0.8
    # a ring of 6 that has taken 8 frames holds frames 2 .. 7; frame t sits at t mod 6
    assert math.isnan(R.span(CONF, IDS, 8, 6, 1, 4, "mean"))                      # start 1 < 8 - 6
    assert R.span(CONF, IDS, 8, 6, 2, 4, "min") == 0.1                            # frames 2, 3
    assert R.span(CONF, IDS, 8, 6, 5, 8, "max") == 0.9                            # frames 5, 6, 7 at columns 5, 0, 1
    nan_conf = CONF[:2] + [math.nan] + CONF[3:]
    for agg in R.AGGREGATIONS:
        assert math.isnan(R.span(nan_conf, IDS, 6, 6, 1, 4, agg)) and not math.isnan(R.span(nan_conf, IDS, 6, 6, 3, 6, agg))
    assert [math.isnan(v) for v in R.spans(CONF, IDS, 6, 6, [0, 1, 2], [1, 2, 3], 2, "mean")] == [False, False, True]


# ---- the greedy spans ---------------------------------------------------------------------------------------------------------------
def test_greedy_spans_by_hand():
    pad, unk = 0, 9
    #      t: 0  1  2  3  4  5  6  7  8  9
    row = [0, 3, 3, 0, 3, 5, 9, 5, 4, 0]                    # 3 repeats across a pad, 5 across an unk; leading and trailing pad
    assert R.greedy_tokens(row, pad, unk) == [3, 5, 4]
    assert R.greedy_spans(row, pad, unk) == ([1, 5, 8] + [-1] * 7, [5, 8, 10] + [-1] * 7)
    assert R.greedy_spans(row, pad, unk, length=8) == ([1, 5] + [-1] * 8, [5, 8] + [-1] * 8)       # lengths shorter than T
    assert R.greedy_spans(row, pad, unk, length=1) == ([-1] * 10, [-1] * 10)
    assert R.greedy_spans([0, 9, 0], pad, unk) == ([-1] * 3, [-1] * 3)                              # all pad
    assert R.greedy_spans([2, 3, 2], pad, unk) == ([0, 1, 2], [1, 2, 3])
    assert R.greedy_spans([2], pad, unk) == ([0], [1])


# ---- host refusals --------------------------------------------------------------------------------------------------------------------
def test_config_defaults_and_names():
    c = ConfidenceConfig()
    assert (c.method, c.alpha, c.aggregation, c.exclude_blank) == ("tsallis", 0.33, "min", True)
    assert c.check() == (METHODS["tsallis"], 0.33, AGGREGATIONS["min"])
    assert tuple(METHODS) == R.METHODS and tuple(AGGREGATIONS) == R.AGGREGATIONS
    assert [METHODS[m] for m in R.METHODS] == [0, 1, 2, 3] and [AGGREGATIONS[a] for a in R.AGGREGATIONS] == [0, 1, 2, 3]
    with pytest.raises(Exception):                          # frozen
        c.alpha = 0.5


def test_unknown_names_are_refused():
    with pytest.raises(ValueError, match="method"):
        ConfidenceConfig(method="gini").check()
    with pytest.raises(ValueError, match="aggregation"):
        ConfidenceConfig(aggregation="median").check()
    with pytest.raises(ValueError, match="exclude_blank"):
        ConfidenceConfig(exclude_blank=1).check()


@pytest.mark.parametrize("alpha", [0, 1, 1.03, 9, 0.06, 0.95, math.nan, "0.33", True])
@pytest.mark.parametrize("method", ["tsallis", "renyi"])
def test_alpha_outside_the_two_ranges_is_refused(method, alpha):
    with pytest.raises(ValueError, match="alpha"):
        ConfidenceConfig(method=method, alpha=alpha).check()
    with pytest.raises(ValueError, match="alpha"):         # before anything touches a device
        StreamingConfidence(2, 0, ConfidenceConfig(method=method, alpha=alpha))


def test_alpha_at_the_ends_of_the_ranges_and_where_it_is_ignored():
    for a in (1 / 16, 15 / 16, 17 / 16, 8, 0.33, 2):
        ConfidenceConfig(method="renyi", alpha=a).check()
    ConfidenceConfig(method="entropy", alpha=1.0).check()
    ConfidenceConfig(method="max_prob", alpha=9).check()


def test_a_cpu_tensor_is_refused_with_the_projects_error():
    x = torch.zeros(2, 3, 5)
    with pytest.raises(_lib.ConformerHipError, match="no CPU fallback"):
        frame_confidence(x)
    with pytest.raises(_lib.ConformerHipError, match="no CPU fallback"):
        greedy_ctc_confidence(x, 0, 1)
    with pytest.raises(_lib.ConformerHipError, match="no CPU fallback"):
        span_confidence(torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 1, dtype=torch.int64),
                        torch.ones(2, 1, dtype=torch.int64))
    with pytest.raises(_lib.ConformerHipError, match="no CPU fallback"):
        word_confidence([[Word("a", 0, 1, 0.0, 0.04, 0.0)], []], torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int64), 0)
    with pytest.raises(_lib.ConformerHipError, match="no CPU fallback"):
        StreamingConfidence(2, 0, device="cpu")
    with pytest.raises(ValueError, match="ConfidenceConfig"):
        frame_confidence(x, config="tsallis")
    with pytest.raises(ValueError, match="history"):
        StreamingConfidence(2, 0, history=0)
    with pytest.raises(ValueError, match="slots"):
        StreamingConfidence(0, 0)
    with pytest.raises(ValueError, match="blank_id"):
        StreamingConfidence(2, -1)


def test_the_transcribers_refuse_confidence_without_times_before_the_model_is_used():
    from conformer_amd.slots import SlotTranscriber
    from conformer_amd.transcribe import StreamingTranscriber
    for cls in (SlotTranscriber, StreamingTranscriber):
        with pytest.raises(ValueError, match="times=True"):
            cls(None, None, 2, 100, confidence=ConfidenceConfig())
        with pytest.raises(ValueError, match="alpha"):
            cls(None, None, 2, 100, times=True, confidence=ConfidenceConfig(alpha=1.0))
        with pytest.raises(ValueError, match="ConfidenceConfig"):
            cls(None, None, 2, 100, times=True, confidence=True)
        with pytest.raises(ValueError, match="confidence_history"):
            cls(None, None, 2, 100, times=True, confidence=ConfidenceConfig(), confidence_history=0)
        tr = object.__new__(cls)
        assert tr.confidence is None
        with pytest.raises(RuntimeError, match="confidence="):
            tr.word_confidence({} if cls is SlotTranscriber else [])


# ---- the binding ----------------------------------------------------------------------------------------------------------------------
def test_the_header_parses_into_its_own_table():
    """what every header shares (record, names, binding, rebuild message, build) is asserted in test_abi_binding_cpu"""
    names = ["cfm_confidence_frames_f32", "cfm_confidence_spans_f32", "cfm_confidence_greedy_spans_i64"]
    header = _lib.HEADERS["conformer_hip_confidence.h"]
    assert list(header.signatures) == names
    p, i, i64, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert header.signatures[names[0]] == (i, [p, i64, i64, p, i, i, i, f, p, p, p, i, i, p])
    assert header.signatures[names[1]] == (i, [p, p, p, i, p, p, p, i, i, p, i, p, i, p])
    assert header.signatures[names[2]] == (i, [p, p, p, p, i, i, i, i, p])
    assert _lib.PARAMS[names[0]] == ["logits", "ld_slot", "ld_row", "k", "k_max", "V", "method", "alpha", "conf", "ids", "total",
                                     "R", "S", "stream"]
    assert _lib.PARAMS[names[1]] == ["conf", "ids", "total", "R", "starts", "ends", "n_spans", "L", "aggregation", "exclude_ids",
                                     "n_exclude", "out", "S", "stream"]
    assert _lib.PARAMS[names[2]] == ["frame_ids", "lengths_or_null", "token_start", "token_end", "B", "T", "pad_id", "unk_id",
                                     "stream"]
    consts = header.constants
    assert sorted(consts) == sorted(f"CFM_CONFIDENCE_{n.upper()}" for n in R.METHODS + R.AGGREGATIONS)
    assert not set(consts) & set(_lib.CONSTANTS)
    with open(_lib.HEADER_PATH) as fh:
        main = fh.read()
    assert "conformer_hip_confidence.h" not in main and "cfm_confidence" not in main       # the main header stays as it was
    assert os.path.exists(_lib.LIB_PATH), "build the library first (python -m conformer_amd.build)"
    with open(_lib.LIB_PATH, "rb") as fh:
        blob = fh.read()
    for n in names:
        assert re.search(n.encode() + b"\0", blob), f"{n} is not in the library's symbol strings"
