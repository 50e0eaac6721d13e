"""Endpointing without a GPU: the float64 restatement against hand-worked flag sequences, the host arithmetic and refusals of
conformer_amd/endpoint.py, the binding of include/conformer_hip_endpoint.h, and SlotTranscriber's host logic on stand-ins."""
import ctypes
import math
import os
import re

import pytest

from conformer_amd import _lib, decode
from conformer_amd.endpoint import (DEFAULT_RULES, Endpoint, EndpointConfig, EndpointRule, StreamingEndpointer, endpoint_of,
                                    silence_ids)
from tests import endpoint_restatement as R

FS = 0.04
RULES = [r.frames(FS) for r in DEFAULT_RULES]


# ---- the restatement, by hand -------------------------------------------------------------------------------------------------
def test_default_rules_in_frames():
    assert RULES == [(125, 0, 0, 0), (25, 0, 1, 0), (0, 500, 0, 0)]


def test_rule_0_fires_after_exactly_5_s_of_silence_with_nothing_spoken():
    assert R.run_flags([True] * 124, RULES) == [124, 124, 0, -1, 0, 0, 0, 0]
    assert R.run_flags([True] * 125, RULES) == [125, 125, 0, 0, 124, 125, 0, 0]


def test_rule_1_fires_after_exactly_1_s_of_silence_behind_speech():
    flags = [True] * 30 + [False] * 10
    assert R.run_flags(flags + [True] * 24, RULES) == [64, 24, 10, -1, 0, 0, 0, 0]
    assert R.run_flags(flags + [True] * 25, RULES) == [65, 25, 10, 1, 64, 25, 0, 0]


def test_rule_2_fires_at_exactly_20_s_whatever_was_said():
    flags = ([False] + [True] * 9) * 50                     # never 25 silent frames in a row
    assert R.run_flags(flags[:499], RULES)[3] == -1
    assert R.run_flags(flags, RULES) == [500, 9, 50, 2, 499, 9, 0, 0]
    assert R.run_flags([False] * 500, RULES) == [500, 0, 500, 2, 499, 0, 0, 0]


def test_the_lowest_rule_index_wins_when_two_hold_at_once():
    rules = [(0, 5, 0, 0), (2, 0, 0, 0)]
    assert R.run_flags([False] * 3 + [True] * 2, rules) == [5, 2, 3, 0, 4, 2, 0, 0]      # both hold at frame 4
    assert R.run_flags([True] * 2, rules) == [2, 2, 0, 1, 1, 2, 0, 0]                     # rule 1 alone holds first
    # all three default rules at frame 499: 125 silent frames end there, something was spoken, 500 frames
    flags = [False] * 375 + [True] * 125
    assert R.run_flags(flags, [RULES[0], RULES[2]]) == [500, 125, 375, 0, 499, 125, 0, 0]


def test_the_latch_holds_while_the_counters_go_on():
    st = R.run_flags([False] * 4 + [True] * 25, RULES)
    assert st == [29, 25, 4, 1, 28, 25, 0, 0]
    R.run_flags([True] * 3 + [False] * 2 + [True] * 200, RULES, st)    # rule 0 and rule 1 hold again later: nothing moves
    assert st == [234, 200, 6, 1, 28, 25, 0, 0]


def test_the_frame_classification():
    inf = math.inf
    thr = 0.8
    assert R.is_silent([2.0, -inf, -inf], [0], thr) and R.log_p_silence([2.0, -inf, -inf], [0]) == 0.0
    assert not R.is_silent([-inf, 0.0, 1.0], [0], thr)
    assert not R.is_silent([5.0, math.nan, 0.0], [0], thr)
    assert not R.is_silent([-inf, -inf, -inf], [0], thr)
    x = [math.log(0.5), math.log(0.4), math.log(0.1)]
    assert not R.is_silent(x, [0], thr) and not R.is_silent(x, [1], thr) and R.is_silent(x, [0, 1], thr)
    assert abs(R.log_p_silence(x, [0, 1]) - math.log(0.9)) < 1e-15


# ---- host arithmetic ----------------------------------------------------------------------------------------------------------
def test_seconds_to_frames():
    assert EndpointRule(1.0).frames(0.04) == (25, 0, 1, 0)
    assert EndpointRule(0.05, 0.07, 0.11).frames(0.04) == (1, 2, 3, 0)            # 1.25, 1.75, 2.75
    assert EndpointRule(1.0, 2.0, 0.2, must_contain_speech=True).frames(0.04) == (25, 50, 5, 0)
    assert EndpointRule(1.0, must_contain_speech=False).frames(0.04) == (25, 0, 0, 0)
    assert EndpointRule(0.0, 0.0, 0.004, must_contain_speech=True).frames(0.04) == (0, 0, 1, 0)   # rounds to 0: one frame
    assert EndpointRule(1.0).frames(0.01) == (100, 0, 1, 0)
    assert EndpointRule(1.0).frames(0.03) == (33, 0, 1, 0)


def test_endpoint_of_a_state_row():
    assert endpoint_of([7, 3, 2, -1, 0, 0, 0, 0], 0.04) is None
    e = endpoint_of([70, 30, 2, 1, 64, 25, 0, 0], 0.04)
    assert e == Endpoint(1, 64, 65 * 0.04, 25)


def test_silence_ids_are_the_blank_first_without_repeats():
    assert silence_ids(3, EndpointConfig()) == [3]
    assert silence_ids(0, EndpointConfig(silence_ids=(15, 0, 15))) == [0, 15]
    assert silence_ids(0, EndpointConfig(silence_ids=(15,)), vocab=16) == [0, 15]


# ---- refusals: ValueError before any device is used ---------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [0.0, 1.0, -0.1, 1.5, math.nan, "0.8", True, None])
def test_threshold_outside_the_open_interval(thr):
    with pytest.raises(ValueError, match="blank_threshold"):
        EndpointConfig(blank_threshold=thr).check(FS)
    with pytest.raises(ValueError, match="blank_threshold"):
        StreamingEndpointer(2, 0, EndpointConfig(blank_threshold=thr))


def test_too_many_or_no_rules_and_ids():
    with pytest.raises(ValueError, match="rules"):
        EndpointConfig(rules=[EndpointRule(1.0)] * 5).check(FS)
    with pytest.raises(ValueError, match="rules"):
        EndpointConfig(rules=()).check(FS)
    with pytest.raises(ValueError, match="EndpointRule"):
        EndpointConfig(rules=[(25, 0, 1, 0)]).check(FS)
    assert len(EndpointConfig(rules=[EndpointRule(1.0)] * 4).check(FS)) == 4
    with pytest.raises(ValueError, match="silence_ids"):
        EndpointConfig(silence_ids=tuple(range(1, 9))).check(FS)                  # 8 beside the blank: 9 ids
    EndpointConfig(silence_ids=tuple(range(1, 8))).check(FS)
    with pytest.raises(ValueError, match="silence_ids"):
        EndpointConfig(silence_ids=(1.5,)).check(FS)


def test_ids_outside_the_vocabulary():
    with pytest.raises(ValueError, match=r"\[16\] outside \[0, 16\)"):
        silence_ids(0, EndpointConfig(silence_ids=(15, 16)), vocab=16)
    with pytest.raises(ValueError, match="outside"):
        silence_ids(16, EndpointConfig(), vocab=16)
    with pytest.raises(ValueError, match="outside"):
        StreamingEndpointer(2, 0, EndpointConfig(silence_ids=(-1,)))
    with pytest.raises(ValueError, match="blank_id"):
        StreamingEndpointer(2, -1)


@pytest.mark.parametrize("field", ["min_trailing_silence", "min_utterance_length", "min_speech"])
@pytest.mark.parametrize("bad", [-0.5, math.nan, math.inf, "1", True])
def test_negative_or_meaningless_times(field, bad):
    kw = dict(min_trailing_silence=1.0)
    kw[field] = bad
    with pytest.raises(ValueError, match=field):
        EndpointRule(**kw).frames(FS)
    with pytest.raises(ValueError, match=field):
        StreamingEndpointer(2, 0, EndpointConfig(rules=[EndpointRule(**kw)]))


def test_other_constructor_refusals():
    with pytest.raises(ValueError, match="frame_seconds"):
        StreamingEndpointer(2, 0, frame_seconds=0.0)
    with pytest.raises(ValueError, match="slots"):
        StreamingEndpointer(0, 0)
    with pytest.raises(ValueError, match="EndpointConfig"):
        StreamingEndpointer(2, 0, config=0.8)
    with pytest.raises(ValueError, match="must_contain_speech"):
        EndpointRule(1.0, must_contain_speech=1).frames(FS)
    with pytest.raises(ValueError, match="int32"):
        EndpointRule(1e9).frames(FS)


def test_slot_transcriber_refuses_a_bad_endpoint_before_the_model_is_used():
    from conformer_amd.slots import SlotTranscriber
    with pytest.raises(ValueError, match="blank_threshold"):
        SlotTranscriber(None, None, 2, 100, endpoint=EndpointConfig(blank_threshold=1.0))
    with pytest.raises(ValueError, match="EndpointConfig"):
        SlotTranscriber(None, None, 2, 100, endpoint=True)


# ---- the binding ----------------------------------------------------------------------------------------------------------------
def test_the_header_parses_into_its_own_table():
    """what every header shares (record, names, binding, rebuild message, build) is asserted in test_abi_binding_cpu"""
    signatures = _lib.HEADERS["conformer_hip_endpoint.h"].signatures
    assert list(signatures) == ["cfm_endpoint_step_f32"]
    p, i, i64, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    res, args = signatures["cfm_endpoint_step_f32"]
    assert res is i and len(args) == 14
    assert args == [p, i64, i64, p, i, i, p, i, f, p, i, p, i, p]
    assert _lib.PARAMS["cfm_endpoint_step_f32"] == ["logits", "ld_slot", "ld_row", "k", "k_max", "V", "silence_ids", "n_silence",
                                                     "log_threshold", "rules", "n_rules", "state", "S", "stream"]
    with open(_lib.HEADER_PATH) as fh:
        main = fh.read()
    assert "conformer_hip_endpoint.h" not in main and "cfm_endpoint" not in main # the main header stays as it was
    assert os.path.exists(_lib.LIB_PATH), "build the library first (python -m conformer_amd.build)"
    with open(_lib.LIB_PATH, "rb") as fh:
        assert re.search(b"cfm_endpoint_step_f32\0", fh.read()), "cfm_endpoint_step_f32 is not in the library's symbol strings"


# ---- SlotTranscriber's host logic on stand-ins ------------------------------------------------------------------------------------
class _Enc:
    def __init__(self):
        self.is_open, self.n0 = [True, True], [40, 7]

    def _check_slot(self, s, want_open):
        if self.is_open[s] != want_open:
            raise RuntimeError(f"slot {s} is {'free' if want_open else 'already open'}")
        return s

    def close(self, s):
        self.is_open[s] = False


def test_endpoints_without_endpoint_raises():
    from conformer_amd import slots
    tr = object.__new__(slots.SlotTranscriber)
    tr.S, tr.encoder = 2, _Enc()
    with pytest.raises(RuntimeError, match="endpoint="):
        tr.endpoints()


def test_segment_returns_the_close_text_and_keeps_the_slot_open(monkeypatch):
    import types

    import torch

    from conformer_amd import slots
    reset, armed = [], []
    st = types.SimpleNamespace(B=2, max_pending=None, times=None)
    monkeypatch.setattr(decode, "beam_ctc_stream_init", lambda *a, **kw: st)
    monkeypatch.setattr(decode, "beam_ctc_stream_reset_slots", lambda st, idx: reset.extend(idx.tolist()))
    tokens = torch.tensor([[[1, 2, -1]], [[2, -1, -1]]])
    monkeypatch.setattr(decode, "beam_ctc_stream_finish", lambda st, n_best=1: (tokens, torch.tensor([[2], [1]]), None, None, None))
    dec = decode.BeamCTCDecoder(["_", "a", "b", "|"], blank_id=0, beam_width=4)
    tr = object.__new__(slots.SlotTranscriber)
    tr.S, tr.encoder, tr.seg_start, tr.frame_seconds = 2, _Enc(), [0, 0], 0.04
    tr.endpointer = types.SimpleNamespace(
        reset_slots=armed.extend,
        read=lambda only=None: [Endpoint(1, 3, 4 * 0.04, 25), None])
    tr.beam = dec.stream(2, 10, "cpu")
    assert tr.endpoints() == {0: Endpoint(1, 3, 4 * 0.04, 25)}
    assert tr.segment(0) == "ab" and reset == [0] and armed == [0]
    assert tr.encoder.is_open == [True, True] and tr.seg_start == [40, 0] and not tr.beam.finished
    assert tr.endpoints() == {0: Endpoint(1, 43, 44 * 0.04, 25)}                  # on the clock of open(0)
    assert tr.segment(1, decode_func=str.upper) == "B" and reset == [0, 1] and tr.seg_start == [40, 7]
    assert tr.close(0) == "ab" and tr.encoder.is_open == [False, True]
    with pytest.raises(RuntimeError, match="free"):
        tr.segment(0)
