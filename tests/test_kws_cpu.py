"""Keyword spotting, the parts that need no GPU: the family in the open table, every refusal of the two ABI entries
(conformer_hip3_kws.h; all return before any HIP call), Keywords' normalisation, refusals and packing, the float32
restatement's own properties and suppress_overlaps."""
import ctypes
import math

import numpy as np
import pytest

from conformer_amd import _lib
from conformer_amd.align import CTCAligner
from conformer_amd.kws import (FLAG_FIRST, FLAG_LAST, FLAG_SKIP, GROUP_LANES, MAX_TOKENS, RING_FRAMES, STATE_ROWS, Detection, Keywords,
                               suppress_overlaps)
from tests import kws_restatement as R


@pytest.fixture(scope="module")
def lib():
    import os
    from conformer_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_family_is_in_the_open_table():
    assert _lib.OPEN_CONSTANTS["conformer_hip3_kws.h"] == {
        "CFM3_KWS_STATE_ROWS": 8, "CFM3_KWS_GROUP_LANES": 64, "CFM3_KWS_MAX_TOKENS": 32, "CFM3_KWS_RING_FRAMES": 8,
        "CFM3_KWS_FLAG_FIRST": 1, "CFM3_KWS_FLAG_SKIP": 2, "CFM3_KWS_FLAG_LAST": 4, "CFM3_KWS_V_MAX": 65536}
    assert (STATE_ROWS, GROUP_LANES, MAX_TOKENS, RING_FRAMES, FLAG_FIRST, FLAG_SKIP, FLAG_LAST) == (8, 64, 32, 8, 1, 2, 4)
    assert _lib.OPEN_PARAMS["cfm3_kws_rowmax_f32"] == ["x", "ld_slot", "ld_row", "k", "k_max", "V", "rowmax", "ld_rowmax", "S",
                                                       "stream"]
    assert _lib.OPEN_PARAMS["cfm3_kws_scan_f32"] == ["x", "ld_slot", "ld_row", "rowmax", "ld_rowmax", "k", "k_max", "V", "lanes",
                                                     "threshold", "G", "K", "state", "detections", "max_detections", "counts",
                                                     "S", "stream"]
    assert [_lib.OPEN_ENTRIES["cfm3_kws_scan_f32"][1][i] for i in (1, 2, 4)] == [ctypes.c_int64] * 3


def test_argument_validation_without_gpu(lib):
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    NULL, SHAPE, UNSUPPORTED = (_lib.CONSTANTS[k] for k in ("CFM_ERR_NULL", "CFM_ERR_BAD_SHAPE", "CFM_ERR_UNSUPPORTED"))

    def call(entry, base, **kw):
        args = list(base)
        for k, v in kw.items():
            args[int(k[1:])] = v
        return entry(*args)

    # x, ld_slot, ld_row, k, k_max, V, rowmax, ld_rowmax, S, stream
    rowmax = dict(entry=lib.cfm3_kws_rowmax_f32, base=[a, 16 * 370, 370, a, 16, 370, a, 16, 3, None])
    for i in (0, 3, 6):
        assert call(**rowmax, **{f"a{i}": None}) == NULL, i
    for bad in (dict(a8=0), dict(a8=-1), dict(a4=-1), dict(a5=1), dict(a5=0), dict(a2=369), dict(a1=16 * 370 - 1), dict(a1=-1),
                dict(a7=15)):
        assert call(**rowmax, **bad) == SHAPE, bad
    assert call(**rowmax, a5=65537, a2=65537, a1=16 * 65537) == UNSUPPORTED and call(**rowmax, a8=65536) == UNSUPPORTED
    assert call(**rowmax, a0=None, a8=0) == NULL and call(**rowmax, a8=0, a5=65537) == SHAPE      # the order
    assert call(**rowmax, a2=369, a8=65536) == SHAPE
    assert call(**rowmax, a4=0, a0=None, a1=0, a7=0) == 0                                         # k_max = 0: nothing launched
    # x, ld_slot, ld_row, rowmax, ld_rowmax, k, k_max, V, lanes, threshold, G, K, state, detections, max_detections, counts, S,
    # stream
    scan = dict(entry=lib.cfm3_kws_scan_f32, base=[a, 16 * 370, 370, a, 16, a, 16, 370, a, a, 2, 5, a, a, 4, a, 3, None])
    for i in (0, 3, 5, 8, 9, 12, 13, 15):
        assert call(**scan, **{f"a{i}": None}) == NULL, i
    for bad in (dict(a16=0), dict(a6=-1), dict(a7=1), dict(a10=0), dict(a11=0), dict(a11=129), dict(a14=0), dict(a2=369),
                dict(a1=16 * 370 - 1), dict(a4=15), dict(a10=-1), dict(a14=-2)):
        assert call(**scan, **bad) == SHAPE, bad
    for bad in (dict(a7=65537, a2=65537, a1=16 * 65537), dict(a16=65536), dict(a10=(1 << 20) + 1), dict(a14=(1 << 24) + 1)):
        assert call(**scan, **bad) == UNSUPPORTED, bad
    assert call(**scan, a0=None, a16=0) == NULL and call(**scan, a16=0, a10=(1 << 20) + 1) == SHAPE
    assert call(**scan, a4=15, a14=(1 << 24) + 1) == SHAPE
    assert call(**scan, a6=0, a0=None, a3=None, a1=0, a4=0) == 0                                  # k_max = 0: nothing launched


# ---- Keywords --------------------------------------------------------------------------------------------------------------------
VOCAB = ["<b>", "|", "a", "b", "c", "d", "e", "ab"]


def test_threshold_has_no_default():
    with pytest.raises(TypeError, match="no default"):
        Keywords([[2, 3]], blank_id=0, vocab_size=8)
    assert Keywords([[2, 3]], blank_id=0, vocab_size=8, threshold=0.0).thresholds.tolist() == [0.0]


def test_normalisation():
    al = CTCAligner(VOCAB, 0)
    kw = Keywords(["ab c", "dd", [4, 5, 6]], al, threshold=1.5)
    assert kw.tokens == [[7, 1, 4], [5, 5], [4, 5, 6]] and kw.phrases == ["ab c", "dd", "cde"]      # (longest token first)
    assert (kw.blank_id, kw.vocab_size, kw.G, len(kw)) == (0, 8, 1, 3)
    assert kw.thresholds.dtype == np.float32 and kw.thresholds.tolist() == [-4.5, -3.0, -4.5]
    kw = Keywords([[2], [3, 4]], blank_id=7, vocab_size=8, thresholds=[0.1, 2.0])
    assert kw.thresholds.tolist() == [np.float32(-0.1), -4.0] and kw.phrases == ["2", "3 4"]
    assert kw.thresholds[0] == np.float32(-(0.1 * 1))
    import torch
    assert Keywords([torch.tensor([2, 3])], blank_id=0, vocab_size=8, threshold=1.0).tokens == [[2, 3]]


@pytest.mark.parametrize("phrases, kw, word", [
    ([], {}, "non-empty"), ("ab", {}, "non-empty"), ([[]], {}, "empty"), ([""], {}, "empty"),
    ([[2, 3], [2, 3]], {}, "again"), (["ab", [7]], {}, "again"), ([[0, 2]], {}, "blank"), ([[2, 8]], {}, "outside"),
    ([[-1]], {}, "outside"), ([[2] * 33], {}, "at most 32"), ([[2.0]], {}, "no token id"), ([[True]], {}, "no token id"),
    (["xyz"], {}, "no vocabulary token"),
    ([[2]], dict(threshold=-0.5), "threshold"), ([[2]], dict(threshold=math.nan), "threshold"),
    ([[2]], dict(threshold=math.inf), "threshold"), ([[2]], dict(threshold="1"), "threshold"),
    ([[2]], dict(threshold=None, thresholds=[1.0, 2.0]), "1 phrases"), ([[2]], dict(thresholds=[1.0]), "not both"),
    ([[2]], dict(threshold=None, thresholds=[-1.0]), "threshold"),
], ids=str)
def test_refusals(phrases, kw, word):
    with pytest.raises(ValueError, match=word):
        Keywords(phrases, CTCAligner(VOCAB, 0), **{"threshold": 1.0, **kw})


def test_refusals_without_a_tokenizer():
    with pytest.raises(ValueError, match="no tokenizer"):
        Keywords(["ab"], blank_id=0, vocab_size=8, threshold=1.0)
    with pytest.raises(ValueError, match="blank_id"):
        Keywords([[2]], vocab_size=8, threshold=1.0)
    with pytest.raises(ValueError, match="do not go together"):
        Keywords([[2]], blank_id=8, vocab_size=8, threshold=1.0)
    with pytest.raises(ValueError, match="come from the tokenizer"):
        Keywords([[2]], CTCAligner(VOCAB, 0), blank_id=0, threshold=1.0)


def test_packing():
    long = [2 + (i % 5) for i in range(32)]                   # 2 3 4 5 6 2 3 ...: no repeated neighbour
    kw = Keywords([long, [3], [4, 4, 5], [6]], blank_id=0, vocab_size=8, threshold=1.0)
    assert kw.packing == [(0, 0, 0), (1, 0, 63), (2, 1, 0), (3, 1, 5)] and kw.G == 2 and kw.lanes.shape == (2, 3, 64)
    label, index, flags = kw.lanes[0]
    assert label[:63:2].tolist() == long and (label[1:63:2] == 0).all() and label[63] == 3        # 32 tokens take 63 lanes
    assert (index[:63] == 0).all() and index[63] == 1                                             # a 1-token keyword in lane 63
    assert flags[0] == FLAG_FIRST and flags[1] == 0 and (flags[2:62:2] == FLAG_SKIP).all() and (flags[1:63:2] == 0).all()
    assert flags[62] == FLAG_SKIP | FLAG_LAST and flags[63] == FLAG_FIRST | FLAG_LAST
    label, index, flags = kw.lanes[1]                                                             # the next opens a new group
    assert label[:6].tolist() == [4, 0, 4, 0, 5, 6] and index[:6].tolist() == [2, 2, 2, 2, 2, 3]
    assert flags[:6].tolist() == [FLAG_FIRST, 0, 0, 0, FLAG_SKIP | FLAG_LAST, FLAG_FIRST | FLAG_LAST]   # no skip over a repeat
    assert (label[6:] == -1).all() and (index[6:] == -1).all() and (flags[6:] == 0).all()         # idle lanes
    many = Keywords([[2 + i % 6, 2 + i // 6] for i in range(30)], blank_id=0, vocab_size=8, threshold=1.0)
    assert many.G == 2 and many.packing[20:23] == [(20, 0, 60), (21, 1, 0), (22, 1, 3)]           # 21 keywords of 3 lanes fit


# ---- the restatement's own properties ------------------------------------------------------------------------------------------
BLANK, V = 0, 12
KW = [[3], [4, 5], [6, 6, 7], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]]
THR = [np.float32(-1.0 * len(k)) for k in KW]


def _planted():
    plants = [(10, R.spell(KW[0], BLANK, 2)), (30, R.spell(KW[1], BLANK, 2)), (60, R.spell(KW[2], BLANK, 2)),
              (100, R.spell(KW[3], BLANK, 1)), (150, R.spell(KW[1], BLANK, 1)), (152, R.spell(KW[1], BLANK, 1))]
    return R.peaky(7, 200, V, BLANK, plants), plants


def test_a_planted_keyword_scores_exactly_zero_with_its_start_and_end():
    x, plants = _planted()
    found = R.run(x, KW, BLANK, THR).finish()
    assert (0, 10, 11, 0.0) in found and (1, 30, 33, 0.0) in found and (2, 60, 66, 0.0) in found and (3, 100, 109, 0.0) in found
    assert all(isinstance(d[3], np.float32) and d[3] <= 0 for d in found)
    assert [d[:3] for d in found if d[0] == 3] == [(3, 100, 109)]


def test_back_to_back_occurrences_are_two_detections():
    x, _ = _planted()
    st = R.run(x, KW, BLANK, THR)
    assert [d for d in st.finish() if d[0] == 1 and d[1] >= 150] == [(1, 150, 151, 0.0), (1, 152, 153, 0.0)]
    assert (1, 150, 151, 0.0) in st.emissions                  # emitted by the frame behind it, not at the stream's end
    assert not np.signbit(st.finish()[0][3])


def test_a_later_start_emits_the_held_detection_while_every_frame_qualifies():
    """rule 1 of the detector: a threshold so loose that every frame qualifies; a one-token keyword that is the argmax at
    frames 0 and 2 only"""
    x = R.peaky(3, 4, V, BLANK, [(0, [3]), (2, [3])])
    st = R.Stream([[3]], BLANK, [np.float32(-100.0)])
    st.push(x[:2])
    assert st.emissions == [] and st.held() == [(0, 0, 0, 0.0)]                    # frame 1 qualifies, but is worse
    st.push(x[2:3])
    assert st.emissions == [(0, 0, 0, 0.0)] and st.held() == [(0, 2, 2, 0.0)]      # start 2 > end 0
    st.push(x[3:])
    assert st.held() == [(0, 2, 2, 0.0)] and len(st.emissions) == 1


@pytest.mark.parametrize("chunks", [[1] * 200, [1, 7, 64, 65, 63], [199, 1]], ids=str)
def test_restatement_chunk_invariance(chunks):
    x, _ = _planted()
    whole, cut = R.run(x, KW, BLANK, THR), R.run(x, KW, BLANK, THR, chunks)
    assert cut.emissions == whole.emissions and cut.held() == whole.held() and len(whole.emissions) >= 6
    for a, b in zip(whole.kw, cut.kw):
        assert np.array_equal(a.a.view(np.int32), b.a.view(np.int32)) and np.array_equal(a.start, b.start)


def test_restatement_breaks_and_nans():
    x, _ = _planted()
    x[31, 2] = math.nan                                        # elsewhere in the row: ignored
    x[61, 6] = math.nan                                        # on a label: -inf for the states that carry it
    x[104] = math.nan                                          # a BREAK in the middle of the long keyword
    st = R.run(x, KW, BLANK, THR)
    found = st.finish()
    assert (1, 30, 33, 0.0) in found and np.isnan(st.rowmax[104]) and st.rowmax[31] == x[31, 4]
    assert not [d for d in found if d[1] <= 104 <= d[2]]
    at61 = R.run(x[:62], KW, BLANK, THR).kw[2]
    assert np.isneginf(at61.a[[0, 2]]).all() and np.isfinite(at61.a[[1, 3, 4]]).all()
    assert np.isnan(R.row_max([math.inf, 1.0])) and np.isnan(R.row_max([-math.inf] * 3)) and R.row_max([math.nan, -2.0]) == -2.0


def test_state_words_layout():
    kw = Keywords(KW, blank_id=BLANK, vocab_size=V, thresholds=[1.0] * 4)
    x, _ = _planted()
    st = R.run(x[:34], KW, BLANK, kw.thresholds)
    w = R.state_words(st, kw.packing, 0)
    assert w.shape == (8, 64) and w[6, 0] == 34 and (w[6, 1:] == 0).all() and (w[7] == 0).all()
    assert w[2, 3] == 1 and w[3:5, 3].tolist() == [30, 33] and w[5, 3] == 0        # keyword 1 holds (30, 33, 0.0) at its last lane
    assert (w[2, :3] == 0).all() and w[0, 3] == 0 and w[1, 3] == 30
    assert w[2:5, 0].tolist() == [0, 10, 11]                   # keyword 0's detection was emitted: dropped, its words stay
    assert (w[0, 28:] == np.float32(-np.inf).view(np.int32)).all() and (w[1:6, 28:] == 0).all()


# ---- suppress_overlaps ---------------------------------------------------------------------------------------------------------
def _d(q, a, b, score):
    return Detection(q, str(q), a * 0.04, b * 0.04, score, a, b)


def test_suppress_overlaps():
    ds = [_d(0, 0, 10, -1.0), _d(0, 5, 15, -0.5), _d(0, 15, 20, -2.0), _d(1, 6, 12, -3.0), _d(0, 18, 30, -2.0), _d(0, 40, 41, -9.0)]
    assert suppress_overlaps(ds) == [_d(1, 6, 12, -3.0), _d(0, 5, 15, -0.5), _d(0, 15, 20, -2.0), _d(0, 40, 41, -9.0)]
    assert suppress_overlaps([]) == [] and suppress_overlaps(ds[:1]) == ds[:1]
    chain = [_d(0, 0, 10, -3.0), _d(0, 8, 18, -1.0), _d(0, 16, 26, -2.0)]          # the middle one wins and both others go
    assert suppress_overlaps(chain) == [chain[1]]
