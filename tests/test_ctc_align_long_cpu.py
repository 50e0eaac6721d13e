"""Long-form CTC forced alignment, the parts that need no GPU: the host planning of the C entries (workspace size, launch
count, argument checks: they return before any HIP call), the Python refusals and `longform.cut_utterances`."""
import ctypes
import math
import os

import pytest
import torch

from conformer_amd import _lib
from conformer_amd import align as A
from conformer_amd.align import Word
from conformer_amd.longform import Utterance, cut_utterances


@pytest.fixture(scope="module")
def lib():
    from conformer_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


def ceil_div(a, b):
    return -(-a // b)


def test_limits_come_from_the_header():
    assert A.LONG_MAX_FRAMES == 1048576 and A.LONG_MAX_TARGET == 262143
    assert A.MAX_FRAMES == 16384 and A.MAX_TARGET == 4096                # the first generation keeps its own


def test_workspace_bytes(lib):
    ws = lib.cfm2_ctc_align_long_workspace_bytes
    for bad in ((0, 10, 4, 512, 16), (2, 0, 4, 512, 16), (2, 10, 0, 512, 16), (-1, 10, 4, 512, 16), (65536, 10, 4, 512, 16),
                (1, 1048577, 4, 512, 16), (1, 10, 262144, 512, 16),
                (1, 10, 4, 511, 16), (1, 10, 4, 256, 16), (1, 10, 4, 8704, 16), (1, 10, 4, -512, 16), (1, 10, 4, 768, 16),
                (1, 10, 4, 512, 8), (1, 10, 4, 512, 24), (1, 10, 4, 512, 65552), (1, 10, 4, 512, -16)):
        assert ws(*bad) == 0, bad
    assert ws(1, 1048576, 4, 512, 65536) > 0 and ws(1, 16, 262143, 8192, 16) > 0 and ws(65535, 1, 1, 0, 0) > 0
    # the moves: 2 bits per (frame, state) over whole tiles; then a float64 per frame, the carries and the edge columns
    for B, T, L, tp, cf in [(1, 1, 1, 512, 16), (3, 1400, 1100, 512, 64), (1, 3000, 600, 512, 16), (2, 17000, 4200, 2048, 512),
                            (1, 90000, 30000, 1024, 256), (1, 90000, 30000, 8192, 65536)]:
        n_tiles = ceil_div(L + 1, tp)
        moves = B * T * n_tiles * tp // 2
        n = ws(B, T, L, tp, cf)
        assert n >= moves + B * T * 8 + B * n_tiles * (2 * tp + T) * 8, (B, T, L, tp, cf, n)
        assert n <= moves + B * T * 8 + B * n_tiles * (2 * tp + T) * 8 + 8 * B + 64
        assert n == ws(B, T, L, tp, 16)                                   # the chunk length costs no memory
    for tp in (512, 2048):                                                # monotone in T
        sizes = [ws(1, T, 3000, tp, 64) for T in (1, 15, 16, 17, 1000, 16384, 16385, 100000)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    # the defaults: some accepted pair, cut down to the shape
    assert ws(1, 90000, 30000, 0, 0) in {ws(1, 90000, 30000, tp, 16) for tp in range(512, 8193, 512)}
    assert ws(1, 40, 7, 0, 0) == ws(1, 40, 7, 512, 48)


def test_launches(lib):
    n = lib.cfm2_ctc_align_long_launches
    for T, L, tp, cf in [(1, 1, 512, 16), (1400, 1100, 512, 64), (3000, 600, 512, 16), (1200, 511, 512, 64), (1200, 512, 512, 64),
                         (2048, 1500, 2048, 2048), (2048, 1500, 1024, 256), (16384, 4096, 512, 512), (90000, 30000, 1024, 256),
                         (90000, 10000, 8192, 4096), (1048576, 262143, 8192, 65536), (600, 520, 512, 64)]:
        assert n(T, L, tp, cf) == ceil_div(L + 1, tp) + ceil_div(T, cf) - 1, (T, L, tp, cf)
    assert n(1400, 1100, 512, 64) == 3 + 22 - 1
    assert n(0, 4, 512, 16) == 0 and n(10, 0, 512, 16) == 0 and n(10, 4, 100, 16) == 0 and n(10, 4, 512, 20) == 0
    assert n(40, 7, 0, 0) == 1 and n(90000, 30000, 0, 0) > 1


def test_argument_validation_without_gpu(lib):
    buf = (ctypes.c_double * 8192)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    n = lib.cfm2_ctc_align_long_workspace_bytes(2, 8, 3, 512, 16)
    assert 0 < n < 8192 * 8 - 16
    good = [a, a, None, None, 2, 8, 5, 3, 0, 512, 16, a, n, a, a, a, a, a, a, a, None]

    def call(**kw):
        args = list(good)
        for k, v in kw.items():
            args[int(k[1:])] = v
        return lib.cfm2_ctc_align_long_f32(*args)

    for i in (0, 1, 11, 13, 14, 15, 16, 17, 18, 19):
        assert call(**{f"a{i}": None}) == -3, i                                    # NULL
    assert call(a4=0) == -1 and call(a5=0) == -1 and call(a6=1) == -1 and call(a7=0) == -1      # B, T, V, Lmax
    assert call(a8=-1) == -1 and call(a8=5) == -1                                   # blank_id outside [0,V)
    assert call(a5=1048577) == -2 and call(a7=262144) == -2 and call(a4=65536) == -2            # beyond the limits
    for tp in (1, 511, 768, 8704, -512):
        assert call(a9=tp) == -2, tp                                                # bad tile_pairs
    for cf in (1, 8, 24, 65552, -16):
        assert call(a10=cf) == -2, cf                                               # bad chunk_frames
    assert call(a11=a + 8) == _lib.CONSTANTS["CFM_ERR_ALIGN"]                       # misaligned workspace
    assert call(a12=n - 1) == -1                                                    # workspace too small
    assert call(a11=a + 8, a12=n - 1) == _lib.CONSTANTS["CFM_ERR_ALIGN"]            # in the order of cfm_ctc_align_f32
    assert call(a0=None, a4=0) == -3 and call(a4=0, a5=1048577) == -1 and call(a5=1048577, a11=a + 8) == -2
    # the chain-only entry: the same refusals for the arguments it has
    chain = [a, a, None, None, 2, 8, 5, 3, 0, 512, 16, a, n, None]
    for i, v, want in ((0, None, -3), (11, None, -3), (4, 0, -1), (8, 5, -1), (5, 1048577, -2), (9, 500, -2), (12, n - 1, -1)):
        args = list(chain)
        args[i] = v
        assert lib.cfm2_ctc_align_long_chain_f32(*args) == want, i


def test_no_cpu_path():
    from conformer_amd._lib import ConformerHipError
    with pytest.raises(ConformerHipError):
        A.ctc_forced_align_long(torch.zeros(1, 4, 3), torch.ones(1, 2, dtype=torch.int64), 0)
    with pytest.raises(ConformerHipError):
        A.CTCAligner(["_", "a", "b"], 0)(torch.zeros(1, 4, 3), ["ab"], long=True)


def test_workspace_refusals():
    moves = 90000 * ceil_div(30001, 1024) * 1024 // 2                               # INTEGRATION.md's formula
    n = A.long_workspace_bytes(1, 90000, 30000, 1024, 256)
    assert moves <= n <= moves + (64 << 20)
    with pytest.raises(ValueError, match=rf"needs a workspace of {n} bytes, max_workspace_bytes is {1 << 30}"):
        A.long_workspace_bytes(1, 90000, 30000, 1024, 256, max_workspace_bytes=1 << 30)
    assert A.long_workspace_bytes(1, 90000, 30000, 1024, 256, max_workspace_bytes=n) == n
    with pytest.raises(ValueError, match="needs a workspace"):
        A.long_workspace_bytes(4, 1048576, 262143)                                  # beyond the default 16 GiB
    for kw in (dict(tile_pairs=500), dict(tile_pairs=0), dict(tile_pairs=16384), dict(chunk_frames=8), dict(chunk_frames=0),
               dict(chunk_frames=100)):
        with pytest.raises(ValueError, match="tile_pairs must be a multiple of 512"):
            A.long_workspace_bytes(1, 100, 10, **kw)
    with pytest.raises(ValueError, match="unsupported shape"):
        A.long_workspace_bytes(1, A.LONG_MAX_FRAMES + 1, 10)


# ---- cut_utterances ---------------------------------------------------------------------------------------------------------

def W(text, start, end, score=-1.0, fps=25):
    return Word(text, round(start * fps), round(end * fps), float(start), float(end), score)


def spans(us):
    return [(u.first_word, u.last_word) for u in us]


def test_cut_at_gaps():
    ws = [W("a", 0.0, 0.4), W("b", 0.5, 1.0), W("c", 2.0, 2.4), W("d", 2.5, 3.0), W("e", 4.0, 4.4)]
    us = cut_utterances(ws, 10.0, 1.0)
    assert spans(us) == [(0, 1), (2, 3), (4, 4)]                                    # a gap of exactly min_gap splits
    assert us[0] == Utterance(0.0, 1.0, "a b", -1.0, 0, 1) and us[1].text == "c d" and (us[2].start, us[2].end) == (4.0, 4.4)
    assert spans(cut_utterances(ws, 10.0, 1.01)) == [(0, 4)]
    assert spans(cut_utterances(ws, 10.0, 0.05)) == [(i, i) for i in range(5)]
    assert cut_utterances([], 10.0, 1.0) == []
    assert spans(cut_utterances(ws[:1], 10.0, 1.0)) == [(0, 0)]


def test_forced_cut_takes_the_earliest_of_the_largest_gaps():
    # one piece of 4.5 s; internal gaps 0.25, 0.5, 0.5, 0.25 (binary fractions: the two 0.5 tie exactly)
    ws = [W("a", 0.0, 0.5), W("b", 0.75, 1.25), W("c", 1.75, 2.25), W("d", 2.75, 3.25), W("e", 3.5, 4.5)]
    assert spans(cut_utterances(ws, 5.0, 9.0)) == [(0, 4)]
    assert spans(cut_utterances(ws, 4.0, 9.0)) == [(0, 1), (2, 4)]                  # the earlier 0.5: after b, not after c
    assert spans(cut_utterances(ws, 2.0, 9.0)) == [(0, 1), (2, 2), (3, 4)]          # c-e is 2.75 s: cut again at its 0.5
    assert spans(cut_utterances(ws, 1.25, 9.0)) == [(0, 1), (2, 2), (3, 3), (4, 4)]  # d-e is 1.75 s; a-b is 1.25 s: it fits
    us = cut_utterances(ws, 0.1, 9.0)                                               # nothing fits: single words stand
    assert spans(us) == [(i, i) for i in range(5)] and [u.text for u in us] == list("abcde")


def test_a_single_word_longer_than_the_maximum_stands():
    ws = [W("loooong", 0.0, 7.0), W("b", 7.5, 8.0), W("c", 8.25, 8.5)]
    us = cut_utterances(ws, 2.0, 5.0)
    assert spans(us) == [(0, 0), (1, 2)] and us[0].end - us[0].start == 7.0 and us[1].text == "b c"


def test_utterance_score_is_frame_weighted():
    ws = [W("a", 0.0, 0.4, -1.0), W("b", 0.4, 2.0, -2.0), W("c", 9.0, 9.2, -0.5)]
    us = cut_utterances(ws, 10.0, 1.0)
    assert spans(us) == [(0, 1), (2, 2)]
    assert us[0].score == pytest.approx((-1.0 * 10 + -2.0 * 40) / 50) and us[1].score == -0.5
    assert us[0].text == "a b" and (us[0].start, us[0].end) == (0.0, 2.0)


def test_cut_utterances_refuses_bad_limits():
    for kw in (dict(max_seconds=0.0, min_gap_seconds=1.0), dict(max_seconds=1.0, min_gap_seconds=-1.0),
               dict(max_seconds=math.inf, min_gap_seconds=1.0), dict(max_seconds=True, min_gap_seconds=1.0),
               dict(max_seconds="3", min_gap_seconds=1.0), dict(max_seconds=1.0, min_gap_seconds=math.nan)):
        with pytest.raises(ValueError, match="cut_utterances"):
            cut_utterances([W("a", 0.0, 1.0)], **kw)


# ---- Transcriber.align, what needs no device --------------------------------------------------------------------------------

def test_transcriber_align_refusals(monkeypatch):
    """Transcriber.__init__ needs a model on the device, so the method runs on a bare object that carries what it reads before
    any tensor is touched (the model check is stood in for): the argument checks come before the front end and the encoder."""
    from conformer_amd import longform
    from conformer_amd.decode import BeamCTCDecoder
    vocab = ["<pad>", "a", "b", "|", "<unk>"]
    tr = longform.Transcriber.__new__(longform.Transcriber)
    tr.decoder, tr.frame_seconds, tr.model = BeamCTCDecoder(vocab, 0, skip_ids=(4,)), 0.04, None
    monkeypatch.setattr(longform, "lstm_state", lambda *a, **kw: (torch.device("cpu"), None))
    mel = torch.zeros(80, 40)
    with pytest.raises(ValueError, match="one text per recording, got 1 recordings and a single string"):
        tr.align([mel], "ab")
    with pytest.raises(ValueError, match="one text per recording, got 2 recordings and 1 texts"):
        tr.align([mel, mel], ["ab"])
    with pytest.raises(ValueError, match="no vocabulary token spells 'x'"):
        tr.align([mel], ["axb"])
    with pytest.raises(ValueError, match="blank id"):
        tr.align([mel], [[1, 0, 2]])
    assert tr.align([], []) == []
