"""conformer_amd/longform.py on the host: the window plan over every admissible (window, hop, length) up to window = 133, against
the independent per-frame restatement (tests/longform_restatement.py), the seconds-to-frames conversion, and the refusals of
window_plan, window_frames, BufferedEncoder and Transcriber that need no device."""
import math

import pytest
import torch

from conformer_amd.confidence import ConfidenceConfig
from conformer_amd.decode import BeamCTCDecoder
from conformer_amd.longform import BufferedEncoder, Transcriber, Transcript, Window, check_window, window_frames, window_plan
from conformer_amd.streaming import encoder_frames
from tests import longform_restatement as R

VOCAB = ["<pad>", "a", "b", "c", "|", "<unk>"]


def _admissible(W):
    return [H for H in range(4, W + 1, 4) if W >= 12 and R.ef(W) >= H // 4]


def test_plan_sweep_tiles_exactly_once():
    """W in 7 .. 133, every admissible hop H (a multiple of 4, >= 4, no gap), n_mel in 7 .. 4W + 8: 756 948 plans.  The kept
    ranges tile [0, ef(n_mel)) exactly once, every kept range lies inside its window, starts are strictly increasing multiples
    of 4 with first == start / 4, the last window ends at ef(n_mel) and is W - 3 .. W long, every other window is W long."""
    plans = 0
    for W in range(7, 134):
        hops = _admissible(W)
        assert hops or W < 12
        for H in hops:
            for n in range(7, 4 * W + 9):
                p = window_plan(n, W, W - H)
                plans += 1
                total = R.ef(n)
                assert p[0].start == 0 and p[0].keep_from == 0 and p[-1].keep_to == total
                assert p[-1].start + p[-1].mel == n and p[-1].first + R.ef(p[-1].mel) == total
                if len(p) == 1:
                    assert n <= W and p[0].mel == n
                else:
                    assert n > W and len(p) == -(-(n - W) // H) + 1 and W - 3 <= p[-1].mel <= W
                for i, w in enumerate(p):
                    assert w.start % 4 == 0 and w.first == w.start // 4
                    assert w.first <= w.keep_from <= w.keep_to <= w.first + R.ef(w.mel), (n, W, H, w)
                    if i + 1 < len(p):
                        assert w.mel == W and w.start == i * H
                        assert w.keep_to == p[i + 1].keep_from and w.start < p[i + 1].start
    assert plans == 756948


@pytest.mark.parametrize("W", [12, 13, 14, 15, 16, 17, 19, 22, 27, 31, 32, 40, 64, 133])
def test_plan_is_the_restated_plan_and_keeps_the_best_window(W):
    """Against the restatement: the same windows and cuts, and every frame is kept from a window in which it is farthest from
    both window edges (one of them at a tie)."""
    for H in _admissible(W):
        for n in range(7, 4 * W + 9):
            p = window_plan(n, W, W - H)
            assert [(w.start, w.mel) for w in p] == R.spans(n, W, W - H)
            assert [(w.keep_from, w.keep_to) for w in p] == R.kept(n, W, W - H)
            best = R.best_windows(n, W, W - H)
            for i, w in enumerate(p):
                for g in range(w.keep_from, w.keep_to):
                    assert i in best[g], (n, W, H, g, i, best[g])


def test_the_issue_example():
    p = window_plan(403, 64, 24)
    assert len(p) == 10 and p[-1] == Window(340, 63, 85, 90, 100)
    assert [(w.keep_from, w.keep_to) for w in p] == [(0, 12)] + [(12 + 10 * i, 22 + 10 * i) for i in range(7)] + [(82, 90), (90, 100)]
    assert [(w.start, w.mel) for w in window_plan(67, 64, 24)] == [(0, 64), (4, 63)]
    assert window_plan(64, 64, 24) == [Window(0, 64, 0, 0, 15)] and window_plan(7, 64, 24) == [Window(0, 7, 0, 0, 1)]


@pytest.mark.parametrize("n_mel,W,O", [(100, 11, 3), (100, 7, 3), (100, 64, 61), (100, 64, 64), (100, 64, 70), (100, 64, 22),
                                       (100, 64, 25), (100, 12, 0), (100, 13, 1), (6, 64, 24), (0, 64, 24), (-5, 64, 24),
                                       (100.0, 64, 24), (100, 64.0, 24), (100, 64, 24.0), (True, 64, 24)])
def test_plan_refusals(n_mel, W, O):
    """W < 12; H < 4 (also 0 and negative); H % 4 != 0; ef(W) < H / 4 (W = 12 makes 2 frames, H = 12 needs 3; W = 13, H = 12);
    n_mel < 7; and what is no integer."""
    with pytest.raises(ValueError):
        window_plan(n_mel, W, O)


def test_the_smallest_windows_pass():
    assert len(window_plan(100, 12, 4)) == 12 and check_window(12, 4) == (12, 8)
    assert encoder_frames(15) == 3 and len(window_plan(100, 15, 3)) == 9          # ef(W) == H / 4 exactly: no gap, no overlap
    for p in (window_plan(100, 12, 4), window_plan(100, 15, 3)):
        assert [w.keep_from for w in p[1:]] == [w.keep_to for w in p[:-1]]


def test_seconds_to_frames():
    """30 s / 8 s at the front end's 10 ms hop: W = 3000, H = 2200 = 4 * 550, overlap 800; the hop is rounded DOWN to a multiple
    of 4, so the overlap only grows."""
    assert window_frames(30.0, 8.0, 160 / 16000) == (3000, 800)
    assert window_frames(30.0, 8.0, 0.04 / 4) == (3000, 800)
    assert window_frames(30, 8.01, 0.01) == (3000, 804)                         # least overlap 801 -> H = 2199 -> 2196
    assert window_frames(30.0, 7.99, 0.01) == (3000, 800)                       # least overlap 799 -> H = 2201 -> 2200
    assert window_frames(0.64, 0.24, 0.01) == (64, 24)
    assert window_frames(0.649, 0.04, 0.01) == (64, 4)                          # whole frames inside the window; H = 60 = 4 ef(64)
    assert window_frames(20.0, 5.0, 256 / 22050)[0] == int(20.0 * 22050 / 256)
    for W, O in ((3000, 800), (64, 24), (1722, window_frames(20.0, 5.0, 256 / 22050)[1])):
        assert (W - O) % 4 == 0
    for w, o, hop in ((30.0, 8.0, 0.01), (12.5, 1.234, 0.0125), (5.0, 4.9, 0.01)):
        W, O = window_frames(w, o, hop)
        assert O * hop >= o - 1e-9 and (O - 4) * hop < o + 1e-9 and W * hop <= w + 1e-9 < (W + 1) * hop + 1e-9


@pytest.mark.parametrize("w,o,hop", [(0.0, 0.0, 0.01), (-1.0, 0.0, 0.01), (30.0, -1.0, 0.01), (30.0, 30.0, 0.01), (30.0, 31.0, 0.01),
                                     (math.inf, 8.0, 0.01), (30.0, math.nan, 0.01), (30.0, 8.0, 0.0), ("30", 8.0, 0.01),
                                     (True, 0.0, 0.01), (0.11, 0.0, 0.01), (30.0, 29.97, 0.01), (0.64, 0.0, 0.01)])
def test_seconds_to_frames_refusals(w, o, hop):
    """no positive finite time; overlap >= window; then window_plan's own: W = 11 < 12, H = 3 < 4, H = 64 with ef(64) = 15 < 16"""
    with pytest.raises(ValueError):
        window_frames(w, o, hop)


def _cpu_model(train=False):
    from conformer_amd.model.conformer import Conformer
    m = Conformer(len(VOCAB), 80, 1, 32, 4, 7, 8, 1, 0.0)
    return m.train() if train else m.eval()


def test_transcriber_refusals_on_the_host():
    dec = BeamCTCDecoder(VOCAB, 0, skip_ids=[5])
    m = _cpu_model()
    ok = dict(window_seconds=30.0, overlap_seconds=8.0)
    with pytest.raises(TypeError):
        Transcriber(m, dec)                                                      # the two window arguments have no default
    with pytest.raises(TypeError):
        Transcriber(m, dec, None, 30.0, 8.0)                                     # and are keywords
    for kw in (dict(times=1), dict(frame_seconds=0.0), dict(frame_seconds=True), dict(confidence=ConfidenceConfig()),
               dict(times=True, confidence="tsallis"), dict(times=True, confidence=ConfidenceConfig(method="softmax")),
               dict(batch_windows=0), dict(batch_windows=2.0), dict(graphs=1)):
        with pytest.raises(ValueError):
            Transcriber(m, dec, **ok, **kw)
    for kw in (dict(window_seconds=0.11, overlap_seconds=0.0), dict(window_seconds=8.0, overlap_seconds=8.0),
               dict(window_seconds=30.0, overlap_seconds=29.97)):
        with pytest.raises(ValueError):
            Transcriber(m, dec, **kw)
    with pytest.raises(ValueError):
        Transcriber(m, "decoder", **ok)
    with pytest.raises(ValueError):
        Transcriber(m, dec, object(), **ok)
    with pytest.raises(RuntimeError, match="HIP device"):
        Transcriber(m, dec, **ok)                                                # a CPU model: no CPU fallback
    with pytest.raises(RuntimeError, match="eval"):
        Transcriber(_cpu_model(train=True), dec, **ok)


def test_buffered_encoder_refusals_on_the_host():
    m = _cpu_model()
    for args in ((11, 3), (64, 61), (64, 22), (12, 0)):
        with pytest.raises(ValueError):
            BufferedEncoder(m.encoder, *args)
    for kw in (dict(batch_windows=0), dict(batch_windows=True), dict(graphs=None)):
        with pytest.raises(ValueError):
            BufferedEncoder(m.encoder, 64, 24, **kw)
    with pytest.raises(RuntimeError, match="HIP device"):
        BufferedEncoder(m.encoder, 64, 24)
    with pytest.raises(RuntimeError, match="eval"):
        BufferedEncoder(_cpu_model(train=True).encoder, 64, 24)


def test_transcript_fields():
    assert Transcript._fields == ("text", "words", "word_confidence", "frames", "seconds")


def test_ambient_autocast_other_than_none_bf16_fp16_is_refused():
    """torch.autocast("cuda") itself only takes bfloat16 and float16; any other ambient type is reached through the setters."""
    from conformer_amd.longform import _ambient_autocast
    keep = torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda")
    try:
        torch.set_autocast_enabled("cuda", False)
        assert _ambient_autocast("BufferedEncoder") is None
        torch.set_autocast_enabled("cuda", True)
        for dt in (torch.bfloat16, torch.float16):
            torch.set_autocast_dtype("cuda", dt)
            assert _ambient_autocast("BufferedEncoder") is dt
        for dt in (torch.float32, torch.float64):
            torch.set_autocast_dtype("cuda", dt)
            with pytest.raises(RuntimeError, match="no gfx950 path"):
                _ambient_autocast("BufferedEncoder")
    finally:
        torch.set_autocast_enabled("cuda", keep[0])
        torch.set_autocast_dtype("cuda", keep[1])
