"""Long-form transcription behind the voice activity detector (Transcriber(vad=...), conformer_amd/longform.py) on the MI355X.

The tiny model and decoder of tests/test_longform_gpu.py, log-mel inputs (frontend=None, 0.01 s per mel frame), window = 64 and
overlap = 24 mel frames.  The recordings are Gaussian frames at a low level with louder stretches, 6 nats above it against an
snr of 3: every decision is far from its threshold, so the float64 restatement's segments are the device's."""
import math
import sys

import pytest
import torch

import conformer_amd
from conformer_amd import _lib
from conformer_amd.confidence import ConfidenceConfig, frame_confidence, word_confidence
from conformer_amd.longform import BufferedEncoder, Transcriber, Transcript, window_plan
from conformer_amd.vad import VadConfig, speech_islands
from tests import vad_restatement as R
from tests.test_stream_slots_gpu import _decoder, _model

pytestmark = pytest.mark.gpu

W, OV = 64, 24
SNR = 3.0
VAD = VadConfig(SNR * 10.0 / math.log(10.0), None, 5.0, 0.03, 0.03, 0.05)        # pads 0.2 s, min_gap 0.5 s: the defaults
KW = dict(smooth=3, noise_window=500, snr=SNR, min_energy=-math.inf, onset=3, hangover=5)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _recording(n, loud, seed):
    """(80, n) fp32: Gaussian frames at -6; in the stretches of `loud` frames around 0 whose spectral shape changes every 10
    frames (the random model writes several words of those; stationary noise gives one)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(80, n, generator=g) - 6.0
    for a, b in loud:
        for s in range(a, b, 10):
            e = min(b, s + 10)
            x[:, s:e] = 3.0 * torch.randn(80, 1, generator=g) + 0.3 * torch.randn(80, e - s, generator=g)
    return x


def _transcriber(dev, vad, **kw):
    m, _ = _model(32, 4, 71, dev)
    return Transcriber(m, _decoder("plain", None), window_seconds=0.64, overlap_seconds=0.24, vad=vad, **kw), m


def _islands(x):
    p = VAD.check(0.01, 80)
    assert (p.smooth, p.noise_window, p.onset, p.hangover, p.snr) == (3, 500, 3, 5, pytest.approx(SNR, abs=1e-12))
    st, _, _, margins = R.run(x.numpy(), **KW)
    assert margins[:, 0].min() > 0.5
    return speech_islands(st.finish(), x.shape[1], p.pad_before, p.pad_after, p.min_gap)


def test_one_island_over_the_whole_recording_changes_nothing(dev):
    x = _recording(403, [(4, 393)], 1)
    assert _islands(x) == [(0, 403)]
    cfg = ConfidenceConfig()
    with_vad, _ = _transcriber(dev, VAD, times=True, confidence=cfg)
    without, _ = _transcriber(dev, None, times=True, confidence=cfg)
    assert (with_vad.window, with_vad.overlap) == (W, OV)
    assert with_vad.speech([x.to(dev)]) == [[(0.0, 403 * 0.01)]]
    got, want = with_vad.transcribe([x.to(dev)])[0], without.transcribe([x.to(dev)])[0]
    assert got.text == want.text and got.words == want.words and got.frames == want.frames == 100 and got.seconds == want.seconds
    assert len(got.word_confidence) == len(want.word_confidence) == len(want.words) > 0
    assert all(a == b or (a != a and b != b) for a, b in zip(got.word_confidence, want.word_confidence))
    assert isinstance(got, Transcript)


def test_two_bursts_are_two_islands(dev, monkeypatch):
    x = _recording(800, [(100, 180), (500, 640)], 4)        # (a seed at which the random model starts a word in the second burst)
    islands = _islands(x)
    assert islands == [(80, 200), (480, 660)]
    cfg = ConfidenceConfig()
    tr, m = _transcriber(dev, VAD, times=True, confidence=cfg)
    dec = tr.decoder
    assert tr.speech([x.to(dev)]) == [[(a * 0.01, b * 0.01) for a, b in islands]]
    planned = []
    plan = BufferedEncoder.plan
    monkeypatch.setattr(BufferedEncoder, "plan", lambda self, n: planned.append(list(n)) or plan(self, n))
    got = tr.transcribe([x.to(dev)])[0]
    monkeypatch.undo()
    assert planned == [[120, 180]]                                           # one encode call, the islands as recordings
    windows = sum(len(window_plan(n, W, OV)) for n in planned[0])
    assert windows == 7 < len(window_plan(800, W, OV)) == 20
    # by hand: the island slices encoded, concatenated, head and search over the concatenation
    hs = BufferedEncoder(m.encoder, W, OV).encode([x[:, a:b].to(dev) for a, b in islands])
    n = [h.shape[0] for h in hs]
    assert n == [29, 44]
    h = torch.cat(hs)[None]
    t = torch.tensor([sum(n)], device=dev)
    with torch.no_grad():
        logits = m.decoder(h, t)
    text, words = dec(logits, t)[0], dec.words(logits, t, 0.04)
    conf, ids = frame_confidence(logits, t, cfg)
    scores = word_confidence(words, conf, ids, dec.blank_id, t, cfg)[0]
    assert got.text == text and got.frames == sum(n) and abs(got.seconds - 8.0) < 1e-9 and len(got.words) == len(words[0]) > 0
    assert all(a == b or (a != a and b != b) for a, b in zip(got.word_confidence, scores))

    def to_global(c):
        return 80 // 4 + c if c < n[0] else 480 // 4 + c - n[0]

    second = 0
    print(f"island frames {n}: {[(w.text, w.start_frame, w.end_frame) for w in words[0]]} -> "
          f"{[(g.start_frame, g.end_frame) for g in got.words]}")
    for g, w in zip(got.words, words[0]):
        assert (g.text, g.score) == (w.text, w.score)
        assert (g.start_frame, g.end_frame) == (to_global(w.start_frame), to_global(w.end_frame - 1) + 1)
        assert (g.start, g.end) == (g.start_frame * 0.04, g.end_frame * 0.04)
        if w.start_frame >= n[0]:
            second += 1
            assert g.start_frame >= 480 // 4
        else:
            assert 80 // 4 <= g.start_frame < 80 // 4 + n[0]
    assert second > 0


def test_a_recording_without_speech_is_an_empty_transcript(dev):
    quiet, spoken = _recording(300, [], 3), _recording(403, [(4, 393)], 1)
    assert _islands(quiet) == []
    tr, _ = _transcriber(dev, VAD, times=True, confidence=ConfidenceConfig())
    got = tr.transcribe([quiet.to(dev), spoken.to(dev), quiet[:, :7].to(dev)])
    assert got[0] == Transcript("", [], [], 0, 300 * 0.01) and got[2] == Transcript("", [], [], 0, 7 * 0.01)
    assert got[1].frames == 100 and got[1].text
    assert tr.speech([quiet.to(dev)]) == [[]]
    plain, _ = _transcriber(dev, VAD)
    assert plain.transcribe([quiet.to(dev)]) == [Transcript("", None, None, 0, 300 * 0.01)]
    with pytest.raises(ValueError, match="least is 7"):
        plain.transcribe([quiet[:, :6].to(dev)])


def test_without_vad_the_new_module_is_neither_imported_nor_called(dev, monkeypatch):
    x = _recording(200, [(40, 120)], 4).to(dev)
    called = []
    call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: called.append(name) or call(name, *a))
    monkeypatch.setitem(sys.modules, "conformer_amd.vad", None)                # an import of it would raise ImportError
    monkeypatch.delattr(conformer_amd, "vad")
    tr, _ = _transcriber(dev, None, times=True)
    assert tr.vad is None and tr.transcribe([x])[0].frames == 49
    with pytest.raises(ValueError, match="without vad="):
        tr.speech([x])
    assert called and not [name for name in called if "vad" in name]
    with pytest.raises(ImportError):
        _transcriber(dev, VAD)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="VadConfig or None"):
        _transcriber(dev, dict(snr_db=9.0))
    tr, _ = _transcriber(dev, VAD)
    monkeypatch.setattr(_lib, "call", lambda name, *a: called.append(name) or call(name, *a))
    del called[:]
    tr.transcribe([x])
    assert {"cfm3_vad_energy_f32", "cfm3_vad_scan_f32"} <= set(called)
