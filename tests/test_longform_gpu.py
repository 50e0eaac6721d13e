"""Offline and long-form transcription (conformer_amd/longform.py) on the MI355X.

A tiny encoder (n_mel 80, 2 blocks, d in {32, 64}, 4 heads, kernel 31 and 7) with window = 64 and overlap = 24 mel frames: a
recording of 403 frames makes 10 windows, the last one 63 frames long.  Pinned here: a list of short recordings is the offline
batch bit for bit; the windowed encoder against the float64 restatement (tests/longform_restatement.py: the oracle on every
batch as pooled and padded, stitched by the restated plan) and away from a full-context forward; each output row comes from the
window the plan names; pooling across recordings and batch sizes; graphs on against off, also after a weight update; bf16
autocast; Transcriber end to end against its stages called by hand; and the peak memory, which one batch of windows bounds."""
import math

import pytest
import torch

from conformer_amd.confidence import ConfidenceConfig, frame_confidence, word_confidence
from conformer_amd.frontend import ConformerAudioFrontend
from conformer_amd.longform import BufferedEncoder, Transcriber, window_plan
from oracle import conformer_oracle as O
from tests import longform_restatement as R
from tests.test_stream_slots_gpu import _decoder, _model
from tests.test_window_gpu import _encoder
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

W, OV, H, L = 64, 24, 4, 2
CASES = [(32, 31), (64, 7)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_PARAMS = {}


def _params(d, K):
    if (d, K) not in _PARAMS:
        _PARAMS[d, K] = O.make_params(vocab=8, n_mel=80, n_blocks=L, d=d, n_heads=H, ksize=K, lstm_hidden=8, seed=11,
                                      dtype=torch.float64, with_decoder=False)
    return _PARAMS[d, K]


def _mels(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(80, n, generator=g, dtype=torch.float64) for n in lengths]


def _on(mels, dev):
    return [m.float().to(dev) for m in mels]


def test_plan_of_the_test_shapes():
    p = window_plan(403, W, OV)
    assert len(p) == 10 and p[-1].mel == 63
    assert [(w.keep_from, w.keep_to) for w in p] == [(0, 12)] + [(12 + 10 * i, 22 + 10 * i) for i in range(7)] + [(82, 90), (90, 100)]


@pytest.mark.parametrize("d,K", CASES)
def test_short_recordings_are_the_offline_batch(dev, d, K):
    """Recordings that each fit one window: encoder(x_padded, lengths) on the batch sorted by length, bit for bit."""
    enc = _encoder(_params(d, K), L, d, H, K, dev)
    n = [30, 64, 7, 61, 64, 12]
    mels = _on(_mels(n, 21), dev)
    got = BufferedEncoder(enc, W, OV).encode(mels)
    order = sorted(range(len(n)), key=lambda i: -n[i])
    assert order == [1, 4, 3, 0, 5, 2]
    x = torch.zeros(len(n), 80, 64, device=dev)
    for k, i in enumerate(order):
        x[k, :, :n[i]] = mels[i]
    with torch.no_grad():
        want, out_len = enc(x, torch.tensor([n[i] for i in order], device=dev))
    assert out_len.tolist() == [R.ef(n[i]) for i in order]
    for k, i in enumerate(order):
        assert got[i].shape == (R.ef(n[i]), d) and torch.equal(got[i], want[k, :R.ef(n[i])]), i
    # one length only: the unpadded batch, encoder(x, None)
    same = _on(_mels([40, 40, 40], 22), dev)
    with torch.no_grad():
        want = enc(torch.stack(same), None)[0]
    assert all(torch.equal(g, w) for g, w in zip(BufferedEncoder(enc, W, OV).encode(same), want))


@pytest.mark.parametrize("d,K", CASES)
def test_windowed_encoder_vs_float64(dev, d, K):
    """403 (10 windows, the last 63 long), 64, 67 (windows of 64 and 63), 7 and 200 mel frames in batches of 5: three full batches of
    full windows, then the ragged batch 64, 63, 63, 7.  Bound: the one test_streaming_encoder_left_context_vs_windowed_float64 holds the
    encoder to at these sizes."""
    P = _params(d, K)
    enc = _encoder(P, L, d, H, K, dev)
    n = [403, 64, 67, 7, 200]
    mels = _mels(n, 4)
    assert [[m for *_, m in b] for b in R.batches(n, W, OV, 5)] == [[64] * 5] * 3 + [[64, 63, 63, 7]]
    ref = R.encode(mels, P, L, H, W, OV, 5)
    got = BufferedEncoder(enc, W, OV, batch_windows=5).encode(_on(mels, dev))
    for r, (g, w) in enumerate(zip(got, ref)):
        assert g.shape == w.shape == (R.ef(n[r]), d) and torch.isfinite(w).all()
        err = rel_l2(g, w)
        print(f"d={d} K={K} recording of {n[r]}: windowed vs float64 {err:.3g}")
        assert err < 2e-5, (r, err)
    full = O.encoder_forward(mels[0][None], None, P, L, H)[0][0]
    away = rel_l2(got[0], full)
    print(f"d={d} K={K}: windowed vs one full-context forward {away:.3g}")
    assert away > 1e-3                                                   # the windows really change the numbers
    assert rel_l2(got[1], O.encoder_forward(mels[1][None], None, P, L, H)[0][0]) < 2e-5     # one window IS full context


@pytest.mark.parametrize("j", [0, 4, 9])
def test_the_right_window_supplies_each_frame(dev, j):
    """Noise over the mel frames that window j alone reads: the rows kept from every other window stay bit for bit, every row
    kept from window j changes."""
    d, K = 32, 31
    enc = _encoder(_params(d, K), L, d, H, K, dev)
    x = _mels([403], 5)[0].float()
    plan = window_plan(403, W, OV)
    lo = 0 if j == 0 else plan[j - 1].start + plan[j - 1].mel            # behind the window before
    hi = 403 if j == 9 else plan[j + 1].start                            # up to the window after
    assert plan[j].start <= lo < hi <= plan[j].start + plan[j].mel
    for i, w in enumerate(plan):
        assert i == j or w.start + w.mel <= lo or w.start >= hi
    y = x.clone()
    y[:, lo:hi] = torch.randn(80, hi - lo, generator=torch.Generator().manual_seed(6)) * 2.0
    be = BufferedEncoder(enc, W, OV)
    a, b = be.encode([x.to(dev)])[0], be.encode([y.to(dev)])[0]
    for i, w in enumerate(plan):
        rows = slice(w.keep_from, w.keep_to)
        if i == j:
            assert w.keep_to > w.keep_from and bool((a[rows] != b[rows]).any(dim=1).all()), i
        else:
            assert torch.equal(a[rows], b[rows]), i


@pytest.mark.parametrize("d,K", CASES)
def test_pooling_across_recordings_and_batch_sizes(dev, d, K):
    """404 and 204 mel frames: (n_mel - 64) % 4 == 0, so every window is 64 long and no batch is padded.  Bound: the one the
    suite holds kernel paths to that differ by the batch size alone."""
    enc = _encoder(_params(d, K), L, d, H, K, dev)
    mels = _on(_mels([404, 204], 7), dev)
    assert all(w.mel == W for n in (404, 204) for w in window_plan(n, W, OV))
    alone = [BufferedEncoder(enc, W, OV).encode([m])[0] for m in mels]
    for bw in (1, 3, 32):
        both = BufferedEncoder(enc, W, OV, batch_windows=bw).encode(mels)
        for r in range(2):
            err = rel_l2(both[r], alone[r])
            print(f"d={d} K={K} batch_windows={bw} recording {r}: together vs alone {err:.3g}")
            assert both[r].shape == alone[r].shape and err <= 1e-6, (bw, r, err)
    one = BufferedEncoder(enc, W, OV, batch_windows=1)                   # every batch is one window either way: the same launches
    assert all(torch.equal(one.encode(mels)[r], one.encode([mels[r]])[0]) for r in range(2))


def test_graphs_on_equals_graphs_off(dev):
    """batch_windows = 2 over 404 + 67 mel frames: 11 windows of 64 (five full batches replay the graph) and the ragged batch
    64, 63 (eager).  Then every weight moves in place: the next call captures again and still equals the eager run."""
    d, K = 32, 31
    enc = _encoder(_params(d, K), L, d, H, K, dev)
    mels = _on(_mels([404, 67], 8), dev)
    assert [[m for *_, m in b] for b in R.batches([404, 67], W, OV, 2)] == [[64, 64]] * 5 + [[64, 63]]
    on, off = BufferedEncoder(enc, W, OV, batch_windows=2, graphs=True), BufferedEncoder(enc, W, OV, batch_windows=2)
    a, b = on.encode(mels), off.encode(mels)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    graph = on._graphed[None]
    assert graph.captures == 1 and tuple(graph.static_x.shape) == (2, 80, 64) and not off._graphed
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for p in enc.parameters():
            p.add_(0.02 * torch.randn(p.shape, generator=g).to(dev) * p.abs().mean())
    a2, b2 = on.encode(mels), off.encode(mels)
    assert graph.captures == 2 and on._graphed[None] is graph
    assert all(torch.equal(p, q) for p, q in zip(a2, b2))
    assert rel_l2(a2[0], a[0]) > 1e-4                                    # the update reached the output


@pytest.mark.parametrize("d,K", CASES)
def test_bf16_autocast(dev, d, K):
    enc = _encoder(_params(d, K), L, d, H, K, dev)
    mels = _on(_mels([403, 67, 7], 10), dev)
    be = BufferedEncoder(enc, W, OV, batch_windows=5)
    ref = be.encode(mels)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = be.encode(mels)
    for r, (g, w) in enumerate(zip(got, ref)):
        err = rel_l2(g.float(), w)
        print(f"d={d} K={K} recording {r}: bf16 autocast vs fp32 {err:.3g}")
        assert g.shape == w.shape and 0 < err < 1e-2, (r, err)


def test_graphs_under_bf16_autocast(dev):
    """Under bf16 autocast the full batches replay a graph of their own, captured under that autocast; the fp32 graph stays."""
    d, K = 32, 31
    enc = _encoder(_params(d, K), L, d, H, K, dev)
    mels = _on(_mels([404, 67], 8), dev)
    on, off = BufferedEncoder(enc, W, OV, batch_windows=2, graphs=True), BufferedEncoder(enc, W, OV, batch_windows=2)
    f32 = on.encode(mels)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        a, b = on.encode(mels), off.encode(mels)
    assert set(on._graphed) == {None, torch.bfloat16} and on._graphed[torch.bfloat16].autocast_dtype is torch.bfloat16
    assert on._graphed[torch.bfloat16].captures == 1 and on._graphed[None].captures == 1
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert 0 < rel_l2(a[0].float(), f32[0]) < 1e-2
    assert all(torch.equal(p, q) for p, q in zip(on.encode(mels), f32))  # and back: the fp32 graph again


def test_other_ambient_autocast_is_refused(dev):
    """torch.autocast("cuda") itself only takes bfloat16 and float16, so any other ambient type is set through the setters."""
    m, _ = _model(32, 4, 71, dev)
    tr = Transcriber(m, _decoder("plain", None), window_seconds=0.64, overlap_seconds=0.24)
    mels = _on(_mels([67], 15), dev)
    want = tr.encoder.encode(mels)
    keep = torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda")
    try:
        torch.set_autocast_enabled("cuda", True)
        torch.set_autocast_dtype("cuda", torch.float32)
        with pytest.raises(RuntimeError, match="no gfx950 path"):
            tr.encoder.encode(mels)
        with pytest.raises(RuntimeError, match="no gfx950 path"):
            tr.transcribe(mels)
    finally:
        torch.set_autocast_enabled("cuda", keep[0])
        torch.set_autocast_dtype("cuda", keep[1])
    assert torch.equal(tr.encoder.encode(mels)[0], want[0])


def _waves():
    """caller's order: a 64-frame recording, 2 s at 8 kHz (201 frames after resampling), 403 frames, 7 frames"""
    g = torch.Generator().manual_seed(14)
    lengths, rates = [63 * 160 + 5, 16000, 402 * 160 + 37, 6 * 160], [16000, 8000, 16000, 16000]
    return [_wave(n, r, g) for n, r in zip(lengths, rates)], rates, [64, 201, 403, 7]


def _wave(n, rate, g):
    """A tone with noise whose pitch and level (over 60 dB) change every 0.1 s: the random model writes several words of it,
    stationary noise gives one."""
    t = torch.arange(n, dtype=torch.float64)
    out = torch.zeros(n, dtype=torch.float64)
    for s in range(0, n, rate // 10):
        e = min(n, s + rate // 10)
        amp = 10.0 ** (3.0 * torch.rand(1, generator=g, dtype=torch.float64).item() - 3.0)
        f = 100.0 + 3000.0 * torch.rand(1, generator=g, dtype=torch.float64).item()
        out[s:e] = amp * (torch.sin(2 * math.pi * f * t[s:e] / rate) + 0.3 * torch.randn(e - s, generator=g, dtype=torch.float64))
    return out.float()


@pytest.mark.parametrize("bw", [2, 4])
def test_transcriber_end_to_end(dev, bw):
    """Text, Words and confidences equal the same stages called by hand on the stitched frames, in groups of bw recordings sorted
    by length; the results come back in the caller's order."""
    m, _ = _model(32, 4, 71, dev)
    dec, cfg = _decoder("plain", None), ConfidenceConfig()
    fe = ConformerAudioFrontend(device=dev)
    waves, rates, n_mel = _waves()
    tr = Transcriber(m, dec, fe, window_seconds=0.64, overlap_seconds=0.24, batch_windows=bw, times=True, confidence=cfg)
    assert (tr.window, tr.overlap) == (W, OV)
    got = tr.transcribe([w.to(dev) for w in waves], sample_rates=rates)
    # by hand
    mel, lengths = fe([w.to(dev) for w in waves], sample_rates=rates)
    assert lengths.tolist() == n_mel
    hs = BufferedEncoder(m.encoder, W, OV, batch_windows=bw).encode([mel[i, :, :n] for i, n in enumerate(n_mel)])
    order = [2, 1, 0, 3]                                                 # longest first
    want = {}
    for k in range(0, 4, bw):
        group = order[k:k + bw]
        T = [hs[i].shape[0] for i in group]
        h = torch.zeros(len(group), T[0], 32, device=dev)
        for row, i in enumerate(group):
            h[row, :T[row]] = hs[i]
        t = torch.tensor(T, device=dev)
        with torch.no_grad():
            logits = m.decoder(h, t)
        assert torch.equal(tr.decoder_head(h, t), logits)
        texts, words = dec(logits, t), dec.words(logits, t, 0.04)
        conf, ids = frame_confidence(logits, t, cfg)
        scores = word_confidence(words, conf, ids, dec.blank_id, t, cfg)
        for row, i in enumerate(group):
            want[i] = (texts[row], words[row], scores[row], T[row])
    assert any(t.text for t in got) and any(len(t.words) > 1 for t in got)
    for i, t in enumerate(got):
        assert (t.text, t.words, t.frames) == (want[i][0], want[i][1], want[i][3]) and t.frames == R.ef(n_mel[i]), i
        assert len(t.word_confidence) == len(t.words)
        assert all(a == b or (a != a and b != b) for a, b in zip(t.word_confidence, want[i][2])), i
        assert abs(t.seconds - n_mel[i] * 0.01) < 1e-9
        starts = [w.start for w in t.words]
        assert starts == sorted(starts) and all(w.start <= w.end for w in t.words)
        assert all(0 <= w.start_frame < w.end_frame <= t.frames and w.end <= t.seconds for w in t.words), i


def test_transcriber_takes_mel_frames_and_refuses_on_the_device(dev):
    m, _ = _model(32, 4, 71, dev)
    dec = _decoder("plain", None)
    tr = Transcriber(m, dec, window_seconds=0.64, overlap_seconds=0.24)
    assert (tr.window, tr.overlap) == (W, OV)                            # frame_seconds / 4 per mel frame
    mels = _on(_mels([67, 403], 13), dev)
    got = tr.transcribe(mels)
    assert [t.frames for t in got] == [R.ef(67), R.ef(403)] and all(t.words is None and t.word_confidence is None for t in got)
    hs = tr.encoder.encode(mels)
    with torch.no_grad():
        assert [t.text for t in got] == [dec(m.decoder(h[None]))[0] for h in hs]
    assert tr.transcribe([]) == []
    with pytest.raises(ValueError):
        tr.transcribe(mels, sample_rates=[16000, 16000])
    with pytest.raises(ValueError):
        tr.transcribe([mels[0][:, :6]])                                  # fewer than 7 mel frames: no encoder frame
    m.train()
    try:
        with pytest.raises(RuntimeError):
            tr.transcribe(mels)
        with pytest.raises(RuntimeError):
            tr.encoder.encode(mels)
    finally:
        m.eval()


def test_memory_is_one_batch_of_windows(dev):
    """403 -> 1603 mel frames at batch_windows = 4 (10 -> 40 windows): the peak above the input, which is allocated before the
    call, grows by the output alone.  Slack 64 KiB: the allocator rounds every block up to 512 bytes, and the runs differ by the
    output and the length vector of one ragged batch; a single further copy of the longer input would be 375 KiB over.
    This is BufferedEncoder's bound.  Transcriber.transcribe is not held to it: it keeps a second, padded copy of a group's stitched
    frames for the decoder head, and the head, the logits and the search grow with the recording (its docstring says so)."""
    d, K = 32, 31
    enc = _encoder(_params(d, K), L, d, H, K, dev)
    be = BufferedEncoder(enc, W, OV, batch_windows=4)
    peaks = []
    for n in (403, 403, 1603):                                           # (the first call builds the weight packs)
        x = _on(_mels([n], 14), dev)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = be.encode(x)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - before)
        assert out[0].shape == (R.ef(n), d)
        del x, out
    grow = (R.ef(1603) - R.ef(403)) * d * 4
    print(f"peak over the input: 403 frames {peaks[1]} B, 1603 frames {peaks[2]} B; output grows by {grow} B")
    assert peaks[2] - peaks[1] <= grow + 64 * 1024, peaks
