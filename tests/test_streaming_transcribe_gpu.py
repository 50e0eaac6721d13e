"""Streaming transcription on the MI355X: the carried LSTM state (ops.lstm_forward(state=...)) of all three forward kernels is
bit-identical to one call over all the frames in any chunking, and StreamingTranscriber (StreamingEncoder -> decoder with the
LSTM state carried -> resumable beam search) gives the logits of the chunked model and the text of BeamCTCDecoder on them."""
import contextlib

import pytest
import torch

from conformer_amd import ops
from conformer_amd.decode import BeamCTCDecoder
from oracle import conformer_oracle as O
from tests.util import rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# (H, autocast dtype): row-major fp32 kernel (H % 16 != 0), fragment-order fp32 kernel, 16-bit kernels
LSTM_CASES = [(20, None), (48, None), (32, torch.bfloat16), (64, torch.float16)]


@pytest.mark.parametrize("H,dt", LSTM_CASES, ids=["rowmajor", "frag", "bf16", "fp16"])
@pytest.mark.parametrize("chunks", [[37], [1] * 37, [7, 1, 20, 9], [36, 1]])
def test_lstm_carry_equals_one_call(dev, H, dt, chunks):
    """The recurrence over the same gates_x (the input-projection GEMM may tile a chunk differently from the whole sequence):
    chunked with the state carried == one call, bit for bit, with ragged lengths (frozen state, an utterance with no
    frames) and from a zero or a random initial state."""
    B, T = 5, 37
    g = torch.Generator().manual_seed(H)
    gx = torch.randn(B, T, 4 * H, generator=g).to(dev)
    w_hh = (torch.randn(4 * H, H, generator=g) / H ** 0.5).to(dev)
    L = torch.tensor([T, 0, 13, T - 1, 1], device=dev)
    amp = contextlib.nullcontext() if dt is None else torch.autocast("cuda", dtype=dt)
    h_init, c_init = torch.randn(B, H, generator=g).to(dev), torch.randn(B, H, generator=g).to(dev)
    with amp, torch.no_grad():
        y1, _, cells = ops.lstm_recurrence(gx, w_hh, L, save=True)
        for lens in (L, None):
            for init in ("zero", "random"):
                h = torch.zeros(B, H, device=dev) if init == "zero" else h_init.clone()
                c = torch.zeros(B, H, device=dev) if init == "zero" else c_init.clone()
                if init == "zero":
                    ref = y1 if lens is not None else ops.lstm_recurrence(gx, w_hh, None)
                else:
                    ref = ops.lstm_recurrence(gx, w_hh, lens, state=(h_init.clone(), c_init.clone()))
                    assert not torch.equal(ref, ops.lstm_recurrence(gx, w_hh, lens))      # the initial state matters
                ys, t0 = [], 0
                for ck in chunks:
                    cl = None if lens is None else (lens - t0).clamp(0, ck)
                    ys.append(ops.lstm_recurrence(gx[:, t0:t0 + ck].contiguous(), w_hh, cl, state=(h, c)))
                    t0 += ck
                assert torch.equal(torch.cat(ys, dim=1), ref), (H, dt, chunks, init, lens is None)
                if init == "zero" and lens is not None:
                    # the state after each utterance's last frame; an utterance with no frames keeps its (zero) state
                    for b, n in enumerate(L.tolist()):
                        assert torch.equal(h[b], y1[b, n - 1] if n else torch.zeros(H, device=dev))
                        assert torch.equal(c[b], cells[b, n - 1] if n else torch.zeros(H, device=dev))


def test_lstm_forward_with_zero_state_is_lstm_forward(dev):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 11, 24, generator=g).to(dev)
    w_ih, w_hh, bias = (torch.randn(128, 24, generator=g) / 5).to(dev), (torch.randn(128, 32, generator=g) / 6).to(dev), \
        (torch.randn(128, generator=g) / 10).to(dev)
    with torch.no_grad():
        state = (torch.zeros(3, 32, device=dev), torch.zeros(3, 32, device=dev))
        assert torch.equal(ops.lstm_forward(x, w_ih, w_hh, bias, state=state), ops.lstm_forward(x, w_ih, w_hh, bias))
        assert torch.equal(state[0], ops.lstm_forward(x, w_ih, w_hh, bias)[:, -1])


def _model(vocab, d, heads, n_blocks, hidden, seed, dev):
    from model.conformer import Conformer
    P = O.make_params(vocab=vocab, n_mel=80, n_blocks=n_blocks, d=d, n_heads=heads, ksize=31, lstm_hidden=hidden, seed=seed,
                      dtype=torch.float64)
    m = Conformer(vocab, 80, n_blocks, d, heads, 31, hidden, 1, 0.0)
    m.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in P.items()}, strict=True)
    return m.to(dev).eval(), P


VOCAB = ["<pad>"] + [chr(ord("a") + i) for i in range(14)] + ["|", "<unk>"]


def _run(tr, x, chunks):
    outs, t0 = [], 0
    for c in chunks:
        outs.append(tr.step(x[:, :, t0:t0 + c]))
        t0 += c
    return torch.cat(outs, dim=1)


@pytest.mark.parametrize("cfg", [dict(d=32, heads=4, hidden=24, chunks=[64, 64, 7, 1, 130, 64, 70]),
                                 dict(d=512, heads=8, hidden=640, chunks=[640, 640, 160])], ids=["small", "cfg5_width"])
def test_transcriber_matches_chunked_model_and_decoder(dev, cfg):
    from conformer_amd.streaming import StreamingEncoder, chunk_ends
    from conformer_amd.transcribe import StreamingTranscriber
    m, P = _model(len(VOCAB), cfg["d"], cfg["heads"], 2, cfg["hidden"], 41, dev)
    chunks = cfg["chunks"]
    T = sum(chunks)
    B = 3
    x = torch.randn(B, 80, T, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    xd = x.float().to(dev)
    dec = BeamCTCDecoder(VOCAB, blank_id=0, skip_ids=(16,), beam_width=16)
    tr = StreamingTranscriber(m, dec, B, T)
    got = _run(tr, xd, chunks)
    with torch.no_grad():
        enc = StreamingEncoder(m.encoder, B, T)
        outs, t0 = [], 0
        for c in chunks:
            outs.append(enc.step(xd[:, :, t0:t0 + c]))
            t0 += c
        want = m.decoder(torch.cat(outs, dim=1))
    assert got.shape == want.shape
    assert rel_l2(got, want) < 1e-5
    ref = O.decoder_forward(O.encoder_forward_chunked(x, P, 2, cfg["heads"], chunk_ends(T, chunks)), None, P)
    assert rel_l2(got, ref) < 2e-5
    partial = tr.partial_text()
    text = tr.finish()
    assert text == dec(got) and len(partial) == B
    assert partial == text                          # no LM, no hotwords: the interim best is the final one
    with pytest.raises(RuntimeError):
        tr.step(xd[:, :, :64])
    tr.reset()
    again = _run(tr, xd, chunks)
    assert torch.equal(again, got) and tr.finish() == text


def test_one_chunk_is_the_model(dev):
    from conformer_amd.transcribe import StreamingTranscriber
    for seed in (1, 2):
        m, _ = _model(len(VOCAB), 32, 4, 2, 24, 50 + seed, dev)
        x = torch.randn(2, 80, 211, generator=torch.Generator().manual_seed(seed)).to(dev)
        dec = BeamCTCDecoder(VOCAB, blank_id=0, skip_ids=(16,), beam_width=8)
        tr = StreamingTranscriber(m, dec, 2, 211)
        got = tr.step(x)
        with torch.no_grad():
            full, _ = m(x)
        assert rel_l2(got, full) < 2e-5
        assert tr.finish() == dec(full)


def test_transcriber_refuses_training_mode(dev):
    from conformer_amd.transcribe import StreamingTranscriber
    m, _ = _model(len(VOCAB), 32, 4, 2, 24, 7, dev)
    with pytest.raises(RuntimeError):
        StreamingTranscriber(m.train(), BeamCTCDecoder(VOCAB, 0), 1, 100)


def test_transcriber_under_autocast_tracks_fp32(dev):
    """bf16 autocast: the encoder's 16-bit path and the 16-bit LSTM with its state carried; logits within the bf16 bar of
    the fp32 stream."""
    from conformer_amd.transcribe import StreamingTranscriber
    m, _ = _model(len(VOCAB), 64, 4, 2, 32, 9, dev)
    x = torch.randn(2, 80, 300, generator=torch.Generator().manual_seed(5)).to(dev)
    dec = BeamCTCDecoder(VOCAB, blank_id=0, beam_width=8)
    ref = _run(StreamingTranscriber(m, dec, 2, 300), x, [100, 100, 100])
    tr = StreamingTranscriber(m, dec, 2, 300)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = _run(tr, x, [100, 100, 100])
        text = tr.finish()
    assert rel_l2(got, ref) < 2e-2 and text == dec(got)
