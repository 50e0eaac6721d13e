"""Long-form CTC forced alignment (`conformer_amd.align.ctc_forced_align_long`) against the float64 restatement
`tests/ctc_align_restatement.py`.

The long kernel keeps float64 state and never re-centres it: every lattice value is the restatement's chain of IEEE double
additions of fp32 logits and exact comparisons.  So the device path must EQUAL the restatement's, state for state, on the
grid families of test_ctc_align_gpu (`g6`, `int`: thousands of exact ties) AND on real-valued logits, where the fp32 kernel
is only held to a near-optimal path.  Everything runs with tile_pairs = 512, chunk_frames = 64 unless stated (the smallest
tile, so these small shapes cross many cell borders in both directions); dead cells (skipped whole) occur on both sides.

Scores: SCORE_TOL / TOTAL_TOL of test_ctc_align_gpu, derived there for T <= 16384 with a margin of 6 decimal digits; every
scored case here has T <= 17000, so the same derivation holds (the per-frame kernels are the same ones)."""
import math

import numpy as np
import pytest
import torch

from conformer_amd import align as A
from conformer_amd.align import CTCAligner, ctc_forced_align, ctc_forced_align_long
from tests import ctc_align_restatement as R
from tests import test_ctc_align_gpu as G
from tests.test_write_guard_gpu import guarded_allocations

pytestmark = pytest.mark.gpu
INF = math.inf
TILE, CHUNK = 512, 64
KINDS = ["g6", "int", "randn"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def run_long(x, y, blank, lengths, tlens, dev, tile_pairs=TILE, chunk_frames=CHUNK):
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    out = ctc_forced_align_long(to(x), to(y), blank, to(lengths), to(tlens), tile_pairs=tile_pairs, chunk_frames=chunk_frames)
    B, T, _ = x.shape
    Lmax = y.shape[1]
    assert out.frame_tokens.shape == out.frame_index.shape == (B, T)
    assert out.token_start.shape == out.token_end.shape == out.token_score.shape == (B, Lmax)
    assert out.score.shape == out.ok.shape == (B,)
    assert out.frame_tokens.dtype == out.frame_index.dtype == out.token_start.dtype == out.token_end.dtype == torch.int64
    assert out.token_score.dtype == torch.float32 and out.score.dtype == torch.float64 and out.ok.dtype == torch.bool
    return A.Alignment(*(t.cpu().numpy() for t in out))


def check_equal(x, y, blank, lengths, tlens, dev, label="", **tiling):
    """every output of the device against the restatement: tokens, indices, states, spans, padding, scores"""
    B, T, V = x.shape
    out = run_long(x, y, blank, lengths, tlens, dev, **tiling)
    worst, oks = (0.0, 0.0), []
    for b in range(B):
        n = T if lengths is None else int(min(max(lengths[b], 0), T))
        L = y.shape[1] if tlens is None else int(min(max(tlens[b], 0), y.shape[1]))
        yb = [int(min(max(v, 0), V - 1)) for v in y[b, :L]]
        ref = R.align(x[b], yb, blank, n)
        G.check_padding(out, b, n, L, ref.ok)
        oks.append(ref.ok)
        if not ref.ok:
            continue
        assert (out.frame_tokens[b, :n] == ref.frame_tokens).all(), (label, b)
        assert (out.frame_index[b, :n] == ref.frame_index).all(), (label, b)
        assert (G.device_states(out, b, n, L) == ref.states).all(), (label, b)
        worst = tuple(max(a, c) for a, c in zip(worst, G.check_scores(out, b, ref, L)))
    print(f"[ctc_align_long {label}] B={B} T={T} V={V} Lmax={y.shape[1]}: token_score diff {worst[0]:.2e}, score diff {worst[1]:.2e}")
    return out, oks


def case(seed, shape, kind, Lmax, blank=0, tlens=None):
    rng = np.random.default_rng(seed)
    x = G.grid(rng, shape, kind)
    y = G.make_targets(rng, shape[0], Lmax, shape[2], blank, [Lmax] * shape[0] if tlens is None else tlens)
    return x, y


@pytest.mark.parametrize("kind", KINDS)
def test_tiles_and_chunks(dev, kind):
    """(1, 1400, 6, 1100): 3 tiles x 22 chunks, front-dead cells above the diagonal t = i"""
    x, y = case(200, (1, 1400, 6), kind, 1100, blank=1)
    _, oks = check_equal(x, y, 1, None, None, dev, f"tiles {kind}")
    assert oks == [True]


RAGGED = {   # lengths, target lengths (clamped on the device): 0 and T, 0 / 2 / Lmax, garbage beyond the target lengths
    "plain": ([1400, 1013, 0], [1100, 2, 0], [True, True, False]),
    "clamped": ([1400 + 1000, 700, 1400], [1100 + 77, 0, 2], [True, True, True]),
}


@pytest.mark.parametrize("kind", KINDS)
def test_ragged(dev, kind):
    for name, (lengths, tlens, want) in RAGGED.items():
        x, y = case(210, (3, 1400, 6), kind, 1100, tlens=np.minimum(tlens, 1100))
        lengths, tlens = np.array(lengths, dtype=np.int64), np.array(tlens, dtype=np.int64)
        _, oks = check_equal(x, y, 0, lengths, tlens, dev, f"ragged {name} {kind}")
        assert oks == want


@pytest.mark.parametrize("kind", KINDS)
def test_many_back_dead_cells(dev, kind):
    """(1, 3000, 5, 600), chunk_frames = 16: T >> L, most cells of tile 0 cannot reach the end any more"""
    x, y = case(220, (1, 3000, 5), kind, 600)
    _, oks = check_equal(x, y, 0, None, None, dev, f"back-dead {kind}", tile_pairs=512, chunk_frames=16)
    assert oks == [True]


def few_repeats(rng, L, V):
    """labels 1 .. V-1 (blank 0) whose neighbours differ, but for every 16th position, which repeats the one before"""
    y = (1 + np.cumsum(rng.integers(1, V - 1, size=L)) % (V - 1)).astype(np.int64)
    y[16::16] = y[15::16][:len(y[16::16])]
    return y


def tight_target(rng, L, V):
    y = rng.integers(1, V, size=L).astype(np.int64)
    y[5::7] = y[4::7][:len(y[5::7])]                     # forced adjacent repeats
    return y


@pytest.mark.parametrize("kind", KINDS)
def test_tightest_feasible_and_infeasible(dev, kind):
    """T = L + repeats exactly (L = 1030): one path exists; one frame fewer: ok False, score -inf, padding"""
    rng = np.random.default_rng(230)
    y = tight_target(rng, 1030, 6)
    T = 1030 + R.repeats(y.tolist())
    assert T > 1030 + 100
    x = G.grid(rng, (1, T, 6), kind)
    out, oks = check_equal(x, y[None], 0, None, None, dev, f"tight {kind}")
    assert oks == [True] and (out.token_end[0] - out.token_start[0] == 1).all()
    out, oks = check_equal(x[:, :T - 1], y[None], 0, None, None, dev, f"infeasible {kind}")
    assert oks == [False] and not out.ok[0] and out.score[0] == -INF


@pytest.mark.parametrize("Lmax", [511, 512, 513, 1023, 1024])
@pytest.mark.parametrize("kind", KINDS)
def test_tile_border(dev, kind, Lmax):
    """pair L and pair L - 1 on either side of a tile border: the end-state choice reads one or two tiles' carries"""
    rng = np.random.default_rng(240 + Lmax)
    x = G.grid(rng, (1, 1200, 6), kind)
    y = few_repeats(rng, Lmax, 6)
    assert Lmax + R.repeats(y.tolist()) <= 1200                        # random labels would repeat too often to fit
    _, oks = check_equal(x, y[None], 0, None, None, dev, f"border L={Lmax} {kind}")
    assert oks == [True]


def test_same_answer_for_every_tiling(dev):
    x, y = case(250, (1, 2048, 6), "randn", 1500)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    outs = [ctc_forced_align_long(xd, yd, 0, tile_pairs=tp, chunk_frames=cf)
            for tp, cf in ((512, 16), (512, 64), (1024, 256), (2048, 2048), (None, None))]
    assert bool(outs[0].ok.all())
    for other in outs[1:]:
        for got, want in zip(other, outs[0]):
            assert torch.equal(got, want)


def test_agrees_with_the_existing_kernel(dev):
    rng = np.random.default_rng(260)
    x = torch.from_numpy(G.grid(rng, (2, 2048, 5), "g6")).to(dev)
    tl = np.array([1500, 611])
    y = torch.from_numpy(G.make_targets(rng, 2, 1500, 5, 0, tl)).to(dev)
    ln, tl = torch.tensor([2048, 1777], device=dev), torch.from_numpy(tl).to(dev)
    long, short = ctc_forced_align_long(x, y, 0, ln, tl, tile_pairs=TILE, chunk_frames=CHUNK), ctc_forced_align(x, y, 0, ln, tl)
    assert bool(short.ok.all())
    for name in ("frame_tokens", "frame_index", "token_start", "token_end", "ok"):
        assert torch.equal(getattr(long, name), getattr(short, name)), name


def test_beyond_the_old_limits(dev):
    """(1, 17000, 6, 4200) on the 2^-4 grid with the default tiling: both old limits exceeded"""
    assert 17000 > A.MAX_FRAMES and 4200 > A.MAX_TARGET
    x, y = case(270, (1, 17000, 6), "g4", 4200)
    _, oks = check_equal(x, y, 0, None, None, dev, "beyond", tile_pairs=None, chunk_frames=None)
    assert oks == [True]


def test_guarded_buffers(dev):
    """the ragged cases again: nothing is written outside the outputs and the workspace"""
    for name, (lengths, tlens, want) in RAGGED.items():
        x, y = case(210, (3, 1400, 6), "g6", 1100, tlens=np.minimum(tlens, 1100))
        with guarded_allocations() as guard:
            saved, A.torch = A.torch, guard
            try:
                lengths, tlens = np.array(lengths, dtype=np.int64), np.array(tlens, dtype=np.int64)
                _, oks = check_equal(x, y, 0, lengths, tlens, dev, f"guarded {name}")
                bad = guard.check()
            finally:
                A.torch = saved
        assert len(guard.allocs) >= 8 and not bad, bad
        assert oks == want


def test_capture_in_a_graph_and_replay_with_new_logits(dev):
    rng = np.random.default_rng(280)
    y = few_repeats(rng, 520, 5)
    assert 520 + R.repeats(y.tolist()) <= 600
    y = torch.from_numpy(y[None]).to(dev)
    static_x = torch.from_numpy(G.grid(rng, (1, 600, 5), "g6")).to(dev)
    run = lambda x: ctc_forced_align_long(x, y, 0, tile_pairs=TILE, chunk_frames=CHUNK)  # noqa: E731
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run(static_x)
        side.synchronize()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(static_x)
    for seed in (281, 282):
        new = torch.from_numpy(G.grid(np.random.default_rng(seed), (1, 600, 5), "randn")).to(dev)
        static_x.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(new)
        for got, want in zip(captured, eager):
            assert torch.equal(got, want)
        ref = R.align(new[0].cpu().numpy(), y[0].tolist(), 0)
        assert (captured.frame_index[0].cpu().numpy() == ref.frame_index).all()
    assert captured.ok.tolist() == [True]


VOCAB = G.VOCAB


def test_aligner_long_equals_short_and_short_keeps_its_limits(dev):
    rng = np.random.default_rng(290)
    V = len(VOCAB)
    x = torch.from_numpy(G.grid(rng, (2, 300, V), "g6")).to(dev)
    aligner = CTCAligner(VOCAB, 0, skip_ids=(V - 1,))
    texts = ["abc def ab", "lk jih g fe"]
    lengths = torch.tensor([300, 211], device=dev)
    short, long = aligner(x, texts, lengths), aligner(x, texts, lengths, long=True)
    assert short == long and all(len(w) >= 3 for w in long)
    ids, al = aligner.align(x, texts, lengths, long=True)
    assert ids == [aligner.tokenize(t) for t in texts] and bool(al.ok.all())
    big = torch.zeros(1, A.MAX_FRAMES + 8, V, device=dev)
    with pytest.raises(ValueError, match="supports T <= 16384"):
        aligner(big, ["ab"])
    with pytest.raises(ValueError, match="supports T <= 16384"):
        aligner(big, ["ab"], long=False)
    assert [w.text for w in aligner(big, ["ab"], long=True)[0]] == ["ab"]


def test_transcriber_align_end_to_end(dev):
    """A tiny model (2 blocks, d = 32), one recording of several windows, the text taken from transcribe itself."""
    from conformer_amd.decode import BeamCTCDecoder
    from conformer_amd.longform import Aligned, Transcriber
    from model.conformer import Conformer
    from oracle import conformer_oracle as O
    V = len(VOCAB)
    P = O.make_params(vocab=V, n_mel=80, n_blocks=2, d=32, n_heads=4, ksize=31, lstm_hidden=24, seed=31)
    m = Conformer(V, 80, 2, 32, 4, 31, 24, 1, 0.0)
    m.load_state_dict(P, strict=True)
    m = m.to(dev).eval()

    class Sharp(Transcriber):                     # random weights give flat logits: sharpen them so that text comes out
        def decoder_head(self, h, lengths=None):
            return (super().decoder_head(h, lengths).float() * 6).contiguous()

    dec = BeamCTCDecoder(VOCAB, 0, skip_ids=(V - 1,), beam_width=16)
    tr = Sharp(m, dec, None, window_seconds=0.64, overlap_seconds=0.24, batch_windows=4)
    mel = torch.randn(80, 403, generator=torch.Generator().manual_seed(300)).to(dev)
    assert len(tr.encoder.plan([403])[0]) >= 4
    first = tr.transcribe([mel])[0]
    assert first.text.strip(), "the decoder returned no text at all: the test would show nothing"
    got = tr.align([mel], [first.text])
    assert len(got) == 1 and isinstance(got[0], Aligned)
    al = got[0]
    assert al.ok and al.frames == first.frames and al.seconds == pytest.approx(first.seconds)
    assert al.words and " ".join(w.text for w in al.words) == " ".join(first.text.split())
    assert -INF < al.score <= 0.0
    prev = 0.0
    for w in al.words:
        assert prev <= w.start <= w.end <= al.seconds + 1e-9, w
        assert 0 <= w.start_frame < w.end_frame <= al.frames
        prev = w.end
    ids = dec.vocab.index("a")
    too_long = tr.align([mel], [[ids, dec.vocab.index("b")] * al.frames])       # more tokens than frames
    assert too_long[0].ok is False and too_long[0].words == [] and too_long[0].score == -INF
