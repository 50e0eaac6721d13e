"""Forced alignment with wildcards on the device (`wildcard_penalty=` of conformer_amd.align) against the definition of
INTEGRATION.md "Wildcards", stated in numpy by tests/ctc_align_wild_fixture.py: the float64 restatement on the logits with
the column w = fl32(max - penalty) appended and the wildcards replaced by the id V.

Exact regime, short form: the grids of test_ctc_align_gpu (2^-6 in [-16,16], 2^-4 in [-8,8], {-2..2}) and penalties 0, 0.5
and 2 keep w on the grid, so every partial sum of the re-centred fp32 recursion is exact up to T = 2048 as derived there;
every case here has T <= 1300.  The device path must EQUAL the restatement's, state for state, ties included.  The long
form computes in float64 on (double)x and (double)w, the restatement's own additions: it must equal it on randn logits too.
Real-valued logits, short form: a valid path within the bound test_ctc_align_gpu derives, the same formula on x'.

Scores (from the state path, over the V real columns, a wildcard frame at max_v log_softmax): G.SCORE_TOL / G.TOTAL_TOL as
G.check_scores holds them (T <= 16384 there, T <= 1300 here)."""
import math

import numpy as np
import pytest
import torch

from conformer_amd import align as A
from conformer_amd.align import CTCAligner, ctc_forced_align, ctc_forced_align_long
from tests import ctc_align_restatement as R
from tests import ctc_align_wild_fixture as F
from tests import test_ctc_align_gpu as G
from tests.test_write_guard_gpu import guarded_allocations

pytestmark = pytest.mark.gpu
INF = math.inf
W = A.WILDCARD
PENALTIES = (0.0, 0.5, 2.0)
KINDS = ("g6", "g4", "int")
TILE, CHUNK = 512, 16
GARBAGE = (W,) + G.GARBAGE                           # what lies in `targets` beyond target_lengths


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def to(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run(x, y, blank, lengths, tlens, penalty, dev, long=None):
    """long: None (short form) or (tile_pairs, chunk_frames)"""
    if long is None:
        out = ctc_forced_align(to(x, dev), to(y, dev), blank, to(lengths, dev), to(tlens, dev), wildcard_penalty=penalty)
    else:
        out = ctc_forced_align_long(to(x, dev), to(y, dev), blank, to(lengths, dev), to(tlens, dev), tile_pairs=long[0],
                                    chunk_frames=long[1], wildcard_penalty=penalty)
    B, T, _ = x.shape
    assert out.frame_tokens.shape == out.frame_index.shape == (B, T)
    assert out.token_start.shape == out.token_end.shape == out.token_score.shape == (B, y.shape[1])
    assert out.frame_tokens.dtype == out.frame_index.dtype == out.token_start.dtype == out.token_end.dtype == torch.int64
    assert out.token_score.dtype == torch.float32 and out.score.dtype == torch.float64 and out.ok.dtype == torch.bool
    return A.Alignment(*(t.cpu().numpy() for t in out))


def geometry(x, y, lengths, tlens, b):
    T, Lmax = x.shape[1], y.shape[1]
    n = T if lengths is None else int(min(max(lengths[b], 0), T))
    L = Lmax if tlens is None else int(min(max(tlens[b], 0), Lmax))
    return n, L


def check_equal(x, y, blank, lengths, tlens, penalty, dev, long=None, label=""):
    """every output of the device against the definition: states, tokens, indices, spans, padding, scores"""
    out = run(x, y, blank, lengths, tlens, penalty, dev, long)
    worst, oks = (0.0, 0.0), []
    for b in range(x.shape[0]):
        n, L = geometry(x, y, lengths, tlens, b)
        ref = F.expected(x[b], y[b, :L].tolist(), blank, penalty, n)
        G.check_padding(out, b, n, L, ref.ok)
        oks.append(ref.ok)
        if not ref.ok:
            continue
        assert (G.device_states(out, b, n, L) == ref.states).all(), (label, b)
        assert (out.frame_tokens[b, :n] == ref.frame_tokens).all(), (label, b)
        assert (out.frame_index[b, :n] == ref.frame_index).all(), (label, b)
        worst = tuple(max(a, c) for a, c in zip(worst, G.check_scores(out, b, ref, L)))
    print(f"[ctc_align_wild {label}] {x.shape} Lmax={y.shape[1]} penalty={penalty}: token_score diff {worst[0]:.2e}, "
          f"score diff {worst[1]:.2e}, ok {oks}")
    return out, oks


def few_repeats(rng, L, V, blank):
    """labels other than the blank whose neighbours differ, but for every 16th position, which repeats the one before"""
    ids = np.array([v for v in range(V) if v != blank])
    y = ids[np.cumsum(rng.integers(1, len(ids), size=L)) % len(ids)].astype(np.int64)
    y[16::16] = y[15::16][:len(y[16::16])]
    return y


def seam_positions(L, P):
    """both ends, every 7th position, both sides of the thread seams (multiples of P), of the wave seams of the workgroup
    and long forms (multiples of 512) and of the lane-32 seam"""
    pos = {0, L - 1} | set(range(3, L, 7))
    for m in (P, 32 * P, 512):
        for k in range(m, L, m * (5 if m == P else 1)):
            pos |= {k - 1, k}
    return sorted(p for p in pos if 0 <= p < L)


def wild_targets(rng, B, Lmax, V, blank, tlens, P):
    """(B,Lmax): few_repeats labels with wildcards at seam_positions of every row's own length; beyond the length garbage,
    the wildcard value included"""
    y = np.stack([few_repeats(rng, Lmax, V, blank) for _ in range(B)])
    for b in range(B):
        L = int(tlens[b])
        y[b, seam_positions(L, P)] = W
        for i in range(L, Lmax):
            y[b, i] = GARBAGE[(b + i) % len(GARBAGE)]
    return y


def shape_P(Lmax):
    P = 1
    while 64 * P < Lmax + 1 and P < 16:
        P *= 2
    return 8 if Lmax > 1023 else P


# Lmax + 1 around 64 P for P = 1 .. 16, then the workgroup form
SEAMS = [62, 63, 64, 126, 127, 128, 254, 255, 256, 510, 511, 512, 1022, 1023, 1024, 1100]


@pytest.mark.parametrize("Lmax", SEAMS)
def test_exact_path_at_every_seam(dev, Lmax):
    k = SEAMS.index(Lmax)
    rng = np.random.default_rng(100 + Lmax)
    kind, V, blank = KINDS[k % 3], 7, k % 2
    B, T = 3, min(1300, Lmax + Lmax // 4 + 40)
    tlens = np.array([Lmax, max(Lmax - 67, 1), 2], dtype=np.int64)
    lengths = np.array([T, T - 29, 11], dtype=np.int64)
    y = wild_targets(rng, B, Lmax, V, blank, tlens, shape_P(Lmax))
    assert (y[0] == W).sum() >= Lmax // 8 and y[0, 0] == W and y[0, Lmax - 1] == W
    x = G.grid(rng, (B, T, V), kind)
    for penalty in PENALTIES:
        out, oks = check_equal(x, y, blank, lengths, tlens, penalty, dev, label=f"seam {kind}")
        assert oks == [True, True, True]
        assert (out.frame_tokens[0] == W).sum() >= (y[0] == W).sum()                   # every wildcard took a frame


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("penalty", PENALTIES)
def test_exact_path_small_batch(dev, kind, penalty):
    """B = 9 ragged rows (0 and the full length among them), V = 40 and V = 370 (several passes of the frame kernels' lanes)"""
    rng = np.random.default_rng(31)
    for V, Lmax, T in ((40, 60, 249), (370, 37, 90)):
        B = 9
        tlens, lengths = G.ragged(rng, B, Lmax), G.ragged(rng, B, T)
        tlens[2], lengths[1], lengths[2] = Lmax, T, T // 2
        y = wild_targets(rng, B, Lmax, V, 0, tlens, 1)
        check_equal(G.grid(rng, (B, T, V), kind), y, 0, lengths, tlens, penalty, dev, label=f"batch {kind}")


HAND = {     # name: (target, frames that just fit = L + repeats)
    "adjacent": ([W, W, 3, 1], 5),
    "beside a repeat": ([3, 3, W, 3, W, W, 2, 2], 11),
    "all wildcards": ([W] * 5, 9),
    "one wildcard": ([W], 1),
    "ends": ([W, 1, 2, W], 4),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_made_targets_tight_and_infeasible(dev, name):
    """T = L + repeats exactly (one path), one frame fewer (infeasible), and room to choose (T = 3 L + 9)"""
    yb, tight = HAND[name]
    assert tight == len(yb) + R.repeats(yb)
    y = np.array([yb], dtype=np.int64)
    for kind in KINDS:
        rng = np.random.default_rng(40 + len(yb))
        for T, want in ((tight, True), (tight - 1, False), (3 * len(yb) + 9, True)):
            if T < 1:
                continue
            x = G.grid(rng, (1, T, 5), kind)
            for penalty in PENALTIES:
                for long in (None, (TILE, CHUNK)):
                    out, oks = check_equal(x, y, 0, None, None, penalty, dev, long, f"{name} {kind} T={T}")
                    assert oks == [want]
                    if T == tight:
                        assert (out.token_end[0] - out.token_start[0] == 1).all()
                    if not want:
                        assert not out.ok[0] and out.score[0] == -INF


def test_all_wildcard_frames_are_wildcard_or_blank(dev):
    x = G.grid(np.random.default_rng(45), (1, 30, 6), "g6")
    out = run(x, np.array([[W] * 4]), 0, None, None, 0.5, dev)
    assert set(out.frame_tokens[0].tolist()) <= {W, 0} and (out.frame_tokens[0] == W).sum() >= 4


@pytest.mark.parametrize("Lmax", [511, 512, 513, 1023, 1024])
@pytest.mark.parametrize("kind", ["g6", "int", "randn"])
def test_long_form_tile_and_chunk_borders(dev, kind, Lmax):
    """tiling 512 x 16, T = 1200: wildcards at both sides of every tile border (seam_positions: 511 | 512, 1023 | 1024), and
    wildcard frames on both sides of chunk borders"""
    rng = np.random.default_rng(300 + Lmax)
    T, V = 1200, 6
    tlens = np.array([Lmax, Lmax - 3], dtype=np.int64)
    lengths = np.array([T, T - 17], dtype=np.int64)
    y = wild_targets(rng, 2, Lmax, V, 0, tlens, 8)
    for border in range(512, Lmax, 512):
        assert y[0, border - 1] == W and y[0, border] == W
    x = G.grid(rng, (2, T, V), kind)
    penalty = PENALTIES[(Lmax + len(kind)) % 3]
    out, oks = check_equal(x, y, 0, lengths, tlens, penalty, dev, (TILE, CHUNK), f"long {kind}")
    assert oks == [True, True]
    ft = out.frame_tokens[0]
    borders = range(CHUNK, T, CHUNK)                                                   # wildcard frames on either side of chunk borders
    assert sum(1 for t in borders if ft[t - 1] == W) >= 3 and sum(1 for t in borders if ft[t] == W) >= 3
    for other in ((512, 64), (1024, 256)):
        again = run(x, y, 0, lengths, tlens, penalty, dev, other)
        for got, want in zip(again, out):
            assert np.array_equal(got, want), other


@pytest.mark.parametrize("B,T,V,Lmax,seed", [(4, 600, 12, 200, 60), (2, 1300, 9, 1023, 61), (2, 1300, 9, 1100, 62)])
def test_real_valued_inputs_give_a_valid_near_optimal_path(dev, B, T, V, Lmax, seed):
    rng = np.random.default_rng(seed)
    x = G.grid(rng, (B, T, V), "randn")
    tlens = np.array([Lmax, Lmax // 2, 3, Lmax][:B], dtype=np.int64)
    lengths = np.array([T, T - 1, T // 2, T][:B], dtype=np.int64)
    y = wild_targets(rng, B, Lmax, V, 0, tlens, shape_P(Lmax))
    penalty = 0.5
    out = run(x, y, 0, lengths, tlens, penalty, dev)
    for b in range(B):
        n, L = int(lengths[b]), int(tlens[b])
        xp, yp = F.extended(x[b, :n], y[b, :L].tolist(), penalty)
        ref_states = R.viterbi(xp, yp, 0)
        assert ref_states is not None and bool(out.ok[b])
        st = G.device_states(out, b, n, L)
        assert R.valid_path(yp, st), b
        sym = R.state_symbols(yp, 0)[st]
        assert (out.frame_tokens[b, :n] == np.where(sym == V, W, sym)).all()
        gap = R.path_score(xp, yp, 0, ref_states) - R.path_score(xp, yp, 0, st)
        bound = 2 * n * 2.0 ** -23 * (n * float(np.abs(xp).max()))
        print(f"[ctc_align_wild real] T={n} L={L}: score gap {gap:.3e} (bound {bound:.3e}), same path {bool((st == ref_states).all())}")
        assert -1e-9 * n <= gap <= bound, (b, gap, bound)
        G.check_scores(out, b, F.reference(x[b, :n], y[b, :L].tolist(), 0, st), L)     # the scores of the path it returned


@pytest.mark.parametrize("Lmax,T", [(60, 249), (300, 700), (1100, 1300)])
def test_without_a_wildcard_every_output_is_the_parent_entrys(dev, Lmax, T):
    """the same arithmetic chain: torch.equal on all seven tensors, both forms, any penalty, garbage (the wildcard value
    too) beyond the target lengths; randn logits: not only where the path is pinned"""
    rng = np.random.default_rng(70 + Lmax)
    B, V = 3, 9
    for kind in ("g6", "randn"):
        x = to(G.grid(rng, (B, T, V), kind), dev)
        tl = np.array([Lmax, Lmax // 3, 0], dtype=np.int64)
        y = np.stack([few_repeats(rng, Lmax, V, 0) for _ in range(B)])
        for b in range(B):
            y[b, tl[b]:] = W
        y, tl, ln = to(y, dev), to(tl, dev), to(np.array([T, T - 40, 17], dtype=np.int64), dev)
        plain = ctc_forced_align(x, y, 0, ln, tl)
        plain_long = ctc_forced_align_long(x, y, 0, ln, tl, tile_pairs=TILE, chunk_frames=64)
        assert plain.ok.tolist() == [True, True, True]
        for penalty in (0.0, 0.5, 123.0):
            for got, want in zip(ctc_forced_align(x, y, 0, ln, tl, wildcard_penalty=penalty), plain):
                assert torch.equal(got, want), (kind, penalty)
            for got, want in zip(ctc_forced_align_long(x, y, 0, ln, tl, tile_pairs=TILE, chunk_frames=64,
                                                       wildcard_penalty=penalty), plain_long):
                assert torch.equal(got, want), (kind, penalty)


def test_none_keeps_clamping_the_wildcard_value(dev):
    """wildcard_penalty=None is today's call: -2 is clamped to id 0 like any negative id"""
    rng = np.random.default_rng(75)
    x = to(G.grid(rng, (1, 40, 5), "g6"), dev)
    a = ctc_forced_align(x, torch.tensor([[2, W, 3]], device=dev), 1)
    b = ctc_forced_align(x, torch.tensor([[2, 0, 3]], device=dev), 1)
    for got, want in zip(a, b):
        assert torch.equal(got, want)
    assert W not in a.frame_tokens.tolist()[0]


def test_short_equals_long(dev):
    rng = np.random.default_rng(80)
    B, T, V, Lmax = 2, 1300, 6, 1100
    tlens, lengths = np.array([Lmax, 611], dtype=np.int64), np.array([T, 1177], dtype=np.int64)
    y = wild_targets(rng, B, Lmax, V, 0, tlens, 8)
    x = G.grid(rng, (B, T, V), "g6")
    args = (to(x, dev), to(y, dev), 0, to(lengths, dev), to(tlens, dev))
    short = ctc_forced_align(*args, wildcard_penalty=0.5)
    long = ctc_forced_align_long(*args, tile_pairs=TILE, chunk_frames=64, wildcard_penalty=0.5)
    assert bool(short.ok.all()) and bool((short.frame_tokens == W).any())
    for got, want in zip(long, short):
        assert torch.equal(got, want)


VOCAB = ["<pad>", "a", "b", "c", "d", "e", "f", "g", "h", "i", "j", "k"]


def test_planted_gaps_are_recovered_through_segments(dev):
    """B = 4 planted recordings (ctc_align_wild_fixture.planted), penalty 0.5: CTCAligner.segments returns every word at its
    planted frames; the same words in one target without wildcards do not come back there."""
    seeds = (1, 2, 3, 4)
    ps = [F.planted(s) for s in seeds]
    x = to(np.stack([p.x for p in ps]), dev)
    aligner = CTCAligner(VOCAB, F.PLANT_BLANK, delim_token="|", frame_seconds=0.04, wildcard_penalty=F.PLANT_PENALTY)
    utterances = [[list(w) for w in F.PLANT_WORDS]] * 4
    segs = aligner.segments(x, utterances)
    for b, p in enumerate(ps):
        assert [s.index for s in segs[b]] == [0, 1, 2]
        for s, spans, word in zip(segs[b], p.spans, F.PLANT_WORDS):
            assert (s.start_frame, s.end_frame) == (spans[0][0], spans[-1][1]), (b, s)
            assert s.start == pytest.approx(0.04 * s.start_frame) and s.end == pytest.approx(0.04 * s.end_frame)
            assert s.text == "".join(VOCAB[t] for t in word) and [w.text for w in s.words] == [s.text]
            assert -0.2 < s.score <= 0.0                              # 6.0 against eleven of at most 2.0: -log(1 + 11 e^-4)
    ids, al = aligner.align(x, [F.planted_target(True)] * 4)
    plain_ids, plain = aligner.align(x, [F.planted_target(False)] * 4)
    assert bool(al.ok.all()) and bool(plain.ok.all())
    for b, p in enumerate(ps):
        as_result = lambda a: R.Result(True, None, None, None, a.token_start[b].cpu().numpy(), a.token_end[b].cpu().numpy(), None, 0.0)  # noqa: E731
        assert F.recovered(as_result(al), ids[b], p), b
        assert not F.recovered(as_result(plain), plain_ids[b], p), b                   # the fixture cannot go soft
    single = aligner.segments(x[0], utterances[0])
    assert single == segs[0]


def test_guarded_buffers(dev):
    """infeasible and clamped rows between feasible ones, all three kernel forms: nothing is written outside the outputs
    and the workspace, whose last part (w) is new"""
    rng = np.random.default_rng(90)
    for Lmax, T, long in ((6, 40, None), (1100, 1300, None), (600, 760, (TILE, CHUNK))):
        B, V = 6, 5
        x = G.grid(rng, (B, T, V), "g6")
        lengths = np.array([T, 0, 3, T + 1000, T, -5], dtype=np.int64)
        tlens = np.array([Lmax, 2, Lmax, Lmax + 77, 0, 1], dtype=np.int64)
        y = wild_targets(rng, B, Lmax, V, 0, np.minimum(tlens, Lmax), 8)
        with guarded_allocations() as guard:
            saved, A.torch = A.torch, guard
            try:
                out, oks = check_equal(x, y, 0, lengths, tlens, 0.5, dev, long, f"guarded Lmax={Lmax}")
                bad = guard.check()
            finally:
                A.torch = saved
        assert len(guard.allocs) >= 8 and not bad, bad
        assert oks == [True, False, False, True, True, False]


def test_capture_in_a_graph_and_replay_with_new_logits(dev):
    rng = np.random.default_rng(95)
    B, T, V, Lmax = 3, 640, 6, 520
    tlens, lengths = np.array([520, 80, 33], dtype=np.int64), np.array([640, 450, 20], dtype=np.int64)   # the last is infeasible
    y = wild_targets(rng, B, Lmax, V, 0, tlens, 8)
    yd, tl, ln = to(y, dev), to(tlens, dev), to(lengths, dev)
    static_x = to(G.grid(rng, (B, T, V), "g6"), dev)
    runs = (lambda x: ctc_forced_align(x, yd, 0, ln, tl, wildcard_penalty=0.5),
            lambda x: ctc_forced_align_long(x, yd, 0, ln, tl, tile_pairs=TILE, chunk_frames=64, wildcard_penalty=0.5))
    for fn in runs:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            fn(static_x)
            side.synchronize()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = fn(static_x)
        for seed in (96, 97):
            new_np = G.grid(np.random.default_rng(seed), (B, T, V), "g6")
            static_x.copy_(to(new_np, dev))
            graph.replay()
            torch.cuda.synchronize()
            for got, want in zip(captured, fn(to(new_np, dev))):
                assert torch.equal(got, want)
            ref = F.expected(new_np[0], y[0].tolist(), 0, 0.5)
            assert (captured.frame_index[0].cpu().numpy() == ref.frame_index).all()
        assert captured.ok.tolist() == [True, True, False]


def test_argument_errors(dev):
    x = torch.zeros(1, 8, 5, device=dev)
    y = torch.tensor([[1, W, 2]], device=dev)
    for bad in (-0.5, math.nan, math.inf, "1", True, 1e39):
        with pytest.raises(ValueError, match="wildcard_penalty"):
            ctc_forced_align(x, y, 0, wildcard_penalty=bad)
        with pytest.raises(ValueError, match="wildcard_penalty"):
            ctc_forced_align_long(x, y, 0, wildcard_penalty=bad)
    assert bool(ctc_forced_align(x, y, 0, wildcard_penalty=0).ok.all())
    aligner = CTCAligner(VOCAB, 0)
    with pytest.raises(ValueError, match="no wildcard_penalty"):
        aligner.align(torch.zeros(1, 8, len(VOCAB), device=dev), [[1, W, 2]])
    with pytest.raises(ValueError, match="wildcard_penalty"):
        aligner.segments(torch.zeros(1, 8, len(VOCAB), device=dev), [[[1], [2]]])


def test_transcriber_segments_end_to_end(dev):
    """The smoke-sized model on random mel input, one recording of several windows; the utterances are pieces of what
    transcribe itself returned."""
    from conformer_amd.decode import BeamCTCDecoder
    from conformer_amd.longform import Segmented, Transcriber
    from model.conformer import Conformer
    from oracle import conformer_oracle as O
    vocab = G.VOCAB
    V = len(vocab)
    P = O.make_params(vocab=V, n_mel=80, n_blocks=2, d=32, n_heads=4, ksize=31, lstm_hidden=24, seed=31)
    m = Conformer(V, 80, 2, 32, 4, 31, 24, 1, 0.0)
    m.load_state_dict(P, strict=True)
    m = m.to(dev).eval()

    class Sharp(Transcriber):                     # random weights give flat logits: sharpen them so that text comes out
        def decoder_head(self, h, lengths=None):
            return (super().decoder_head(h, lengths).float() * 6).contiguous()

    dec = BeamCTCDecoder(vocab, 0, skip_ids=(V - 1,), beam_width=16)
    tr = Sharp(m, dec, None, window_seconds=0.64, overlap_seconds=0.24, batch_windows=4)
    mel = torch.randn(80, 403, generator=torch.Generator().manual_seed(300)).to(dev)
    first = tr.transcribe([mel])[0]
    aligner = CTCAligner.from_decoder(dec, wildcard_penalty=1.0)
    spoken = aligner.tokenize(first.text)
    assert len([i for i in spoken if i != aligner.delim_id]) >= 4, "the decoder returned too little text: the test would show nothing"
    cut = len(spoken) // 2                           # the text may be a single word: cut the tokens, not the words
    utterances = [spoken[:cut], spoken[cut:]]
    got = tr.segments([mel], [utterances], 1.0)
    assert len(got) == 1 and isinstance(got[0], Segmented)
    sg = got[0]
    assert sg.ok and sg.frames == first.frames and sg.seconds == pytest.approx(first.seconds) and -INF < sg.score <= 0.0
    assert [s.index for s in sg.segments] == [0, 1]
    assert "".join(s.text for s in sg.segments).replace(" ", "") == first.text.replace(" ", "")
    prev = 0
    for s, u in zip(sg.segments, utterances):
        assert prev <= s.start_frame < s.end_frame <= sg.frames, s                     # ordered, disjoint, inside
        assert s.start == pytest.approx(0.04 * s.start_frame) and s.end == pytest.approx(0.04 * s.end_frame)
        assert " ".join(w.text for w in s.words) == s.text and s.words and -INF < s.score <= 0.0
        assert all(s.start_frame <= w.start_frame < w.end_frame <= s.end_frame for w in s.words)
        prev = s.end_frame + 1                                                         # a wildcard frame lies between two
    # the frames collapse to the utterances' ids, a wildcard where one was placed
    with torch.no_grad():
        logits = next(tr._group_logits([mel], None))[3]
    target, ranges = aligner.segment_targets(utterances)
    ids, al = aligner.align(logits, [target], None, long=True)
    ft = al.frame_tokens[0].cpu().tolist()
    assert R.collapse(ft, 0) == target == ids[0]
    for s, (lo, hi) in zip(sg.segments, ranges):
        assert R.collapse(ft[s.start_frame:s.end_frame], 0) == target[lo:hi]
    # no wildcard placed at all (one utterance, ends=False): the words of Transcriber.align on the joined text
    whole = tr.segments([mel], [[first.text]], 1.0, ends=False)[0]
    aligned = tr.align([mel], [first.text])[0]
    assert whole.ok and len(whole.segments) == 1 and whole.segments[0].words == aligned.words
    assert whole.score == aligned.score
    # Transcriber.align with a wildcard token: the second half of the text, whatever comes before it absorbed
    half = tr.align([mel], ["* " + sg.segments[1].text], wildcard_token="*", wildcard_penalty=1.0)[0]
    assert half.ok and " ".join(w.text for w in half.words) == sg.segments[1].text
    assert half.words[0].start_frame >= 1
    too_many = tr.segments([mel], [[[dec.vocab.index("a"), dec.vocab.index("b")] * sg.frames]], 1.0)[0]
    assert too_many.ok is False and too_many.segments == [] and too_many.score == -INF
