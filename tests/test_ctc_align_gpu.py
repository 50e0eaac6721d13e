"""CTC forced alignment on the device (`conformer_amd.align`) against the float64 restatement `tests/ctc_align_restatement.py`.

Exact regime: logits on a grid (integer multiples of 2^-6 in [-16,16], or of 2^-4 in [-8,8] for the long-form case) make
every partial sum of the recursion exact in fp32 (below 2^15 with 6 fractional bits up to T = 2048; below 2^17 with 4 at
T = 16384), and re-centring subtracts a lattice value, which is on the grid too.  The device path must then EQUAL the
restatement's, state for state, ties included (thousands per case in the {-2..2} family).

Real-valued logits: the smallest decision margin seen in float64 was 6.5e-6 at T = 2048, too close to fp32 rounding to demand
the same path.  The device path must be a valid path whose float64 score is within 2 * T * 2^-23 * (T * max|x|) of the
optimum: the accumulated rounding of T fp32 additions at the largest magnitude an un-centred lattice can reach, once for
each side of a comparison.  The largest gap seen is printed (DESIGN.md records it).

Scores: token_score within 1e-4 (fp32 output, the SCORE_TOL of the beam tests), score within 1e-7 (float64 per-frame terms
agree with numpy to ~1e-12; 16384 of them leave a margin of 6)."""
import math

import numpy as np
import pytest
import torch

from conformer_amd import align as A
from conformer_amd.align import CTCAligner, ctc_forced_align
from tests import ctc_align_restatement as R
from tests.test_write_guard_gpu import guarded_allocations

pytestmark = pytest.mark.gpu
INF = math.inf
SCORE_TOL = 1e-4
TOTAL_TOL = 1e-7
GARBAGE = (1 << 40, -7, 0, 123456789)        # what lies in `targets` beyond target_lengths


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def grid(rng, shape, kind):
    if kind == "g6":
        return (rng.integers(-1024, 1025, size=shape) / 64.0).astype(np.float32)        # 2^-6 grid in [-16,16]
    if kind == "g4":
        return (rng.integers(-128, 129, size=shape) / 16.0).astype(np.float32)          # 2^-4 grid in [-8,8]
    if kind == "int":
        return rng.integers(-2, 3, size=shape).astype(np.float32)                       # {-2..2}: ties everywhere
    return (rng.standard_normal(shape) * 3).astype(np.float32)


def make_targets(rng, B, Lmax, V, blank, tlens):
    """(B,Lmax) int64 with random non-blank labels and garbage beyond each target length"""
    ids = np.array([v for v in range(V) if v != blank])
    y = ids[rng.integers(0, len(ids), size=(B, max(Lmax, 1)))][:, :Lmax].astype(np.int64)
    for b in range(B):
        for i in range(int(tlens[b]), Lmax):
            y[b, i] = GARBAGE[(b + i) % len(GARBAGE)]
    return y


def ragged(rng, B, hi, lo=0):
    if B == 1:
        return np.array([hi], dtype=np.int64)
    L = rng.integers(lo, hi + 1, size=B).astype(np.int64)
    L[0], L[1] = hi, 0
    return L


def run_device(x, y, blank, lengths, tlens, dev):
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    out = ctc_forced_align(to(x), to(y), blank, to(lengths), to(tlens))
    B, T, _ = x.shape
    Lmax = y.shape[1]
    assert out.frame_tokens.shape == out.frame_index.shape == (B, T)
    assert out.token_start.shape == out.token_end.shape == out.token_score.shape == (B, Lmax)
    assert out.score.shape == out.ok.shape == (B,)
    assert out.frame_tokens.dtype == out.frame_index.dtype == out.token_start.dtype == out.token_end.dtype == torch.int64
    assert out.token_score.dtype == torch.float32 and out.score.dtype == torch.float64 and out.ok.dtype == torch.bool
    return A.Alignment(*(t.cpu().numpy() for t in out))


def device_states(out, b, n, L):
    """the state of every frame from frame_index: a label frame of token i is 2i+1, a blank frame after i labels is 2i"""
    idx = out.frame_index[b, :n]
    started = np.maximum.accumulate(np.concatenate([[-1], idx]))[1:] + 1
    return np.where(idx >= 0, 2 * idx + 1, 2 * started)


def check_padding(out, b, n, L, ok):
    T, Lmax = out.frame_tokens.shape[1], out.token_start.shape[1]
    n, L = (n, L) if ok else (0, 0)
    assert (out.frame_tokens[b, n:] == -1).all() and (out.frame_index[b, n:] == -1).all(), b
    assert (out.token_start[b, L:] == -1).all() and (out.token_end[b, L:] == -1).all(), b
    assert (out.token_score[b, L:] == -INF).all(), b
    assert bool(out.ok[b]) == ok
    if not ok:
        assert out.score[b] == -INF


def check_scores(out, b, ref, L):
    assert (out.token_start[b, :L] == ref.token_start).all() and (out.token_end[b, :L] == ref.token_end).all(), b
    d_tok = float(np.abs(out.token_score[b, :L].astype(np.float64) - ref.token_score).max()) if L else 0.0
    d_tot = abs(float(out.score[b]) - ref.score)
    assert d_tok <= SCORE_TOL, (b, d_tok)
    assert d_tot <= TOTAL_TOL, (b, d_tot, ref.score)
    return d_tok, d_tot


def check_exact(x, y, blank, lengths, tlens, dev, label=""):
    B, T, V = x.shape
    out = run_device(x, y, blank, lengths, tlens, dev)
    worst = (0.0, 0.0)
    for b in range(B):
        n = T if lengths is None else int(min(max(lengths[b], 0), T))
        L = y.shape[1] if tlens is None else int(min(max(tlens[b], 0), y.shape[1]))
        yb = y[b, :L].tolist()
        ref = R.align(x[b], yb, blank, n)
        check_padding(out, b, n, L, ref.ok)
        if not ref.ok:
            continue
        assert (out.frame_tokens[b, :n] == ref.frame_tokens).all(), (label, b)
        assert (out.frame_index[b, :n] == ref.frame_index).all(), (label, b)
        assert (device_states(out, b, n, L) == ref.states).all(), (label, b)
        worst = tuple(max(a, c) for a, c in zip(worst, check_scores(out, b, ref, L)))
    print(f"[ctc_align exact {label}] B={B} T={T} V={V} Lmax={y.shape[1]}: token_score diff {worst[0]:.2e}, score diff {worst[1]:.2e}")
    return out


# (B, T, V, Lmax, grid, seed): P = 1 (Lmax 60 / 63), 2 (64), 8 (300), 16 (1023: the last one-wave shape), the workgroup
# form from 1024 on up to the limit 4096; V = 370; B = 1 and 32; ragged lengths with 0 and T, target lengths with 0 and Lmax
EXACT = [
    (1, 1, 5, 1, "g6", 1),
    (3, 7, 4, 3, "int", 2),
    (32, 249, 370, 60, "g6", 3),
    (32, 249, 370, 60, "int", 4),
    (5, 300, 7, 63, "g6", 5),
    (5, 300, 7, 64, "int", 6),
    (3, 2048, 4, 300, "g6", 7),
    (3, 2048, 4, 300, "int", 8),
    (1, 700, 9, 130, "g6", 9),
    (3, 2048, 6, 1023, "g6", 10),
    (3, 2048, 6, 1024, "g6", 11),
    (3, 1500, 5, 1023, "int", 12),
    (3, 1500, 5, 1024, "int", 13),
    (2, 2048, 5, 1500, "g6", 14),
    (2, 6000, 6, 4096, "g4", 15),
]


@pytest.mark.parametrize("B,T,V,Lmax,kind,seed", EXACT)
def test_exact_path_on_grid_inputs(dev, B, T, V, Lmax, kind, seed):
    rng = np.random.default_rng(seed)
    x = grid(rng, (B, T, V), kind)
    blank = seed % 2 if V > 2 else 0
    lengths = ragged(rng, B, T)
    tlens = ragged(rng, B, Lmax)
    if B > 2:
        tlens[0], tlens[1], tlens[2], lengths[1], lengths[2] = Lmax, min(Lmax, 2), 0, T, T // 2     # 0 and Lmax on live rows
    y = make_targets(rng, B, Lmax, V, blank, tlens)
    check_exact(x, y, blank, lengths, tlens, dev, kind)


def test_exact_path_long_form(dev):
    """T = 16384, L = 2048 on the 2^-4 grid in [-8,8]: partial sums stay below 2^24 * 2^-4."""
    rng = np.random.default_rng(40)
    x = grid(rng, (1, 16384, 6), "g4")
    y = make_targets(rng, 1, 2048, 6, 0, [2048])
    check_exact(x, y, 0, None, None, dev, "long-form")


def test_no_target_slots_and_default_lengths(dev):
    rng = np.random.default_rng(41)
    x = grid(rng, (2, 9, 4), "int")
    out = check_exact(x, np.zeros((2, 0), dtype=np.int64), 1, None, None, dev, "Lmax=0")
    assert (out.frame_tokens == 1).all() and (out.frame_index == -1).all() and out.ok.all()
    y = make_targets(rng, 2, 3, 4, 1, [3, 3])
    check_exact(x, y, 1, None, None, dev, "lengths=None")


# (B, T, V, Lmax, seed)
REAL = [(32, 249, 370, 60, 50), (4, 2048, 6, 300, 51), (3, 2048, 12, 1023, 52), (3, 2048, 12, 1024, 53), (1, 16384, 8, 2048, 54),
        (2, 6000, 5, 4096, 55)]


@pytest.mark.parametrize("B,T,V,Lmax,seed", REAL)
def test_real_valued_inputs_give_a_valid_near_optimal_path(dev, B, T, V, Lmax, seed):
    rng = np.random.default_rng(seed)
    x = grid(rng, (B, T, V), "randn")
    lengths = ragged(rng, B, T, lo=T // 2)
    if B > 1:
        lengths[1] = T - 1
    tlens = np.full(B, Lmax, dtype=np.int64) if B == 1 else ragged(rng, B, Lmax)
    if B > 1:
        tlens[1] = Lmax // 2
    y = make_targets(rng, B, Lmax, V, 0, tlens)
    out = run_device(x, y, 0, lengths, tlens, dev)
    worst_gap, same = 0.0, 0
    for b in range(B):
        n, L = int(lengths[b]), int(tlens[b])
        yb = y[b, :L].tolist()
        ref = R.align(x[b], yb, 0, n)
        check_padding(out, b, n, L, ref.ok)
        if not ref.ok:
            continue
        st = device_states(out, b, n, L)
        assert R.valid_path(yb, st), b
        assert R.collapse(out.frame_tokens[b, :n].tolist(), 0) == yb, b
        assert (out.frame_tokens[b, :n] == R.state_symbols(yb, 0)[st]).all()
        gap = R.path_score(x[b, :n], yb, 0, ref.states) - R.path_score(x[b, :n], yb, 0, st)
        bound = 2 * n * 2.0 ** -23 * (n * float(np.abs(x[b, :n]).max()))
        print(f"[ctc_align real] T={n} L={L} V={V}: score gap {gap:.3e} (bound {bound:.3e}), same path: {bool((st == ref.states).all())}")
        assert -1e-9 * n <= gap <= bound, (b, gap, bound)
        worst_gap, same = max(worst_gap, gap), same + int((st == ref.states).all())
        check_scores(out, b, R.outputs_of(x[b, :n], yb, 0, st), L)                     # the scores of the path it returned
    print(f"[ctc_align real] B={B} T={T} V={V} Lmax={Lmax}: largest gap {worst_gap:.3e}, {same} paths equal the restatement's")


@pytest.mark.parametrize("B,T,V", [(3, 400, 12), (2, 3000, 40)])
def test_aligning_the_collapsed_argmax_returns_the_argmax(dev, B, T, V):
    """Per frame a permutation of grid values (unique arg-max); the target is the standard CTC collapse of the arg-max
    sequence, computed with torch; no other path can score higher, so frame_tokens must be that sequence."""
    g = torch.Generator().manual_seed(60 + T)
    x = torch.stack([torch.stack([torch.randperm(V, generator=g) for _ in range(T)]) for _ in range(B)]).float() / 4.0
    am = x.argmax(-1)
    blank = 2
    ys = []
    for b in range(B):
        merged = torch.unique_consecutive(am[b])
        ys.append(merged[merged != blank])
    Lmax = max(len(v) for v in ys)
    y = torch.full((B, Lmax), 1 << 33, dtype=torch.int64)
    for b, v in enumerate(ys):
        y[b, :len(v)] = v
    tl = torch.tensor([len(v) for v in ys])
    out = ctc_forced_align(x.to(dev), y.to(dev), blank, None, tl.to(dev))
    assert bool(out.ok.all())
    assert torch.equal(out.frame_tokens.cpu(), am)


def test_padding_infeasible_rows_and_guarded_buffers(dev):
    """Infeasible rows (no frames; fewer frames than labels + repeats) between feasible ones, garbage target lengths and
    lengths, in both kernel forms: the padding is as tabulated, neighbours are untouched, and nothing is written outside
    the outputs and the workspace."""
    rng = np.random.default_rng(70)
    for Lmax, T in ((6, 40), (1100, 1700)):
        B, V = 6, 5
        x = grid(rng, (B, T, V), "g6")
        lengths = np.array([T, 0, 3, T + 1000, T, -5], dtype=np.int64)                 # clamped: T+1000 -> T, -5 -> 0
        tlens = np.array([Lmax, 2, Lmax, Lmax + 77, 0, 1], dtype=np.int64)             # clamped: Lmax+77 -> Lmax
        y = make_targets(rng, B, Lmax, V, 0, np.minimum(tlens, Lmax))
        y[2, :4] = 3                                                                   # repeats: 3 frames cannot hold them
        with guarded_allocations() as guard:
            saved, A.torch = A.torch, guard
            try:
                out = check_exact(x, y, 0, lengths, tlens, dev, f"guarded Lmax={Lmax}")
                bad = guard.check()
            finally:
                A.torch = saved
        assert len(guard.allocs) >= 8 and not bad, bad
        assert out.ok.tolist() == [True, False, False, True, True, False]


def test_argument_errors(dev):
    from conformer_amd._lib import ConformerHipError
    x = torch.zeros(2, 8, 5, device=dev)
    y = torch.ones(2, 3, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        ctc_forced_align(x, y, 5)
    with pytest.raises(ValueError):
        ctc_forced_align(x, y, -1)
    with pytest.raises(ValueError):
        ctc_forced_align(x, y[:1], 0)
    with pytest.raises(ConformerHipError):
        ctc_forced_align(x, y.int(), 0)
    with pytest.raises(ConformerHipError):
        ctc_forced_align(x, y.cpu(), 0)
    with pytest.raises(ValueError):
        ctc_forced_align(x, torch.ones(2, 4097, dtype=torch.int64, device=dev), 0)
    with pytest.raises(ValueError):
        ctc_forced_align(torch.zeros(1, 16385, 2, device=dev), y[:1], 0)
    with pytest.raises(ValueError):
        ctc_forced_align(x, y, 0, torch.ones(3, dtype=torch.int64, device=dev))
    out = ctc_forced_align(x.transpose(0, 1).contiguous().transpose(0, 1), y, 0)       # non-contiguous logits are copied
    assert bool(out.ok.all())


def test_capture_in_a_graph_and_replay_with_new_logits(dev):
    rng = np.random.default_rng(80)
    B, T, V, Lmax = 4, 200, 9, 40
    tl = torch.tensor([40, 17, 0, 33], device=dev)
    ln = torch.tensor([200, 150, 9, 20], device=dev)                                   # the last row is infeasible
    y = torch.from_numpy(make_targets(rng, B, Lmax, V, 0, tl.cpu().numpy())).to(dev)
    static_x = torch.from_numpy(grid(rng, (B, T, V), "g6")).to(dev)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ctc_forced_align(static_x, y, 0, ln, tl)
        side.synchronize()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ctc_forced_align(static_x, y, 0, ln, tl)
    for seed in (81, 82):
        new = torch.from_numpy(grid(np.random.default_rng(seed), (B, T, V), "g6")).to(dev)
        static_x.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        eager = ctc_forced_align(new, y, 0, ln, tl)
        for got, want in zip(captured, eager):
            assert torch.equal(got, want)
    assert captured.ok.tolist() == [True, True, True, False]


VOCAB = ["<pad>"] + [chr(ord("a") + i) for i in range(12)] + ["|", "<unk>"]


def test_end_to_end_words_of_a_beam_search_result(dev):
    """The smoke configuration's Conformer on random mel input: BeamCTCDecoder gives the text, CTCAligner.hypotheses the
    words of the best hypothesis.  They read the same text; spans are ordered, disjoint and inside the utterance; the
    frames collapse to the decoded ids."""
    from conformer_amd.decode import BeamCTCDecoder, beam_ctc_decode
    from model.conformer import Conformer
    from oracle import conformer_oracle as O
    V = len(VOCAB)
    P = O.make_params(vocab=V, n_mel=80, n_blocks=2, d=32, n_heads=4, ksize=31, lstm_hidden=24, seed=31)
    m = Conformer(V, 80, 2, 32, 4, 31, 24, 1, 0.0)
    m.load_state_dict(P, strict=True)
    m = m.to(dev).eval()
    g = torch.Generator().manual_seed(90)
    mel = torch.randn(3, 80, 203, generator=g).to(dev)
    mel_len = torch.tensor([203, 160, 75], device=dev)
    with torch.no_grad():
        logits, out_len = m(mel, mel_len)
    logits = (logits.float() * 6).contiguous()               # random weights give flat logits: sharpen them so that text comes out
    dec = BeamCTCDecoder(VOCAB, 0, skip_ids=(V - 1,), beam_width=32)
    texts = dec(logits, out_len)
    tokens, counts = beam_ctc_decode(logits, 0, out_len, beam_width=32, n_best=1, token_min_logp=dec.token_min_logp,
                                     beam_prune_logp=dec.beam_prune_logp, max_candidates=dec.max_candidates)[:2]
    aligner = CTCAligner.from_decoder(dec)
    words = aligner.hypotheses(logits, tokens, counts, out_len)
    assert any(texts), "the decoder returned no text at all: the test would show nothing"
    ids, al = aligner.align(logits, [tokens[b, 0, :int(counts[b, 0])].tolist() for b in range(3)], out_len)
    ft = al.frame_tokens.cpu().numpy()
    for b in range(3):
        n = int(out_len[b])
        assert " ".join(w.text for w in words[b]) == texts[b], (b, words[b], texts[b])
        prev_end = 0
        for w in words[b]:
            assert prev_end <= w.start_frame < w.end_frame <= n, (b, w)
            assert w.start == pytest.approx(w.start_frame * 0.04) and w.end == pytest.approx(w.end_frame * 0.04)
            assert -INF < w.score <= 0.0
            prev_end = w.end_frame
        assert bool(al.ok[b])
        assert R.collapse(ft[b, :n].tolist(), 0) == ids[b]
    # a transcript given as text aligns to the same words
    assert [[w.text for w in ws] for ws in aligner(logits, texts, out_len)] == [[w.text for w in ws] for ws in words]
