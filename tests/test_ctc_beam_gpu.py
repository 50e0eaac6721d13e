"""CTC prefix beam search on the MI355X (conformer_amd.decode.beam_ctc_decode / BeamCTCDecoder) against brute force and the
float64 restatement of tests/ctc_beam_restatement.py.

The device keeps the normaliser and the scores in fp64, so it agrees with the restatement to ~1e-12 on every score it
compares.  A decision can only come out differently where the restatement reports a margin (cut / prune / candidate /
order gap) below that error: the comparisons require every margin >= MARGIN, so a seed with a near-tie fails loudly."""
import math

import numpy as np
import pytest
import torch

from conformer_amd.decode import BeamCTCDecoder, beam_ctc_decode
from tests import ctc_beam_restatement as R
from tests.test_write_guard_gpu import guarded_allocations

pytestmark = pytest.mark.gpu
INF = math.inf
MARGIN = 1e-8          # >= 100x the device / restatement score difference (fp64 on both sides)
SCORE_TOL = 1e-4       # the returned scores are fp32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def ragged(B, T, rng):
    if B == 1:
        return np.array([T])
    L = rng.integers(0, T + 1, size=B)
    L[0], L[1] = T, 0
    return L


def check_against_restatement(x, lengths, blank, W, N, dev, **kw):
    """x (B,T,V) float32 numpy; runs the device and the restatement and compares hypotheses, scores and padding."""
    B, T, V = x.shape
    xt = torch.from_numpy(x).to(dev)
    Lt = None if lengths is None else torch.from_numpy(np.asarray(lengths, dtype=np.int64)).to(dev)
    tokens, counts, scores, num = (t.cpu() for t in beam_ctc_decode(xt, blank, Lt, beam_width=W, n_best=N, **kw))
    assert tokens.shape == (B, N, T) and counts.shape == (B, N) and scores.shape == (B, N) and num.shape == (B,)
    assert scores.dtype == torch.float32 and tokens.dtype == counts.dtype == num.dtype == torch.int64
    ref = R.restate_batch(x, blank, lengths, beam_width=W, n_best=N, **kw)
    for b, (hyps, margins) in enumerate(ref):
        assert R.min_margin(margins) >= MARGIN, (b, margins)
        assert int(num[b]) == len(hyps), (b, int(num[b]), len(hyps))
        for r, (seq, sc) in enumerate(hyps):
            n = int(counts[b, r])
            assert tuple(tokens[b, r, :n].tolist()) == seq, (b, r)
            assert abs(float(scores[b, r]) - sc) <= SCORE_TOL, (b, r, float(scores[b, r]), sc)
            assert bool((tokens[b, r, n:] == -1).all())
        for r in range(len(hyps), N):                              # unused rows hold their padding values
            assert int(counts[b, r]) == 0 and float(scores[b, r]) == -INF and bool((tokens[b, r] == -1).all())
    return tokens, counts, scores, num


@pytest.mark.parametrize("T", [1, 3, 5])
@pytest.mark.parametrize("blank", [0, 1])
def test_device_equals_brute_force_in_the_exact_regime(dev, T, blank):
    rng = np.random.default_rng(10 * T + blank)
    x = (rng.standard_normal((2, T, 3)) * 2).astype(np.float32)
    tokens, counts, scores, num = beam_ctc_decode(torch.from_numpy(x).to(dev), blank, beam_width=64, n_best=64,
                                                  max_candidates=2, token_min_logp=-INF, beam_prune_logp=-INF)
    for b in range(2):
        bf = R.brute_force(x[b], blank)
        got = {}
        for r in range(int(num[b])):
            if float(scores[b, r]) > -INF:
                got[tuple(tokens[b, r, :int(counts[b, r])].tolist())] = float(scores[b, r])
        assert set(got) == set(bf)
        for seq, sc in bf.items():
            assert abs(got[seq] - sc) <= 1e-5, (seq, got[seq], sc)


# (B, T, V, W, n_best, logit scale, seed): every B, T, V and W of the issue's grid appears; lengths are ragged with 0 and T
CASES = [
    (1, 1, 5, 1, 1, 1.0, 0),
    (3, 7, 5, 8, 4, 1.0, 1),
    (3, 7, 17, 256, 64, 1.0, 2),
    (3, 49, 17, 8, 8, 2.0, 3),
    (3, 49, 370, 190, 16, 2.0, 4),
    (32, 49, 17, 100, 4, 2.0, 5),
    (32, 249, 370, 100, 4, 2.0, 6),
    (3, 249, 370, 256, 8, 2.0, 7),
    (1, 249, 370, 190, 190, 2.0, 8),
    (32, 249, 5, 1, 1, 1.0, 9),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B{}_T{}_V{}_W{}".format(*c[:4]))
def test_device_equals_restatement_on_random_logits(dev, case):
    B, T, V, W, N, scale, seed = case
    rng = np.random.default_rng(1000 + seed)
    x = (rng.standard_normal((B, T, V)) * scale).astype(np.float32)
    check_against_restatement(x, ragged(B, T, rng), seed % V, W, N, dev)


def test_pruning_knobs_follow_the_restatement(dev):
    rng = np.random.default_rng(77)
    x = (rng.standard_normal((3, 49, 17)) * 2).astype(np.float32)
    L = ragged(3, 49, rng)
    check_against_restatement(x, L, 0, 32, 8, dev, max_candidates=3, token_min_logp=-3.0, beam_prune_logp=-6.0)
    check_against_restatement(x, L, 0, 16, 16, dev, max_candidates=32, token_min_logp=-INF, beam_prune_logp=-INF)


def test_ties_follow_the_origin_key_on_the_device(dev):
    x = torch.zeros(1, 1, 5, device=dev)
    tokens, counts, scores, num = beam_ctc_decode(x, 0, beam_width=8, n_best=8, max_candidates=3, token_min_logp=-INF,
                                                  beam_prune_logp=-INF)
    assert int(num[0]) == 4
    assert [tokens[0, r, :int(counts[0, r])].tolist() for r in range(4)] == [[], [1], [2], [3]]
    assert bool((scores[0, :4] == scores[0, 0]).all())
    tokens, counts, _, num = beam_ctc_decode(torch.zeros(1, 1, 5, device=dev), 2, beam_width=3, n_best=3, max_candidates=4,
                                             token_min_logp=-INF, beam_prune_logp=-INF)
    assert [tokens[0, r, :int(counts[0, r])].tolist() for r in range(3)] == [[], [0], [1]]


def test_peaky_logits_decode_to_the_ctc_collapse(dev):
    """One dominant id per frame: the best prefix is the standard-CTC collapse of the frame path (a blank separates
    repeats), which the reference-compatible greedy decoder does not produce."""
    rng = np.random.default_rng(11)
    B, T, V, blank = 8, 120, 29, 0
    path = rng.integers(0, V, size=(B, T))
    path[:, 1::7] = blank
    path[:, 3::11] = path[:, 2::11][:, :path[:, 3::11].shape[1]]          # repeats
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    np.put_along_axis(x, path[..., None], 12.0, axis=-1)
    tokens, counts, _, _ = beam_ctc_decode(torch.from_numpy(x).to(dev), blank, beam_width=16)
    for b in range(B):
        assert tuple(tokens[b, 0, :int(counts[b, 0])].tolist()) == R.collapse(path[b].tolist(), blank)


def test_bf16_logits_equal_their_fp32_cast(dev):
    g = torch.Generator().manual_seed(3)
    x16 = (torch.randn(4, 60, 33, generator=g) * 2).to(dev, torch.bfloat16)
    L = torch.tensor([60, 0, 31, 59], device=dev)
    a = beam_ctc_decode(x16, 1, L, beam_width=32, n_best=4)
    b = beam_ctc_decode(x16.float(), 1, L, beam_width=32, n_best=4)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_two_runs_are_bit_identical(dev):
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(32, 249, 370, generator=g) * 2).to(dev)
    L = torch.randint(0, 250, (32,), generator=g).to(dev)
    a = beam_ctc_decode(x, 0, L, beam_width=190, n_best=8)
    b = beam_ctc_decode(x, 0, L, beam_width=190, n_best=8)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_no_write_outside_outputs_and_workspace(dev):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(5, 49, 17, generator=g) * 2).to(dev)
    L = torch.tensor([49, 0, 13, 48, 1], device=dev)
    with guarded_allocations() as guard:
        for W, N in ((1, 1), (100, 100), (256, 7)):
            beam_ctc_decode(x, 3, L, beam_width=W, n_best=N)
        bad = guard.check()
    assert guard.allocs and not bad, bad


def test_conformer_logits_through_beam_decoder(dev):
    """End to end: a small Conformer forward on the device, then BeamCTCDecoder on its logits and output lengths; at W = 1
    with no pruning the text is the restatement's best prefix."""
    from model.conformer import Conformer
    from oracle import conformer_oracle as O
    vocab = ["<pad>"] + [chr(ord("a") + i) for i in range(14)] + ["|", "<unk>"]
    P = O.make_params(vocab=17, n_mel=80, n_blocks=2, d=32, n_heads=4, ksize=31, lstm_hidden=24, seed=31)
    m = Conformer(17, 80, 2, 32, 4, 31, 24, 1, 0.0)
    m.load_state_dict(P, strict=True)
    m = m.to(dev).eval()
    g = torch.Generator().manual_seed(32)
    x = torch.randn(3, 80, 103, generator=g)
    with torch.no_grad():
        logits, out_len = m(x.to(dev), torch.tensor([103, 80, 31]).to(dev))
    dec = BeamCTCDecoder(vocab, blank_id=0, skip_ids=(16,), beam_width=1, beam_prune_logp=-INF, token_min_logp=-INF,
                         max_candidates=16)
    texts = dec(logits, out_len)
    lg = logits.float().cpu().numpy()
    ref = R.restate_batch(lg, 0, out_len.cpu().numpy(), beam_width=1, max_candidates=16, token_min_logp=-INF,
                          beam_prune_logp=-INF)
    assert isinstance(texts, list) and len(texts) == 3
    for b, (hyps, margins) in enumerate(ref):
        assert R.min_margin(margins) >= MARGIN, margins
        assert texts[b] == dec.text(hyps[0][0])
    one = dec(logits[1], out_len[1:2].cpu().numpy())
    assert isinstance(one, str) and one == texts[1]
