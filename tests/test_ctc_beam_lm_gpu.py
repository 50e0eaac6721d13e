"""CTC beam search fused with a word n-gram model on the MI355X (conformer_amd.decode.beam_ctc_lm_decode, BeamCTCDecoder(lm=...),
NgramLanguageModel.score_sentences) against the float64 restatement of tests/ctc_beam_lm_restatement.py and brute force.

The device sums every score in fp64 from the same float32 table values, so it agrees with the restatement to ~1e-12; the
returned scores are fp32, so a returned score must equal the restatement's value to within 1e-9 plus half an fp32 ulp.
Decisions can only differ where the restatement reports a margin below the fp64 error: every margin must be >= MARGIN."""
import math

import numpy as np
import pytest
import torch

from conformer_amd.decode import BeamCTCDecoder, beam_ctc_decode, beam_ctc_lm_decode
from conformer_amd.lm import NgramLanguageModel, write_synthetic_arpa
from tests import ctc_beam_lm_restatement as LR
from tests import ctc_beam_restatement as R
from tests.test_ctc_beam_lm_cpu import ARPA3, HAND, VOCAB
from tests.test_write_guard_gpu import guarded_allocations

pytestmark = pytest.mark.gpu
INF = math.inf
MARGIN = 1e-8


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def close32(got: float, want: float) -> bool:
    """an fp32 output of an fp64 value within 1e-9 of `want`"""
    if want == -INF:
        return got == -INF
    return abs(got - want) <= 1e-9 + 0.5 * float(np.spacing(np.float32(abs(want))))


@pytest.fixture(scope="module")
def arpa3(tmp_path_factory):
    p = tmp_path_factory.mktemp("lm") / "m3.arpa"
    p.write_text(ARPA3, encoding="utf-8")
    return str(p)


# a grapheme vocabulary: blank, letters, two multi-character tokens, the delimiter, <unk>
TOKS = [chr(ord("A") + i) for i in range(14)] + ["TH", "CH"]
GVOCAB = ["<pad>"] + TOKS + ["|", "<unk>"]
G_UNK = len(GVOCAB) - 1


@pytest.fixture(scope="module")
def small_lm(tmp_path_factory):
    """a 4-gram over 60 words spelled in TOKS (short words, so random logits complete many of them)"""
    p = tmp_path_factory.mktemp("lm") / "small.arpa"
    write_synthetic_arpa(p, TOKS, 60, [0, 300, 400, 300], seed=7, max_tokens_per_word=2)
    return str(p), NgramLanguageModel.from_arpa(p), LR.Arpa.read(str(p))


def test_device_scorer_matches_hand_values(dev, arpa3):
    lm = NgramLanguageModel.from_arpa(arpa3)
    ref = LR.Arpa.read(arpa3)
    sents = [list(h) + [w] for w, h, _ in HAND if "<s>" not in h] + [["A", "B"], ["Q"], []]
    got = lm.score_sentences(sents, boundary=False, device=dev).cpu().numpy()
    for s, g in zip(sents, got):
        assert abs(g - ref.sentence(s, boundary=False)) <= 1e-9, (s, g)
    got = lm.score_sentences([["A", "B"], ["A", "AB"], []], boundary=True, device=dev).cpu().numpy()
    assert abs(got[0] - (-0.4 + -0.2 + -0.1)) <= 1e-6
    for s, g in zip([["A", "B"], ["A", "AB"], []], got):
        assert abs(g - ref.sentence(s)) <= 1e-9


def test_device_scorer_on_every_ngram_of_a_5gram_model(dev, tmp_path):
    p = tmp_path / "big.arpa.gz"
    write_synthetic_arpa(p, TOKS, 3000, [0, 20000, 16000, 10000, 6000], seed=11)
    lm = NgramLanguageModel.from_arpa(p)
    ref = LR.Arpa.read(str(p))
    assert sum(lm.counts) >= 50000
    sents = [[lm.words[i] for i in row] for ids, _, _ in lm.ngrams for row in ids]
    got = lm.score_sentences(sents, boundary=False, device=dev).cpu().numpy()
    want = np.array([ref.sentence(s, boundary=False) for s in sents])
    assert np.max(np.abs(got - want)) <= 1e-9
    # random sentences with OOV words, with and without <s> / </s>
    rng = np.random.default_rng(12)
    pool = lm.words[3:] + ["ZZZ", "QQ", "<unk>"]
    rs = [[pool[i] for i in rng.integers(0, len(pool), size=rng.integers(0, 12))] for _ in range(2000)]
    for boundary in (True, False):
        got = lm.score_sentences(rs, boundary=boundary, device=dev).cpu().numpy()
        want = np.array([ref.sentence(s, boundary=boundary) for s in rs])
        assert np.max(np.abs(got - want)) <= 1e-9


def run(x, lengths, blank, lm, vocab, dev, **kw):
    xt = torch.from_numpy(x).to(dev) if isinstance(x, np.ndarray) else x
    Lt = None if lengths is None else torch.from_numpy(np.asarray(lengths, dtype=np.int64)).to(dev)
    return [t.cpu() for t in beam_ctc_lm_decode(xt, blank, lm, Lt, vocab=vocab, **kw)]


@pytest.mark.parametrize("T", [1, 2, 4])
def test_device_equals_brute_force_in_the_exact_regime(dev, arpa3, T):
    rng = np.random.default_rng(40 + T)
    x = (rng.standard_normal((2, T, 4)) * 2).astype(np.float32)
    f = LR.Fusion(LR.Arpa.read(arpa3), VOCAB)
    tokens, counts, scores, am, num = run(x, None, 0, arpa3, VOCAB, dev, beam_width=256, n_best=256, max_candidates=3,
                                          token_min_logp=-INF, beam_prune_logp=-INF)
    for b in range(2):
        bf = LR.brute_force(x[b], 0, f)
        amb = R.brute_force(x[b], 0)
        got = {}
        for r in range(int(num[b])):
            if float(am[b, r]) > -INF:
                got[tuple(tokens[b, r, :int(counts[b, r])].tolist())] = (float(scores[b, r]), float(am[b, r]))
        assert set(got) == set(bf)
        for seq, sc in bf.items():
            assert abs(got[seq][0] - sc) <= 1e-4 and abs(got[seq][1] - amb[seq]) <= 1e-5, (seq, got[seq], sc)


def check_against_restatement(x, lengths, blank, lm_path, ref_lm, vocab, W, N, dev, skip_ids=(), **kw):
    B, T, V = x.shape
    fz = {k: kw.pop(k) for k in ("alpha", "beta", "unk_score_offset", "score_boundary") if k in kw}
    tokens, counts, scores, am, num = run(x, lengths, blank, lm_path, vocab, dev, skip_ids=skip_ids, beam_width=W,
                                          n_best=N, **fz, **kw)
    assert tokens.shape == (B, N, T) and scores.dtype == am.dtype == torch.float32
    f = LR.Fusion(ref_lm, vocab, skip_ids=skip_ids, **fz)
    ref = LR.restate_batch(x, blank, f, lengths, beam_width=W, n_best=N, **kw)
    for b, (hyps, margins) in enumerate(ref):
        assert R.min_margin(margins) >= MARGIN, (b, margins)
        assert int(num[b]) == len(hyps), (b, int(num[b]), len(hyps))
        for r, (seq, sc, a) in enumerate(hyps):
            n = int(counts[b, r])
            assert tuple(tokens[b, r, :n].tolist()) == seq, (b, r)
            assert close32(float(scores[b, r]), sc), (b, r, float(scores[b, r]), sc)
            assert close32(float(am[b, r]), a), (b, r, float(am[b, r]), a)
            assert bool((tokens[b, r, n:] == -1).all())
        for r in range(len(hyps), N):
            assert int(counts[b, r]) == 0 and float(scores[b, r]) == -INF and float(am[b, r]) == -INF
            assert bool((tokens[b, r] == -1).all())
    return tokens, counts, scores, am, num


# (B, T, W, n_best, logit scale, beam_prune_logp, seed): a wide prune threshold keeps the beams of W = 100 and 256 full
CASES = [(1, 9, 1, 1, 1.0, -10.0, 0), (3, 49, 16, 8, 2.0, -10.0, 1), (3, 49, 100, 16, 2.0, -40.0, 2),
         (2, 30, 256, 64, 2.0, -40.0, 3)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B{}_T{}_W{}".format(*c[:3]))
def test_device_equals_restatement_on_random_logits(dev, small_lm, case):
    B, T, W, N, scale, prune, seed = case
    path, _, ref = small_lm
    rng = np.random.default_rng(2000 + seed)
    x = (rng.standard_normal((B, T, len(GVOCAB))) * scale).astype(np.float32)
    L = np.array([T]) if B == 1 else np.concatenate([[T, 0], rng.integers(0, T + 1, size=B - 2)])
    check_against_restatement(x, L, 0, path, ref, GVOCAB, W, N, dev, skip_ids=(G_UNK,), beam_prune_logp=prune)


def test_fusion_knobs_follow_the_restatement(dev, small_lm):
    path, _, ref = small_lm
    rng = np.random.default_rng(77)
    x = (rng.standard_normal((3, 40, len(GVOCAB))) * 2).astype(np.float32)
    L = np.array([40, 0, 23])
    check_against_restatement(x, L, 0, path, ref, GVOCAB, 32, 8, dev, alpha=0.5, beta=1.5, unk_score_offset=-4.0,
                              score_boundary=False, max_candidates=5, token_min_logp=-4.0, beam_prune_logp=-12.0)


def test_zero_weight_lm_is_bit_identical_to_the_lm_free_search(dev, small_lm):
    path, lm, _ = small_lm
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(6, 80, len(GVOCAB), generator=g) * 2).to(dev)
    L = torch.tensor([80, 0, 1, 57, 79, 33], device=dev)
    for W, N in ((1, 1), (64, 8), (256, 32)):
        a = beam_ctc_decode(x, 0, L, beam_width=W, n_best=N)
        tk, ct, sc, am, nh = beam_ctc_lm_decode(x, 0, lm, L, vocab=GVOCAB, skip_ids=(G_UNK,), alpha=0.0, beta=0.0,
                                                unk_score_offset=0.0, beam_width=W, n_best=N)
        for u, v in zip(a, (tk, ct, sc, nh)):
            assert torch.equal(u, v)
        assert torch.equal(am, sc)


def test_lm_changes_the_best_hypothesis(dev, arpa3):
    # acoustically "B" wins; the model's word A wins the fused search
    x = np.log(np.array([[[0.05, 0.42, 0.5, 0.03]]], dtype=np.float64)).astype(np.float32)
    t0, c0, s0, _ = (u.cpu() for u in beam_ctc_decode(torch.from_numpy(x).to(dev), 0, beam_width=8, n_best=8,
                                                      token_min_logp=-INF, beam_prune_logp=-INF))
    assert t0[0, 0, :int(c0[0, 0])].tolist() == [2]
    tokens, counts, scores, am, _ = run(x, None, 0, arpa3, VOCAB, dev, alpha=2.0, beta=0.0, beam_width=8, n_best=8,
                                        token_min_logp=-INF, beam_prune_logp=-INF)
    assert tokens[0, 0, :int(counts[0, 0])].tolist() == [1]
    assert float(am[0, 0]) < float(s0[0, 0])            # the LM, not the acoustics, put it first
    ref, margins = LR.beam_search(x[0], 0, LR.Fusion(LR.Arpa.read(arpa3), VOCAB, alpha=2.0, beta=0.0), 8, n_best=8,
                                  token_min_logp=-INF, beam_prune_logp=-INF)
    assert ref[0][0] == (1,) and close32(float(scores[0, 0]), ref[0][1])


def test_bf16_logits_equal_their_fp32_cast_and_runs_are_bit_identical(dev, small_lm):
    _, lm, _ = small_lm
    g = torch.Generator().manual_seed(3)
    x16 = (torch.randn(4, 60, len(GVOCAB), generator=g) * 2).to(dev, torch.bfloat16)
    L = torch.tensor([60, 0, 31, 59], device=dev)
    kw = dict(vocab=GVOCAB, skip_ids=(G_UNK,), beam_width=32, n_best=4)
    a = beam_ctc_lm_decode(x16, 1, lm, L, **kw)
    b = beam_ctc_lm_decode(x16.float(), 1, lm, L, **kw)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    x = (torch.randn(32, 249, len(GVOCAB), generator=g) * 2).to(dev)
    L = torch.randint(0, 250, (32,), generator=g).to(dev)
    a = beam_ctc_lm_decode(x, 0, lm, L, vocab=GVOCAB, skip_ids=(G_UNK,), beam_width=190, n_best=8)
    b = beam_ctc_lm_decode(x, 0, lm, L, vocab=GVOCAB, skip_ids=(G_UNK,), beam_width=190, n_best=8)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_no_write_outside_outputs_and_workspace(dev, small_lm):
    _, lm, _ = small_lm
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(5, 49, len(GVOCAB), generator=g) * 2).to(dev)
    L = torch.tensor([49, 0, 13, 48, 1], device=dev)
    with guarded_allocations() as guard:
        for W, N in ((1, 1), (100, 100), (256, 7)):
            beam_ctc_lm_decode(x, 3, lm, L, vocab=GVOCAB, skip_ids=(G_UNK,), beam_width=W, n_best=N)
        bad = guard.check()
    assert guard.allocs and not bad, bad


def test_conformer_logits_through_beam_decoder_with_lm(dev, tmp_path):
    """End to end: a small Conformer forward, then BeamCTCDecoder(lm=<ARPA path>) on its logits; at W = 1 with no pruning
    the text is the restatement's best hypothesis."""
    from model.conformer import Conformer
    from oracle import conformer_oracle as O
    vocab = ["<pad>"] + [chr(ord("a") + i) for i in range(14)] + ["|", "<unk>"]
    arpa = tmp_path / "c.arpa"
    write_synthetic_arpa(arpa, vocab[1:15], 50, [0, 200, 200], seed=21, max_tokens_per_word=2)
    P = O.make_params(vocab=17, n_mel=80, n_blocks=2, d=32, n_heads=4, ksize=31, lstm_hidden=24, seed=31)
    m = Conformer(17, 80, 2, 32, 4, 31, 24, 1, 0.0)
    m.load_state_dict(P, strict=True)
    m = m.to(dev).eval()
    g = torch.Generator().manual_seed(32)
    x = torch.randn(3, 80, 103, generator=g)
    with torch.no_grad():
        logits, out_len = m(x.to(dev), torch.tensor([103, 80, 31]).to(dev))
    dec = BeamCTCDecoder(vocab, blank_id=0, skip_ids=(16,), beam_width=1, beam_prune_logp=-INF, token_min_logp=-INF,
                         max_candidates=16, lm=str(arpa), alpha=0.5, beta=1.0)
    texts = dec(logits, out_len)
    f = LR.Fusion(LR.Arpa.read(str(arpa)), vocab, skip_ids=(16,), alpha=0.5, beta=1.0)
    ref = LR.restate_batch(logits.float().cpu().numpy(), 0, f, out_len.cpu().numpy(), beam_width=1, max_candidates=16,
                           token_min_logp=-INF, beam_prune_logp=-INF)
    assert isinstance(texts, list) and len(texts) == 3
    for b, (hyps, margins) in enumerate(ref):
        assert R.min_margin(margins) >= MARGIN, margins
        assert texts[b] == dec.text(hyps[0][0])
    one = dec(logits[1], out_len[1:2].cpu().numpy())
    assert isinstance(one, str) and one == texts[1]
