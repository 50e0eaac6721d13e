"""CTC beam search with hotword boosting on the MI355X (conformer_amd.decode.beam_ctc_hotword_decode, BeamCTCDecoder(hotwords=...))
against the float64 restatement of tests/ctc_beam_hotword_restatement.py (count by re.findall) and brute force, with and
without the word n-gram model.

As in tests/test_ctc_beam_lm_gpu.py: every score is fp64 on the device, so a returned fp32 score must equal the restatement's
value to within 1e-9 plus half an fp32 ulp, and every decision margin of the restatement must be >= MARGIN."""
import math

import numpy as np
import pytest
import torch

from conformer_amd.decode import BeamCTCDecoder, beam_ctc_decode, beam_ctc_hotword_decode, beam_ctc_lm_decode
from conformer_amd.lm import NgramLanguageModel, write_synthetic_arpa
from tests import ctc_beam_hotword_restatement as HR
from tests import ctc_beam_lm_restatement as LR
from tests import ctc_beam_restatement as R
from tests.test_ctc_beam_lm_cpu import ARPA3
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
    if want == -INF:
        return got == -INF
    return abs(got - want) <= 1e-9 + 0.5 * float(np.spacing(np.float32(abs(want))))


# blank, letters, multi-character and non-ASCII tokens, the delimiter, <unk>
TOKS = [chr(ord("A") + i) for i in range(10)] + ["TH", "É", "ßA"]
GVOCAB = ["<pad>"] + TOKS + ["|", "<unk>"]
G_UNK = len(GVOCAB) - 1
# overlapping multi-word and non-ASCII phrases over short words random logits complete often
PHRASES = ["A", "B C", "A B", "ÉA", "THE", "C D E", "A B C D", "ßAB", "D", "É É", "CA B", "  B   C  ", "THÉ ßA"]


@pytest.fixture(scope="module")
def small_lm(tmp_path_factory):
    """a 3-gram over 40 words spelled in TOKS, plus every hotword unigram"""
    p = tmp_path_factory.mktemp("lm") / "small.arpa"
    words = write_synthetic_arpa(p, TOKS, 40, [0, 200, 200], seed=9, max_tokens_per_word=2)
    uni = sorted({w for ph in PHRASES for w in ph.split()} - set(words))
    text = p.read_text(encoding="utf-8")
    n1 = int(text.split("ngram 1=")[1].split()[0])
    text = text.replace(f"ngram 1={n1}", f"ngram 1={n1 + len(uni)}", 1)
    text = text.replace("\\1-grams:\n", "\\1-grams:\n" + "".join(f"-2.5\t{w}\t-0.3\n" for w in uni), 1)
    p.write_text(text, encoding="utf-8")
    return str(p), NgramLanguageModel.from_arpa(p), LR.Arpa.read(str(p))


def run(x, lengths, blank, phrases, vocab, dev, **kw):
    xt = torch.from_numpy(x).to(dev) if isinstance(x, np.ndarray) else x
    Lt = None if lengths is None else torch.from_numpy(np.asarray(lengths, dtype=np.int64)).to(dev)
    return [t.cpu() for t in beam_ctc_hotword_decode(xt, blank, phrases, Lt, vocab=vocab, **kw)]


def fusion(phrases, vocab, weight, ref_lm=None, skip_ids=(), **lmkw):
    lm = None if ref_lm is None else LR.Fusion(ref_lm, vocab, skip_ids=skip_ids, **lmkw)
    return HR.Fusion(phrases, vocab, skip_ids=skip_ids, weight=weight, lm=lm)


@pytest.mark.parametrize("T", [1, 2, 4])
@pytest.mark.parametrize("with_lm", [False, True], ids=["nolm", "lm"])
def test_device_equals_brute_force_in_the_exact_regime(dev, tmp_path, T, with_lm):
    vocab = ["_", "A", "B", "|"]
    phrases = ["A", "AB", "A B", "BB"]
    rng = np.random.default_rng(60 + T)
    x = (rng.standard_normal((2, T, 4)) * 2).astype(np.float32)
    arpa, ref = None, None
    if with_lm:
        arpa = tmp_path / "m3.arpa"
        arpa.write_text(ARPA3, encoding="utf-8")
        ref = LR.Arpa.read(str(arpa))
        arpa = str(arpa)
    f = fusion(phrases, vocab, 2.5, ref, alpha=0.7, beta=0.5)
    tokens, counts, scores, am, num = run(x, None, 0, phrases, vocab, dev, hotword_weight=2.5, lm=arpa, alpha=0.7, beta=0.5,
                                          beam_width=256, n_best=256, max_candidates=3, token_min_logp=-INF,
                                          beam_prune_logp=-INF)
    for b in range(2):
        bf = HR.brute_force(x[b], 0, f)
        amb = R.brute_force(x[b], 0)
        got = {}
        for r in range(int(num[b])):
            if float(am[b, r]) > -INF:
                got[tuple(tokens[b, r, :int(counts[b, r])].tolist())] = (float(scores[b, r]), float(am[b, r]))
        assert set(got) == set(bf)
        for seq, sc in bf.items():
            assert abs(got[seq][0] - sc) <= 1e-4 and abs(got[seq][1] - amb[seq]) <= 1e-5, (seq, got[seq], sc)


def check_against_restatement(x, lengths, blank, phrases, weight, vocab, W, N, dev, lm=None, skip_ids=(), **kw):
    B, T, V = x.shape
    path, ref = lm if lm is not None else (None, None)
    lmkw = {k: kw.pop(k) for k in ("alpha", "beta", "unk_score_offset", "score_boundary") if k in kw}
    tokens, counts, scores, am, num = run(x, lengths, blank, phrases, vocab, dev, hotword_weight=weight, lm=path,
                                          skip_ids=skip_ids, beam_width=W, n_best=N, **lmkw, **kw)
    assert tokens.shape == (B, N, T) and scores.dtype == am.dtype == torch.float32
    f = fusion(phrases, vocab, weight, ref, skip_ids=skip_ids, **lmkw)
    ref_out = HR.restate_batch(x, blank, f, lengths, beam_width=W, n_best=N, **kw)
    for b, (hyps, margins) in enumerate(ref_out):
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


# (B, T, W, n_best, logit scale, beam_prune_logp, weight, seed)
CASES = [(1, 9, 1, 1, 1.0, -10.0, 9.0, 0), (3, 49, 16, 8, 2.0, -10.0, 9.0, 1), (3, 49, 100, 16, 2.0, -40.0, 3.0, 2),
         (2, 30, 256, 64, 2.0, -40.0, 9.0, 3), (3, 40, 16, 8, 2.0, -15.0, -4.0, 4), (2, 40, 32, 8, 2.0, -30.0, 40.0, 5)]


@pytest.mark.parametrize("with_lm", [False, True], ids=["nolm", "lm"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "B{}_T{}_W{}_w{}".format(c[0], c[1], c[2], c[6]))
def test_device_equals_restatement_on_random_logits(dev, small_lm, case, with_lm):
    B, T, W, N, scale, prune, weight, seed = case
    rng = np.random.default_rng(3000 + seed)
    x = (rng.standard_normal((B, T, len(GVOCAB))) * scale).astype(np.float32)
    L = np.array([T]) if B == 1 else np.concatenate([[T, 0], rng.integers(0, T + 1, size=B - 2)])
    lm = (small_lm[0], small_lm[2]) if with_lm else None
    check_against_restatement(x, L, 0, PHRASES, weight, GVOCAB, W, N, dev, lm=lm, skip_ids=(G_UNK,), beam_prune_logp=prune)


def test_knobs_follow_the_restatement(dev, small_lm):
    rng = np.random.default_rng(78)
    x = (rng.standard_normal((3, 40, len(GVOCAB))) * 2).astype(np.float32)
    check_against_restatement(x, np.array([40, 0, 23]), 0, PHRASES, 5.0, GVOCAB, 32, 8, dev, lm=(small_lm[0], small_lm[2]),
                              skip_ids=(G_UNK,), alpha=0.5, beta=1.5, unk_score_offset=-4.0, score_boundary=False,
                              max_candidates=5, token_min_logp=-4.0, beam_prune_logp=-12.0)


def test_zero_weight_is_bit_identical_to_the_unboosted_searches(dev, small_lm):
    _, lm, _ = small_lm
    g = torch.Generator().manual_seed(18)
    x = (torch.randn(6, 80, len(GVOCAB), generator=g) * 2).to(dev)
    L = torch.tensor([80, 0, 1, 57, 79, 33], device=dev)
    kw = dict(vocab=GVOCAB, skip_ids=(G_UNK,), hotword_weight=0.0)
    for W, N in ((1, 1), (64, 8), (256, 32)):
        a = beam_ctc_decode(x, 0, L, beam_width=W, n_best=N)
        tk, ct, sc, am, nh = beam_ctc_hotword_decode(x, 0, PHRASES, L, beam_width=W, n_best=N, **kw)
        for u, v in zip(a, (tk, ct, sc, nh)):
            assert torch.equal(u, v)
        assert torch.equal(am, sc)
        b = beam_ctc_lm_decode(x, 0, lm, L, vocab=GVOCAB, skip_ids=(G_UNK,), beam_width=W, n_best=N)
        c = beam_ctc_hotword_decode(x, 0, PHRASES, L, lm=lm, beam_width=W, n_best=N, **kw)
        for u, v in zip(b, c):
            assert torch.equal(u, v)


def test_hotwords_change_the_best_transcript(dev):
    vocab = ["_", "A", "B", "|"]
    x = np.log(np.array([[[0.05, 0.42, 0.5, 0.03]]], dtype=np.float64)).astype(np.float32)
    t0, c0, s0, _ = (u.cpu() for u in beam_ctc_decode(torch.from_numpy(x).to(dev), 0, beam_width=8, n_best=8,
                                                      token_min_logp=-INF, beam_prune_logp=-INF))
    assert t0[0, 0, :int(c0[0, 0])].tolist() == [2]
    tokens, counts, scores, am, _ = run(x, None, 0, ["A"], vocab, dev, hotword_weight=1.0, beam_width=8, n_best=8,
                                        token_min_logp=-INF, beam_prune_logp=-INF)
    assert tokens[0, 0, :int(counts[0, 0])].tolist() == [1]
    assert float(am[0, 0]) < float(s0[0, 0])
    ref, _ = HR.beam_search(x[0], 0, HR.Fusion(["A"], vocab, weight=1.0), 8, n_best=8, token_min_logp=-INF,
                            beam_prune_logp=-INF)
    assert ref[0][0] == (1,) and close32(float(scores[0, 0]), ref[0][1]) and close32(float(am[0, 0]), ref[0][2])


def test_bf16_logits_equal_their_fp32_cast_and_runs_are_bit_identical(dev, small_lm):
    _, lm, _ = small_lm
    g = torch.Generator().manual_seed(13)
    x16 = (torch.randn(4, 60, len(GVOCAB), generator=g) * 2).to(dev, torch.bfloat16)
    L = torch.tensor([60, 0, 31, 59], device=dev)
    kw = dict(vocab=GVOCAB, skip_ids=(G_UNK,), beam_width=32, n_best=4)
    for m in (None, lm):
        a = beam_ctc_hotword_decode(x16, 1, PHRASES, L, lm=m, **kw)
        b = beam_ctc_hotword_decode(x16.float(), 1, PHRASES, L, lm=m, **kw)
        for u, v in zip(a, b):
            assert torch.equal(u, v)
    x = (torch.randn(32, 249, len(GVOCAB), generator=g) * 2).to(dev)
    L = torch.randint(0, 250, (32,), generator=g).to(dev)
    for m in (None, lm):
        a = beam_ctc_hotword_decode(x, 0, PHRASES, L, lm=m, vocab=GVOCAB, skip_ids=(G_UNK,), beam_width=190, n_best=8)
        b = beam_ctc_hotword_decode(x, 0, PHRASES, L, lm=m, vocab=GVOCAB, skip_ids=(G_UNK,), beam_width=190, n_best=8)
        for u, v in zip(a, b):
            assert torch.equal(u, v)


def test_no_write_outside_outputs_and_workspace(dev, small_lm):
    _, lm, _ = small_lm
    g = torch.Generator().manual_seed(15)
    x = (torch.randn(5, 49, len(GVOCAB), generator=g) * 2).to(dev)
    L = torch.tensor([49, 0, 13, 48, 1], device=dev)
    with guarded_allocations() as guard:
        for W, N in ((1, 1), (100, 100), (256, 7)):
            for m in (None, lm):
                beam_ctc_hotword_decode(x, 3, PHRASES, L, lm=m, vocab=GVOCAB, skip_ids=(G_UNK,), beam_width=W, n_best=N)
        bad = guard.check()
    assert guard.allocs and not bad, bad


def test_conformer_logits_through_beam_decoder_with_hotwords(dev, tmp_path):
    """End to end: a small Conformer forward, then BeamCTCDecoder(hotwords=...) with and without an LM; at W = 1 with no
    pruning the text is the restatement's best hypothesis, and hotwords=None leaves the decoder's output unchanged."""
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
    hot = ["a", "b c", "c d", "ab"] + [vocab[i] for i in range(1, 15)]
    common = dict(blank_id=0, skip_ids=(16,), beam_width=1, beam_prune_logp=-INF, token_min_logp=-INF, max_candidates=16)
    for lm_path in (None, str(arpa)):
        lmkw = {} if lm_path is None else dict(lm=lm_path, alpha=0.5, beta=1.0)
        plain = BeamCTCDecoder(vocab, **common, **lmkw)
        assert plain(logits, out_len) == BeamCTCDecoder(vocab, **common, **lmkw, hotwords=None)(logits, out_len)
        assert plain(logits, out_len) == BeamCTCDecoder(vocab, **common, **lmkw, hotwords=[])(logits, out_len)
        dec = BeamCTCDecoder(vocab, **common, **lmkw, hotwords=hot, hotword_weight=3.0)
        texts = dec(logits, out_len)
        ref_lm = None if lm_path is None else LR.Arpa.read(lm_path)
        f = fusion(hot, vocab, 3.0, ref_lm, skip_ids=(16,), **({} if lm_path is None else dict(alpha=0.5, beta=1.0)))
        ref = HR.restate_batch(logits.float().cpu().numpy(), 0, f, out_len.cpu().numpy(), beam_width=1, max_candidates=16,
                               token_min_logp=-INF, beam_prune_logp=-INF)
        assert isinstance(texts, list) and len(texts) == 3
        for b, (hyps, margins) in enumerate(ref):
            assert R.min_margin(margins) >= MARGIN, margins
            assert texts[b] == dec.text(hyps[0][0])
