"""Streaming (resumable) CTC prefix beam search on the MI355X (conformer_amd.decode.beam_ctc_stream_*, BeamCTCDecoder.stream):
any split of the frames into chunks, fed through step and then finish, equals one-shot decoding of the consumed frames bit
for bit in every output, in all four modes (plain, LM, hotwords, LM + hotwords); the interim hypotheses of the plain search
are the one-shot search over the frames so far; the stream buffer and the outputs are written inside their bounds only."""
import numpy as np
import pytest
import torch

from conformer_amd.decode import (BeamCTCDecoder, beam_ctc_decode, beam_ctc_hotword_decode, beam_ctc_lm_decode,
                                  beam_ctc_stream_finish, beam_ctc_stream_init, beam_ctc_stream_step)
from conformer_amd.hotwords import Hotwords
from conformer_amd.lm import NgramLanguageModel, write_synthetic_arpa
from tests.test_write_guard_gpu import guarded_allocations

pytestmark = pytest.mark.gpu

TOKS = [chr(ord("A") + i) for i in range(10)] + ["TH", "É", "ßA"]
VOCAB = ["<pad>"] + TOKS + ["|", "<unk>"]
UNK = len(VOCAB) - 1
BLANK = 0
PHRASES = ["A", "B C", "A B", "ÉA", "THE", "C D E", "A B C D", "ßAB", "D", "É É", "CA B", "THÉ ßA"]
KN = dict(alpha=1.3, beta=2.5, unk_score_offset=-7.0, score_boundary=True, hotword_weight=4.0)
T = 41
MODES = ["plain", "lm", "hw", "lm_hw"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tables(dev, tmp_path_factory):
    """(lm, hotwords, lm device blob, hotword device blob): a 3-gram over 40 words spelled in TOKS, plus every hotword unigram"""
    p = tmp_path_factory.mktemp("lm") / "small.arpa"
    words = write_synthetic_arpa(p, TOKS, 40, [0, 200, 200], seed=9, max_tokens_per_word=2)
    uni = sorted({w for ph in PHRASES for w in ph.split()} - set(words))
    text = p.read_text(encoding="utf-8")
    n1 = int(text.split("ngram 1=")[1].split()[0])
    text = text.replace(f"ngram 1={n1}", f"ngram 1={n1 + len(uni)}", 1)
    text = text.replace("\\1-grams:\n", "\\1-grams:\n" + "".join(f"-2.5\t{w}\t-0.3\n" for w in uni), 1)
    p.write_text(text, encoding="utf-8")
    lm = NgramLanguageModel.from_arpa(p)
    hw = Hotwords(PHRASES)
    return lm, hw, lm.device_tables(VOCAB, "|", (UNK,), dev), hw.device_tables(VOCAB, "|", (UNK,), dev)


def logits(B, seed, dev, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, T, len(VOCAB), generator=g) * scale).to(dev)


def one_shot(mode, x, L, W, N, tables):
    lm, hw, _, _ = tables
    common = dict(beam_width=W, n_best=N, token_min_logp=-6.0, beam_prune_logp=-12.0, max_candidates=8)
    if mode == "plain":
        tk, ct, sc, nh = beam_ctc_decode(x, BLANK, L, **common)
        return [tk, ct, sc, nh]
    lmkw = dict(alpha=KN["alpha"], beta=KN["beta"], unk_score_offset=KN["unk_score_offset"], score_boundary=KN["score_boundary"])
    if mode == "lm":
        return list(beam_ctc_lm_decode(x, BLANK, lm, L, vocab=VOCAB, skip_ids=(UNK,), **lmkw, **common))
    return list(beam_ctc_hotword_decode(x, BLANK, hw, L, vocab=VOCAB, skip_ids=(UNK,), hotword_weight=KN["hotword_weight"],
                                        lm=lm if mode == "lm_hw" else None, **lmkw, **common))


def streamed(mode, x, L, chunks, W, N, tables, dev, interim=None):
    """feed x in `chunks` (per-chunk lengths cut from L), then finish; interim: list that receives every step's outputs"""
    _, _, lmt, hwt = tables
    st = beam_ctc_stream_init(x.shape[0], T, dev, beam_width=W, max_candidates=8,
                              lm_tables=lmt if mode in ("lm", "lm_hw") else None,
                              hw_tables=hwt if mode in ("hw", "lm_hw") else None, **KN)
    t0 = 0
    for c in chunks:
        cl = None if L is None else (L - t0).clamp(0, c)
        out = beam_ctc_stream_step(st, x[:, t0:t0 + c].contiguous(), BLANK, cl, n_best=N, token_min_logp=-6.0,
                                   beam_prune_logp=-12.0)
        if interim is not None:
            interim.append((t0 + c, [o for o in out if o is not None]))
        t0 += c
    assert t0 == T
    return [o for o in beam_ctc_stream_finish(st, n_best=N) if o is not None]


def chunkings(seed):
    rng = np.random.default_rng(seed)
    irregular = [7, 1, 20, 3, 10]
    assert sum(irregular) == T
    cuts = sorted(rng.choice(np.arange(1, T), size=5, replace=False).tolist())
    rand = [b - a for a, b in zip([0] + cuts, cuts + [T])]
    return {"ones": [1] * T, "whole": [T], "irregular": irregular, "random": rand}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W", [1, 16, 100, 256])
def test_chunked_equals_one_shot_bit_for_bit(dev, tables, mode, W):
    N = min(W, 7)
    x = logits(5, 100 + W, dev)
    # ragged utterances: one with no frames at all, and chunks where some utterances consume 0 frames
    L = torch.tensor([T, 0, 13, T - 1, 1], device=dev)
    want = one_shot(mode, x, L, W, N, tables)
    assert int(want[-1].min()) >= 1
    for name, ch in chunkings(W).items():
        for lens in (L, None):
            got = streamed(mode, x, lens, ch, W, N, tables, dev)
            ref = want if lens is not None else one_shot(mode, x, None, W, N, tables)
            assert len(got) == len(ref)
            for i, (g, r) in enumerate(zip(got, ref)):
                assert g.shape == r.shape and torch.equal(g, r), (mode, W, name, i)


@pytest.mark.parametrize("W", [1, 16, 100, 256])
def test_plain_interim_is_one_shot_over_frames_so_far(dev, tables, W):
    N = min(W, 5)
    x = logits(4, 200 + W, dev)
    L = torch.tensor([T, 9, 0, 30], device=dev)
    ch = chunkings(W + 1)["irregular"]
    interim = []
    streamed("plain", x, L, ch, W, N, tables, dev, interim)
    for end, out in interim:
        ref = beam_ctc_decode(x, BLANK, L.clamp(max=end), beam_width=W, n_best=N, token_min_logp=-6.0, beam_prune_logp=-12.0,
                              max_candidates=8)
        for i, (g, r) in enumerate(zip(out, ref)):
            assert torch.equal(g, r), (W, end, i)


@pytest.mark.parametrize("mode", ["lm", "hw", "lm_hw"])
@pytest.mark.parametrize("W", [1, 16, 100])
def test_finish_reranks_the_interim_set(dev, tables, mode, W):
    """With n_best = W: the interim hypotheses after the last chunk are the final ones as a set of token sequences; finish
    re-ranks them and changes their scores, it adds and removes none."""
    x = logits(3, 300 + W, dev)
    L = torch.tensor([T, 20, 5], device=dev)
    interim = []
    final = streamed(mode, x, L, [10, 1, 30], W, W, tables, dev, interim)
    tk_i, ct_i, _, _, nh_i = interim[-1][1]
    tk_f, ct_f, _, _, nh_f = final
    assert torch.equal(nh_i, nh_f)
    for b in range(3):
        seqs = lambda tk, ct: sorted(tuple(tk[b, r, :int(ct[b, r])].tolist()) for r in range(int(nh_f[b])))
        assert seqs(tk_i.cpu(), ct_i.cpu()) == seqs(tk_f.cpu(), ct_f.cpu())


@pytest.mark.parametrize("mode", MODES)
def test_decoder_stream_finish_equals_decoder_call(dev, tables, mode):
    lm, hw, _, _ = tables
    dec = BeamCTCDecoder(VOCAB, BLANK, skip_ids=(UNK,), beam_width=32, lm=lm if "lm" in mode else None,
                         hotwords=PHRASES if "hw" in mode else None, alpha=KN["alpha"], beta=KN["beta"],
                         unk_score_offset=KN["unk_score_offset"], hotword_weight=KN["hotword_weight"])
    x = logits(3, 400, dev, scale=4.0)
    s = dec.stream(3, T + 5)
    t0 = 0
    for c in [5, 17, 1, T - 23]:
        tk, ct, sc = s.step(x[:, t0:t0 + c])
        assert tk.is_cuda and tk.shape == (3, 1, T + 5) and ct.shape == (3, 1) and sc.shape == (3, 1)
        t0 += c
    partial = s.partial_text()
    want = dec(x)
    assert s.finish() == want and len(partial) == 3
    if mode == "plain":
        assert partial == want                       # no end-of-utterance step without LM and hotwords
    with pytest.raises(RuntimeError):
        s.step(x[:, :1])
    s.reset()
    s.step(x[:, :T // 2])
    assert s.finish() == dec(x[:, :T // 2])
    with pytest.raises(ValueError):
        dec.stream(3, T).step(x[:, :T].repeat(1, 2, 1))   # more frames than max_frames


def test_no_write_outside_stream_state_and_outputs(dev, tables):
    _, _, lmt, hwt = tables
    x = logits(5, 500, dev)
    L = torch.tensor([T, 0, 13, T - 1, 1], device=dev)
    with guarded_allocations() as guard:
        for W, N in ((1, 1), (100, 100), (256, 7)):
            for lm_t, hw_t in ((None, None), (lmt, None), (None, hwt), (lmt, hwt)):
                st = beam_ctc_stream_init(5, T, dev, beam_width=W, max_candidates=8, lm_tables=lm_t, hw_tables=hw_t, **KN)
                t0 = 0
                for c in [1, 15, T - 16]:
                    beam_ctc_stream_step(st, x[:, t0:t0 + c].contiguous(), BLANK, (L - t0).clamp(0, c), n_best=N)
                    t0 += c
                beam_ctc_stream_finish(st, n_best=N)
        bad = guard.check()
    assert guard.allocs and not bad, bad
