"""Committed-prefix streaming search on the MI355X (beam_ctc_stream_init(max_pending=...), BeamCTCStream, the transcribers)
against the float64 restatement of tests/ctc_beam_commit_restatement.py and, where nothing is forced, against one-shot decoding
bit for bit.

As in tests/test_ctc_beam_gpu.py the device keeps every score in fp64, so a decision can only differ from the restatement's
where the restatement reports a margin below that error: every comparison requires the margins of the restatement's own
(forced) trajectory to be >= MARGIN, so a near-tie fails loudly.  After every compared step the survivors are read with a
finish at n_best = W, which saves no state: the whole live set is compared, not only the best."""
import numpy as np
import pytest
import torch

from conformer_amd import _lib
from conformer_amd.decode import (BeamCTCDecoder, BeamCTCStream, beam_ctc_decode, beam_ctc_hotword_decode, beam_ctc_lm_decode,
                                  beam_ctc_stream_finish, beam_ctc_stream_init, beam_ctc_stream_step)
from conformer_amd.hotwords import Hotwords
from conformer_amd.lm import NgramLanguageModel, write_synthetic_arpa
from tests import ctc_beam_commit_restatement as CR
from tests import ctc_beam_restatement as R
from tests.test_ctc_beam_gpu import MARGIN, SCORE_TOL
from tests.test_write_guard_gpu import guarded_allocations

pytestmark = pytest.mark.gpu

CHUNKS = [1, 7, 3, 16, 2, 11, 5, 15]
K_CAP = 16
T, V, K, W = 60, 7, 4, 8
BLANK = 0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def random_logits(seed, B=3, T=T, V=V):
    """utterance 0: 3 * default_rng(seed).normal((T, V)); the other utterances: further draws of the same generator"""
    rng = np.random.default_rng(seed)
    return np.stack([(3 * rng.normal(size=(T, V))).astype(np.float32) for _ in range(B)])


def peaky_logits(seed, B=3, T=T, V=V):
    """5 * onehot of a random path with runs of 1-3 frames, plus N(0, 1)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, T, V)).astype(np.float32)
    for b in range(B):
        t = 0
        while t < T:
            run, c = int(rng.integers(1, 4)), int(rng.integers(0, V))
            x[b, t:t + run, c] += 5.0
            t += run
    return x


def ragged_steps(B, T, chunks, seed):
    """[(begin, end, lengths (B))]: utterance 0 takes every frame, the others a prefix of each chunk (sometimes none)"""
    rng = np.random.default_rng(100 + seed)
    out = []
    for a, b in CR.chunk_ends(T, chunks):
        L = rng.integers(0, b - a + 1, size=B)
        L[0] = b - a
        if B > 2 and len(out) % 3 == 1:
            L[2] = 0
        out.append((a, b, L))
    return out


def read_new(st, prev_total):
    """the tokens committed since prev_total (per utterance, <= L of them) and the new totals"""
    total = st.total.cpu().tolist()
    log, L = st.log.cpu(), st.log.shape[1]
    return [log[b, torch.arange(prev_total[b], total[b]) % L].tolist() for b in range(st.B)], total


def check_against_restatement(x, steps, M, k_cap, W, K, dev, every=1, commit_log=1, n_final=1):
    """x (B, T, V) float32; steps from ragged_steps.  Device and restatement side by side; every `every`-th step and at the
    end: total, the log, the tokens this step committed, the step's own best, nh and every survivor (tokens, score)."""
    B = x.shape[0]
    xt = torch.from_numpy(x).to(dev)
    st = beam_ctc_stream_init(B, None, dev, beam_width=W, max_candidates=K, max_pending=M, max_chunk_frames=k_cap,
                              commit_log=commit_log)
    assert st.buf.numel() == _lib.load().cfm_ctc_beam_commit_state_bytes(B, M, k_cap, W, K, 0, 0) and st.t_max == M + k_cap
    ref = [CR.CommitSearch(BLANK, W, K, max_pending=M) for _ in range(B)]
    C_dev, total = [[] for _ in range(B)], [0] * B
    for i, (a, b, L) in enumerate(steps):
        tk, ct, sc, _, nh = beam_ctc_stream_step(st, xt[:, a:b].contiguous(), BLANK, torch.from_numpy(L).to(dev), n_best=W)
        before = [len(r.C) for r in ref]
        for u in range(B):
            if L[u]:
                ref[u].step(x[u, a:a + L[u]])
        if (i + 1) % every and i + 1 < len(steps):
            continue
        new, total = read_new(st, total)
        fin = beam_ctc_stream_finish(st, n_best=W)
        ftk, fct, fsc, fnh = fin[0].cpu(), fin[1].cpu(), fin[2].cpu(), fin[4].cpu()
        tk, ct, nc = tk.cpu(), ct.cpu(), st.committed.cpu().tolist()
        assert tk.shape == (B, W, M + k_cap) and ftk.shape == (B, W, M + k_cap)
        for u in range(B):
            C_dev[u] += new[u]
            C = list(ref[u].C)
            assert total[u] == len(C) and C_dev[u] == C, (i, u, total[u], len(C))
            surv = ref[u].survivors()
            assert int(fnh[u]) == len(surv), (i, u, int(fnh[u]), len(surv))
            for r, (seq, s) in enumerate(surv):
                n = int(fct[u, r])
                assert tuple(ftk[u, r, :n].tolist()) == seq, (i, u, r)
                assert bool((ftk[u, r, n:] == -1).all())
                assert abs(float(fsc[u, r]) - s) <= SCORE_TOL, (i, u, r, float(fsc[u, r]), s)
            if L[u]:
                assert nc[u] == ref[u].last_commit == len(C) - before[u], (i, u)
                # the step's own best is relative to C before the step: the new tokens, then the pending best
                assert tk[u, 0, :int(ct[u, 0])].tolist() == C[before[u]:] + list(surv[0][0]), (i, u)
            else:
                assert nc[u] == 0
    ftk, fct, fsc = (t.cpu() for t in beam_ctc_stream_finish(st, n_best=n_final)[:3])
    finals = []
    for u in range(B):
        hyps = ref[u].finish(n_final)
        assert min(ref[u].margins.values()) >= MARGIN, (u, ref[u].margins)
        for r, (seq, s) in enumerate(hyps):
            assert tuple(C_dev[u]) + tuple(ftk[u, r, :int(fct[u, r])].tolist()) == seq, (u, r)
            assert abs(float(fsc[u, r]) - s) <= SCORE_TOL, (u, r, float(fsc[u, r]), s)
        finals.append(hyps)
    return ref, finals


# ---- 1. forced commits ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forced_figures():
    """From the restatement alone, on utterance 0 (every frame): each (seed, M) forces and drops enough to prove something, and
    forcing changes the result of at least one of them."""
    differs = 0
    for seed in range(4):
        x = random_logits(seed)[0]
        one, _ = R.beam_search(x, BLANK, W, max_candidates=K)
        for M in (1, 2, 4, 8):
            final, cs, _ = CR.commit_search(x, CHUNKS, BLANK, M, beam_width=W, max_candidates=K)
            assert cs.forced >= 3 and cs.dropped >= 10, (seed, M, cs.forced, cs.dropped)
            differs += final[0][0] != one[0][0]
    assert differs >= 1
    return differs


@pytest.mark.parametrize("M", [1, 2, 4, 8])
@pytest.mark.parametrize("seed", range(4))
def test_forced_commits_equal_the_restatement(dev, forced_figures, seed, M):
    x = random_logits(seed)
    # commit_log=1: the ring is the smallest allowed, M + k_cap tokens, and wraps within the run
    check_against_restatement(x, ragged_steps(3, T, CHUNKS, seed), M, K_CAP, W, K, dev, commit_log=1)


# ---- 2. no forcing: one-shot bit for bit, all four modes -------------------------------------------------------------------------
TOKS = ["A", "B", "C", "D"]
VOCAB = ["<pad>"] + TOKS + ["|", "<unk>"]
UNK = len(VOCAB) - 1
PHRASES = ["A", "B C", "A B", "D", "C D A", "BA"]
KN = dict(alpha=1.3, beta=2.5, unk_score_offset=-7.0, score_boundary=True, hotword_weight=4.0)
MODES = ["plain", "lm", "hw", "lm_hw"]


@pytest.fixture(scope="module")
def tables(dev, tmp_path_factory):
    """(lm, hotwords, lm device blob, hotword device blob) as tests/test_ctc_beam_stream_gpu.py builds them, over 7 tokens"""
    p = tmp_path_factory.mktemp("lm") / "small.arpa"
    words = write_synthetic_arpa(p, TOKS, 20, [0, 60, 60], seed=9, max_tokens_per_word=2)
    uni = sorted({w for ph in PHRASES for w in ph.split()} - set(words))
    text = p.read_text(encoding="utf-8")
    n1 = int(text.split("ngram 1=")[1].split()[0])
    text = text.replace(f"ngram 1={n1}", f"ngram 1={n1 + len(uni)}", 1)
    text = text.replace("\\1-grams:\n", "\\1-grams:\n" + "".join(f"-2.5\t{w}\t-0.3\n" for w in uni), 1)
    p.write_text(text, encoding="utf-8")
    lm = NgramLanguageModel.from_arpa(p)
    hw = Hotwords(PHRASES)
    return lm, hw, lm.device_tables(VOCAB, "|", (UNK,), dev), hw.device_tables(VOCAB, "|", (UNK,), dev)


def one_shot(mode, x, L, N, tables):
    lm, hw, _, _ = tables
    common = dict(beam_width=W, n_best=N, max_candidates=K)
    if mode == "plain":
        return list(beam_ctc_decode(x, BLANK, L, **common))
    lmkw = dict(alpha=KN["alpha"], beta=KN["beta"], unk_score_offset=KN["unk_score_offset"], score_boundary=KN["score_boundary"])
    if mode == "lm":
        return list(beam_ctc_lm_decode(x, BLANK, lm, L, vocab=VOCAB, skip_ids=(UNK,), **lmkw, **common))
    return list(beam_ctc_hotword_decode(x, BLANK, hw, L, vocab=VOCAB, skip_ids=(UNK,), hotword_weight=KN["hotword_weight"],
                                        lm=lm if mode == "lm_hw" else None, **lmkw, **common))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("inputs", ["seed0", "seed1", "seed2", "seed3", "peaky"])
def test_without_forcing_equals_one_shot_bit_for_bit(dev, tables, mode, inputs):
    M, N, B = 64, 4, 3
    x = peaky_logits(7) if inputs == "peaky" else random_logits(int(inputs[-1]))
    steps = ragged_steps(B, T, CHUNKS, 5)
    # the frames each utterance consumed, concatenated: what one-shot decoding sees
    cat, Lc = np.zeros_like(x), np.zeros(B, dtype=np.int64)
    for a, b, L in steps:
        for u in range(B):
            cat[u, Lc[u]:Lc[u] + L[u]] = x[u, a:a + L[u]]
            Lc[u] += L[u]
    want = one_shot(mode, torch.from_numpy(cat).to(dev), torch.from_numpy(Lc).to(dev), N, tables)
    _, _, lmt, hwt = tables
    st = beam_ctc_stream_init(B, None, dev, beam_width=W, max_candidates=K, lm_tables=lmt if "lm" in mode else None,
                              hw_tables=hwt if "hw" in mode else None, max_pending=M, max_chunk_frames=K_CAP, **KN)
    xt = torch.from_numpy(x).to(dev)
    for a, b, L in steps:
        beam_ctc_stream_step(st, xt[:, a:b].contiguous(), BLANK, torch.from_numpy(L).to(dev), n_best=N)
    C, total = read_new(st, [0] * B)
    assert total[0] > 0, "nothing was committed before the finish: the case proves nothing"
    got = [o for o in beam_ctc_stream_finish(st, n_best=N) if o is not None]
    tk, ct = got[0], got[1]
    full = torch.full((B, N, T), -1, dtype=torch.int64, device=dev)
    for u in range(B):
        for r in range(int(got[-1][u])):
            n = int(ct[u, r])
            full[u, r, :total[u] + n] = torch.cat([torch.tensor(C[u], dtype=torch.int64, device=dev), tk[u, r, :n]])
            ct[u, r] += total[u]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip([full] + got[1:], want)):
        assert g.shape == w.shape and torch.equal(g, w), (mode, inputs, i)


# ---- 3. the tree is reused: a stream 100 times the tree ------------------------------------------------------------------------
def test_tree_reuse_over_a_long_stream(dev):
    Tl, M, B = 2000, 4, 2
    x = random_logits(11, B=B, T=Tl)
    steps = [(a, b, np.full(B, b - a)) for a, b in CR.chunk_ends(Tl, list(range(1, 17)))]
    assert Tl == 100 * (M + K_CAP)
    ref, finals = check_against_restatement(x, steps, M, K_CAP, W, K, dev, every=50, commit_log=4096)
    # SCORE_TOL holds here too: the scores stay below 1024 in magnitude, where half an fp32 ulp is 3.1e-5
    assert all(abs(h[0][1]) < 1024 for h in finals)
    assert all(r.forced >= 50 for r in ref)


# ---- 4. full width -------------------------------------------------------------------------------------------------------------
def test_full_width_scan_and_compaction(dev):
    x = random_logits(21, B=1, T=120, V=40)
    steps = [(a, b, np.full(1, b - a)) for a, b in CR.chunk_ends(120, CHUNKS)]
    ref, _ = check_against_restatement(x, steps, 6, K_CAP, 100, 16, dev)
    assert ref[0].forced >= 3 and ref[0].dropped >= 100


def test_no_write_outside_state_log_and_outputs(dev):
    x = torch.from_numpy(random_logits(31, B=3)).to(dev)
    with guarded_allocations() as guard:
        for Wg, M in ((1, 1), (8, 2), (100, 6), (256, 64)):
            st = beam_ctc_stream_init(3, None, dev, beam_width=Wg, max_candidates=K, max_pending=M, max_chunk_frames=K_CAP,
                                      commit_log=1)
            for a, b, L in ragged_steps(3, T, CHUNKS, 2):
                beam_ctc_stream_step(st, x[:, a:b].contiguous(), BLANK, torch.from_numpy(L).to(dev), n_best=min(Wg, 3))
            beam_ctc_stream_finish(st, n_best=1)
        bad = guard.check()
    assert guard.allocs and not bad, bad


# ---- 5. slots ------------------------------------------------------------------------------------------------------------------
SLOT_VOCAB = ["<pad>"] + [chr(ord("a") + i) for i in range(14)] + ["|", "<unk>"]


def tiny_model(seed, dev):
    from model.conformer import Conformer
    from oracle import conformer_oracle as O
    P = O.make_params(vocab=len(SLOT_VOCAB), n_mel=80, n_blocks=2, d=32, n_heads=4, ksize=31, lstm_hidden=24, seed=seed)
    m = Conformer(len(SLOT_VOCAB), 80, 2, 32, 4, 31, 24, 1, 0.0)
    m.load_state_dict(P, strict=True)
    return m.to(dev).eval()


def test_slots_commit_per_slot_and_outlive_max_mel_frames(dev):
    from conformer_amd.slots import SlotTranscriber
    m = tiny_model(71, dev)
    dec = BeamCTCDecoder(SLOT_VOCAB, 0, skip_ids=(16,), beam_width=16)
    kw = dict(left_context=8, max_chunk_mel_frames=64)
    S, M = 3, 4
    tr = SlotTranscriber(m, dec, S, None, max_pending=M, **kw)
    k_cap = tr.commit[1]
    assert isinstance(tr.beam, BeamCTCStream) and tr.beam.state.buf.numel() == _lib.load().cfm_ctc_beam_commit_state_bytes(S, M, k_cap, 16, 16, 0, 0)
    # every step: closes, then opens, then mel frames per slot; slot 1 is closed and reopened mid-run
    schedule = [dict(open=[0, 1], frames={0: 64, 1: 5}), dict(frames={0: 33, 1: 3}), dict(open=[2], frames={0: 64, 1: 60, 2: 6}),
                dict(frames={0: 1, 1: 64, 2: 64}), dict(close=[1], open=[1], frames={0: 64, 1: 64, 2: 0}),
                dict(frames={0: 64, 1: 7, 2: 50}), dict(frames={0: 64, 1: 64}), dict(close=[2], frames={0: 40, 1: 64})]
    g = torch.Generator().manual_seed(5)
    fed, texts, mel_seen = {s: [] for s in range(S)}, [], [0] * S
    for stp in schedule:
        for s in stp.get("close", []):
            texts.append((tr.close(s), fed[s]))
            fed[s] = []
        for s in stp.get("open", []):
            others = [o for o in range(S) if o != s]
            before = (tr.beam.state.total.cpu()[others].clone(), tr.beam.state.log.cpu()[others].clone())
            tr.open(s)
            assert int(tr.beam.state.total[s]) == 0 and tr.beam.popped[s] == 0
            assert torch.equal(tr.beam.state.total.cpu()[others], before[0])
            assert torch.equal(tr.beam.state.log.cpu()[others], before[1])
            mel_seen[s] = 0
        fr = [stp["frames"].get(s, 0) for s in range(S)]
        logits, k = tr.step(torch.randn(S, 80, max(fr), generator=g).mul(3.0).to(dev), fr)
        for s in range(S):
            mel_seen[s] += fr[s]
            if k[s]:
                fed[s].append(logits[s:s + 1, :k[s]].clone())
        assert set(tr.partial_text()) == {s for s in range(S) if tr.is_open[s]}
    for s in range(S):
        if tr.is_open[s]:
            texts.append((tr.close(s), fed[s]))
    assert len(texts) == 4 and int(tr.beam.state.total.sum()) == 0          # every closed slot's total is reset
    committed_any = False
    for text, chunks in texts:
        ref = dec.stream(1, None, dev, max_pending=M, max_chunk_frames=k_cap)
        for c in chunks:
            ref.step(c)
        committed_any |= int(ref.state.total[0]) > 0
        assert ref.finish() == [text]
    assert committed_any
    # the same object without max_pending ends with max_mel_frames; slot 0 above went past it
    short = SlotTranscriber(m, dec, S, 200, **kw)
    short.open(0)
    for _ in range(3):
        short.step(torch.randn(S, 80, 64, generator=g).to(dev), [64, 0, 0])
    with pytest.raises(RuntimeError, match="max_mel_frames"):
        short.step(torch.randn(S, 80, 64, generator=g).to(dev), [64, 0, 0])
    assert mel_seen[0] > 200 + 64


# the slot semantics at the search level: (chunk frames, frames each of the 3 utterances takes); after step 4 utterance 2 ends
# and its row is given to a new utterance, which takes nothing in its first step
SLOT_STEPS = [(5, [5, 3, 0]), (3, [3, 0, 3]), (7, [7, 7, 4]), (4, [0, 4, 4]), (6, [6, 2, 0]), (7, [5, 0, 7]), (3, [3, 3, 3]),
              (5, [5, 5, 1])]


@pytest.mark.parametrize("commit", [False, True], ids=["max_frames", "max_pending"])
def test_stream_rows_are_independent_utterances(dev, commit):
    """One BeamCTCStream over B = 3 rows against one-utterance streams fed the same frames: the step's tokens and counts
    (torch.equal), every partial_text and every final text, through finish(only=[2]) + reset_slots([2]) and a second
    utterance in row 2.  V = 4 (blank, two letters, the delimiter: the fewest tokens with which decoder.text still joins and
    splits words); the frames of a chunk past an utterance's length hold noise."""
    Vs, total = 4, sum(tc for tc, _ in SLOT_STEPS)
    dec = BeamCTCDecoder(["<pad>", "A", "B", "|"], BLANK, beam_width=4, max_candidates=4)
    x = torch.from_numpy(peaky_logits(17, B=4, T=total, V=Vs)).to(dev)        # utterances 0..2, and 3: the second one of row 2
    noise = torch.randn(3, 8, Vs, generator=torch.Generator().manual_seed(3)).mul(3.0).to(dev)

    def stream(B):
        return dec.stream(B, None, dev, max_pending=4, max_chunk_frames=8) if commit else dec.stream(B, total, dev)

    s, refs = stream(3), [stream(1) for _ in range(3)]
    utt, pos, finals = [0, 1, 2], [0] * 4, {}
    for i, (tc, L) in enumerate(SLOT_STEPS):
        if i == 4:
            finals[2] = (s.finish(only=[2]), refs[2].finish())
            assert finals[2][0] == ["", "", finals[2][1][0]] and not s.finished
            s.reset_slots([2])
            utt[2], refs[2] = 3, stream(1)
            assert s.partial_text()[2] == "" and s.popped[2] == 0
            assert s.partial_text(only=[0, 1])[:2] == [r.partial_text()[0] for r in refs[:2]]
        chunk = noise[:, :tc].clone()
        for b in range(3):
            chunk[b, :L[b]] = x[utt[b], pos[utt[b]]:pos[utt[b]] + L[b]]
            pos[utt[b]] += L[b]
        tk, ct, _ = s.step(chunk, torch.tensor(L))
        for b in range(3):
            if L[b]:
                rtk, rct, _ = refs[b].step(chunk[b:b + 1, :L[b]].contiguous())
                assert torch.equal(tk[b:b + 1], rtk) and torch.equal(ct[b:b + 1], rct), (i, b)
        assert s.partial_text() == [r.partial_text()[0] for r in refs], i
    assert pos == [34, 24, 11, 11]
    want = [r.finish()[0] for r in refs]
    assert s.finish() == want and s.finished
    # the references alone say that the case is not vacuous: no empty text, and row 0 committed on the way
    assert all(want) and finals[2][1][0] and (not commit or int(refs[0].state.total[0]) > 0)


# ---- 6. pop_committed ----------------------------------------------------------------------------------------------------------
def test_pop_committed_pieces_rejoin(dev):
    dec = BeamCTCDecoder(VOCAB, BLANK, skip_ids=(UNK,), beam_width=W, max_candidates=K)
    x = torch.from_numpy(peaky_logits(3, B=2, T=120)).to(dev)
    ends = CR.chunk_ends(120, CHUNKS)

    def run(pop_every, **kw):
        s = dec.stream(2, None, dev, max_pending=4, max_chunk_frames=K_CAP, **kw)
        pieces = [[], []]
        for i, (a, b) in enumerate(ends):
            s.step(x[:, a:b])
            if pop_every and (i + 1) % pop_every == 0:
                for u, ids in enumerate(s.pop_committed()):
                    pieces[u] += ids
        return s, pieces

    whole, _ = run(0)
    all_ids = whole.pop_committed()
    final = beam_ctc_stream_finish(whole.state)
    tail = [final[0][u, 0, :int(final[1][u, 0])].tolist() for u in range(2)]
    assert min(len(i) for i in all_ids) > 4 + K_CAP                # more than the smallest ring holds
    for every in (1, 3):
        s2, pieces = run(every)
        rest = s2.committed_text()
        left = s2.pop_committed()
        assert [pieces[u] + left[u] for u in range(2)] == all_ids
        assert rest == [dec.text(i) for i in left]
        assert s2.finish() == [dec.text(t) for t in tail]          # everything committed was popped: only the final tokens
    s, _ = run(0)
    assert s.partial_text() == s.finish() == [dec.text(all_ids[u] + tail[u]) for u in range(2)]
    small, _ = run(0, commit_log=1)                                # the ring holds M + k_cap = 20 tokens
    with pytest.raises(RuntimeError, match="commit log"):
        small.pop_committed()
    with pytest.raises(RuntimeError, match="without max_pending"):
        dec.stream(2, 120, dev).pop_committed()


# ---- 7. StreamingTranscriber ---------------------------------------------------------------------------------------------------
def test_streaming_transcriber_with_a_huge_max_pending_is_the_existing_one(dev):
    from conformer_amd.transcribe import StreamingTranscriber
    m = tiny_model(91, dev)
    dec = BeamCTCDecoder(SLOT_VOCAB, 0, skip_ids=(16,), beam_width=8)
    chunks = [64, 64, 7, 1, 64, 50, 64]
    x = torch.randn(2, 80, sum(chunks), generator=torch.Generator().manual_seed(4)).mul(3.0).to(dev)
    kw = dict(left_context=8, max_chunk_mel_frames=64)
    ref, tr = StreamingTranscriber(m, dec, 2, sum(chunks), **kw), StreamingTranscriber(m, dec, 2, None, max_pending=10 ** 6, **kw)
    t0 = 0
    for c in chunks:
        a, b = ref.step(x[:, :, t0:t0 + c]), tr.step(x[:, :, t0:t0 + c])
        assert torch.equal(a, b)
        t0 += c
    assert tr.partial_text() == ref.partial_text()
    assert tr.finish() == ref.finish()
