"""Token and word timestamps from the CTC beam search on the MI355X (return_times=, beam_ctc_stream_init(times=True),
BeamCTCStream / SlotTranscriber(times=True)) against the two float64 statements of tests/ctc_beam_times_restatement.py.

Frames are integers and compared exactly.  A log-probability is the search's fp64 value (it agrees with the restatement's to
~1e-12) rounded to fp32, so it must lie within one fp32 ulp of the float64 value.  As in tests/test_ctc_beam_gpu.py a decision
can only differ from the restatement's where the restatement reports a margin below the fp64 error: every compared case requires
the restatement's own margins to be >= MARGIN (the seeds were chosen on the CPU so that they are)."""
import math

import numpy as np
import pytest
import torch

from conformer_amd.decode import (BeamCTCDecoder, beam_ctc_decode, beam_ctc_hotword_decode, beam_ctc_lm_decode,
                                  beam_ctc_stream_committed, beam_ctc_stream_finish, beam_ctc_stream_init, beam_ctc_stream_step)
from conformer_amd.hotwords import Hotwords
from conformer_amd.lm import NgramLanguageModel, write_synthetic_arpa
from tests import ctc_beam_commit_restatement as CR
from tests import ctc_beam_hotword_restatement as HR
from tests import ctc_beam_lm_restatement as LR
from tests import ctc_beam_restatement as R
from tests import ctc_beam_times_restatement as TR
from tests.test_ctc_beam_gpu import MARGIN

pytestmark = pytest.mark.gpu
INF = math.inf

BLANK, V, T, B, N, W, K = 0, 7, 20, 3, 3, 6, 4
LENGTHS = np.array([T, 0, 13])
CHUNKS = (1, 5, 3)
TOKS = ["A", "B", "C", "D"]
VOCAB = ["<pad>"] + TOKS + ["|", "<unk>"]
UNK = len(VOCAB) - 1
PHRASES = ["A", "B C", "A B", "D", "C D A", "BA"]
KN = dict(alpha=1.3, beta=2.5, unk_score_offset=-7.0, score_boundary=True, hotword_weight=4.0)
LMKW = {k: KN[k] for k in ("alpha", "beta", "unk_score_offset", "score_boundary")}
MODES = ["plain", "lm", "hw", "lm_hw"]
SEED = {"plain": 2, "lm": 4, "hw": 2, "lm_hw": 0}          # each has a natural re-entry too (checked by test 1)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def random_logits(seed, B=B, T=T, V=V):
    rng = np.random.default_rng(seed)
    return np.stack([(3 * rng.normal(size=(T, V))).astype(np.float32) for _ in range(B)])


def write_arpa(path):
    """the model of tests/test_ctc_beam_commit_gpu.py over the 7 tokens: a synthetic 3-gram plus every hotword unigram"""
    words = write_synthetic_arpa(path, TOKS, 20, [0, 60, 60], seed=9, max_tokens_per_word=2)
    uni = sorted({w for ph in PHRASES for w in ph.split()} - set(words))
    text = path.read_text(encoding="utf-8")
    n1 = int(text.split("ngram 1=")[1].split()[0])
    text = text.replace(f"ngram 1={n1}", f"ngram 1={n1 + len(uni)}", 1)
    text = text.replace("\\1-grams:\n", "\\1-grams:\n" + "".join(f"-2.5\t{w}\t-0.3\n" for w in uni), 1)
    path.write_text(text, encoding="utf-8")
    return path


@pytest.fixture(scope="module")
def arpa(tmp_path_factory):
    return write_arpa(tmp_path_factory.mktemp("lm") / "small.arpa")


def ref_search(mode, arpa_path, W=W, K=K):
    """the existing restatement of `mode` with everything bound but (logits, length=, n_best=)"""
    kw = dict(beam_width=W, max_candidates=K)
    if mode == "plain":
        return lambda lg, **k: R.beam_search(lg, BLANK, **kw, **k)
    lm = LR.Fusion(LR.Arpa.read(str(arpa_path)), VOCAB, skip_ids=(UNK,), **LMKW)
    if mode == "lm":
        return lambda lg, **k: LR.beam_search(lg, BLANK, lm, **kw, **k)
    f = HR.Fusion(PHRASES, VOCAB, skip_ids=(UNK,), weight=KN["hotword_weight"], lm=lm if mode == "lm_hw" else None)
    return lambda lg, **k: HR.beam_search(lg, BLANK, f, **kw, **k)


def reference(mode, arpa_path, x, lengths, n_best=N, W=W, K=K):
    """Statement 1 per utterance: [(hypotheses, their value tuples, the live sets)]; the margins of the full search are checked."""
    search = ref_search(mode, arpa_path, W, K)
    out = []
    for b in range(x.shape[0]):
        n = int(lengths[b])
        hyps, margins = search(x[b], length=n, n_best=n_best)
        assert R.min_margin(margins) >= MARGIN, (mode, b, margins)
        sets = TR.live_sets(search, x[b], n, W)
        vals = TR.times_from_live_sets(sets, R.log_softmax64(x[b]))
        out.append((hyps, [vals[-1][tuple(h[0])] if n else () for h in hyps], sets))
    return out


def device_objects(mode, arpa_path, dev):
    lm = NgramLanguageModel.from_arpa(arpa_path) if "lm" in mode else None
    hw = Hotwords(PHRASES) if "hw" in mode else None
    return lm, hw


def one_shot(mode, objs, x, L, n_best=N, W=W, K=K, **kw):
    lm, hw = objs
    common = dict(beam_width=W, n_best=n_best, max_candidates=K, **kw)
    if mode == "plain":
        return list(beam_ctc_decode(x, BLANK, L, **common))
    if mode == "lm":
        return list(beam_ctc_lm_decode(x, BLANK, lm, L, vocab=VOCAB, skip_ids=(UNK,), **LMKW, **common))
    return list(beam_ctc_hotword_decode(x, BLANK, hw, L, vocab=VOCAB, skip_ids=(UNK,), hotword_weight=KN["hotword_weight"], lm=lm,
                                        **LMKW, **common))


def stream_state(mode, objs, dev, B=B, max_frames=T, W=W, K=K, **kw):
    lm, hw = objs
    lmt = None if lm is None else lm.device_tables(VOCAB, "|", (UNK,), dev)
    hwt = None if hw is None else hw.device_tables(VOCAB, "|", (UNK,), dev)
    return beam_ctc_stream_init(B, max_frames, dev, beam_width=W, max_candidates=K, lm_tables=lmt, hw_tables=hwt, **KN, **kw)


def ulp_close(got: float, want: float) -> bool:
    """within one fp32 ulp of the float64 value"""
    return abs(got - want) <= float(np.spacing(np.float32(abs(want))))


def check_invariants(tokens, counts, tf, tl, consumed, token_min_logp=-5.0):
    """on every output: frames strictly increasing inside [0, consumed), frame[i] >= i, logp >= token_min_logp, padding -1 / -inf"""
    tokens, counts, tf, tl = tokens.cpu(), counts.cpu(), tf.cpu(), tl.cpu()
    assert tf.dtype == torch.int64 and tl.dtype == torch.float32 and tf.shape == tokens.shape == tl.shape
    for b in range(tokens.shape[0]):
        for r in range(tokens.shape[1]):
            n = int(counts[b, r])
            fr, lp = tf[b, r, :n].tolist(), tl[b, r, :n].tolist()
            assert all(a < c for a, c in zip(fr, fr[1:])) and all(i <= f < int(consumed[b]) for i, f in enumerate(fr)), (b, r, fr)
            assert all(p >= token_min_logp for p in lp), (b, r, lp)
            assert bool((tf[b, r, n:] == -1).all()) and bool((tl[b, r, n:] == -INF).all()) and bool((tokens[b, r, n:] == -1).all())


def check_values(ref, tokens, counts, tf, tl, offset=None):
    """device rows against statement 1: tokens and frames exactly, logp within one ulp.  offset[b]: tokens of the reference's
    absolute sequences the device rows do not repeat (commit mode)."""
    tokens, counts, tf, tl = tokens.cpu(), counts.cpu(), tf.cpu(), tl.cpu()
    for b, (hyps, vals, _) in enumerate(ref):
        o = 0 if offset is None else offset[b]
        for r, (h, v) in enumerate(zip(hyps, vals)):
            n = int(counts[b, r])
            assert tuple(tokens[b, r, :n].tolist()) == tuple(h[0])[o:], (b, r)
            assert tf[b, r, :n].tolist() == [f for f, _ in v[o:]], (b, r, tf[b, r, :n].tolist(), v)
            assert all(ulp_close(g, p) for g, (_, p) in zip(tl[b, r, :n].tolist(), v[o:])), (b, r)
        for r in range(len(hyps), tokens.shape[1]):
            assert int(counts[b, r]) == 0


def chunked(st, xt, lengths, chunks, dev, n_best=N):
    """step the frames each utterance consumes, chunk by chunk; per step the outputs and the (B) frames consumed so far"""
    outs, used = [], np.zeros(len(lengths), dtype=np.int64)
    for a, b in CR.chunk_ends(xt.shape[1], chunks):
        L = np.clip(lengths - a, 0, b - a)
        used = used + L
        outs.append((beam_ctc_stream_step(st, xt[:, a:b].contiguous(), BLANK, torch.from_numpy(L).to(dev), n_best=n_best),
                     L, used.copy()))
    return outs


# ---- 1. exact agreement, all four modes, one-shot and chunked ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_times_equal_the_restatement_one_shot_and_chunked(dev, arpa, mode):
    x = random_logits(SEED[mode])
    ref = reference(mode, arpa, x, LENGTHS)
    assert sum(len(h[0]) for h in ref[0][0]) >= 6                          # the case has tokens to time
    assert TR.reentries(ref[0][2]), "no prefix was pruned and found again in this case"
    objs = device_objects(mode, arpa, dev)
    xt, Lt = torch.from_numpy(x).to(dev), torch.from_numpy(LENGTHS).to(dev)
    plain = one_shot(mode, objs, xt, Lt)
    timed = one_shot(mode, objs, xt, Lt, return_times=True)
    assert len(timed) == len(plain) + 1
    for i, (g, w) in enumerate(zip(timed[:-1], plain)):                    # every other output is the plain entries', bit for bit
        assert torch.equal(g, w), (mode, i)
    tf, tl = timed[-1]
    check_invariants(timed[0], timed[1], tf, tl, LENGTHS)
    check_values(ref, timed[0], timed[1], tf, tl)
    # chunked (1, 5, 3): the finish equals one-shot bit for bit, values included; every step's interim rows keep the invariants
    st = stream_state(mode, objs, dev, times=True)
    st0 = stream_state(mode, objs, dev)
    steps = chunked(st, xt, LENGTHS, CHUNKS, dev)
    steps0 = chunked(st0, xt, LENGTHS, CHUNKS, dev)
    for (out, L, used), (out0, _, _) in zip(steps, steps0):
        assert len(out) == 6 and len(out0) == 5
        for i, (g, w) in enumerate(zip(out[:5], out0)):
            assert (g is None and w is None) or torch.equal(g, w), (mode, i)
        check_invariants(out[0], out[1], out[5][0], out[5][1], used)
        if mode == "plain":                                                # the interim ranking is the search's own: compare it too
            check_values(reference(mode, arpa, x, used), out[0], out[1], out[5][0], out[5][1])
    fin = beam_ctc_stream_finish(st, n_best=N)
    for i, (g, w) in enumerate(zip([o for o in fin[:5] if o is not None], plain)):
        assert torch.equal(g, w), (mode, i)
    assert torch.equal(fin[5][0], tf) and torch.equal(fin[5][1], tl)


# ---- 2. a prefix that is pruned and found again ---------------------------------------------------------------------------------
def test_a_re_entered_prefix_gets_the_later_frame(dev, arpa):
    x = random_logits(5, T=10)
    x[0] = TR.reentry_logits(T=10)
    L = np.array([4, 0, 10])
    ref = reference("plain", arpa, x, L, W=4, K=4)
    sets = ref[0][2]
    assert (3, (1, 2)) in TR.reentries(sets) and (1, 2) in sets[1] and (1, 2) not in sets[2]      # it happened, on the CPU side
    assert ref[0][0][0][0] == (1, 2) and [f for f, _ in ref[0][1][0]] == [0, 3]
    out = one_shot("plain", (None, None), torch.from_numpy(x).to(dev), torch.from_numpy(L).to(dev), W=4, K=4, return_times=True)
    check_invariants(out[0], out[1], out[-1][0], out[-1][1], L)
    check_values(ref, out[0], out[1], *out[-1])
    assert out[-1][0][0, 0, :2].tolist() == [0, 3]                         # not frame 1, where (1, 2) entered first


# ---- 3. commit mode: forced commits, a ring that laps --------------------------------------------------------------------------------
def ragged_steps(T, chunks, seed, B=B):
    """[(begin, end, lengths (B))]: utterance 0 takes every frame, utterance 1 a prefix of each chunk, utterance 2 sometimes none"""
    rng = np.random.default_rng(200 + seed)
    out = []
    for a, b in CR.chunk_ends(T, chunks):
        L = rng.integers(0, b - a + 1, size=B)
        L[0] = b - a
        if len(out) % 3 == 1:
            L[2] = 0
        out.append((a, b, L))
    return out


def counter(st):
    """the (B) int64 absolute frame counts at the head of the times buffer"""
    return st.times[:st.B * 8].view(torch.int64).cpu().tolist()


def run_commit_case(x, steps, M, k_cap, W, K, dev, commit_log=1, **knobs):
    """Device and TimedCommitSearch side by side: after every step the popped (token, frame, logp) triples equal the
    restatement's log of that step; the counter counts each utterance's own frames; an utterance that took no frame keeps its
    log, total and counter.  Returns the restatements and the device's concatenated log."""
    Bx = x.shape[0]
    xt = torch.from_numpy(x).to(dev)
    st = beam_ctc_stream_init(Bx, None, dev, beam_width=W, max_candidates=K, max_pending=M, max_chunk_frames=k_cap,
                              commit_log=commit_log, times=True)
    ref = [TR.TimedCommitSearch(BLANK, W, K, max_pending=M, **knobs) for _ in range(Bx)]
    popped, used, logged = [0] * Bx, [0] * Bx, [[] for _ in range(Bx)]
    for a, b, L in steps:
        before = (st.log.cpu().clone(), st.log_frames.cpu().clone(), st.log_logp.cpu().clone(), st.total.cpu().clone())
        out = beam_ctc_stream_step(st, xt[:, a:b].contiguous(), BLANK, torch.from_numpy(L).to(dev), n_best=N, **knobs)
        ids, total, frames, logps = beam_ctc_stream_committed(st, popped, times=True)
        for u in range(Bx):
            used[u] += int(L[u])
            if L[u]:
                ref[u].step(x[u, a:a + L[u]])
                want = ref[u].log_steps[-1]
                assert ids[u] == [t for t, _, _ in want] and frames[u] == [f for _, f, _ in want], (a, u, ids[u], frames[u], want)
                assert all(ulp_close(g, p) for g, (_, _, p) in zip(logps[u], want)), (a, u)
                logged[u] += list(zip(ids[u], frames[u], logps[u]))
            else:
                assert ids[u] == [] and total[u] == popped[u]
                for now, was in zip((st.log, st.log_frames, st.log_logp), before):
                    assert torch.equal(now.cpu()[u], was[u]), (a, u)
            assert total[u] == len(ref[u].C)
        popped = total
        assert counter(st) == used
        check_invariants(out[0], out[1], out[5][0], out[5][1], used, knobs.get("token_min_logp", -5.0))
    fin = beam_ctc_stream_finish(st, n_best=N)
    check_invariants(fin[0], fin[1], fin[5][0], fin[5][1], used, knobs.get("token_min_logp", -5.0))
    for u in range(Bx):
        hyps = ref[u].finish(N)
        assert min(ref[u].margins.values()) >= MARGIN, (u, ref[u].margins)
        vals = ref[u].final_times(N)
        check_values([(hyps, vals, None)], fin[0][u:u + 1], fin[1][u:u + 1], fin[5][0][u:u + 1], fin[5][1][u:u + 1],
                     offset=[len(ref[u].C)])
        # what was logged is the committed prefix of the final best, with the values it had when it was logged
        assert len(logged[u]) == len(ref[u].C) and [t for t, _, _ in logged[u]] == list(ref[u].C)
        assert all(f == g and ulp_close(p, q) for (_, f, p), (g, q) in zip(logged[u], vals[0])), u
    return ref, logged, st


def test_commit_mode_pops_the_restatements_triples(dev):
    M, k_cap, Tc = 3, 5, 24
    x = random_logits(1, T=Tc)
    steps = ragged_steps(Tc, CHUNKS, 1)
    ref, logged, st = run_commit_case(x, steps, M, k_cap, W, K, dev)
    assert st.log.shape[1] == M + k_cap == st.t_max                        # the smallest ring: L = T_tree
    assert len(logged[0]) > st.log.shape[1]                                # ... and it lapped within the test
    assert ref[0].forced >= 1                                              # at least one step forced a commit (committed > lcp)
    assert any(len(s) == 0 for s in ref[0].log_steps)                      # ... and at least one committed nothing
    assert any(int(L[2]) == 0 for _, _, L in steps) and any(int(L[1]) == 0 for _, _, L in steps)


def test_commit_scan_crosses_waves_at_full_width(dev):
    """W = 100: more than 64 hypotheses are live at a commit and survivors sit past rank 63, so the ranks come from more than
    one wave's ballot.  Wide pruning knobs keep the beam full at V = 8."""
    knobs = dict(token_min_logp=-12.0, beam_prune_logp=-60.0)
    x = random_logits(3, B=1, T=24, V=8)
    steps = [(a, b, np.full(1, b - a)) for a, b in CR.chunk_ends(24, CHUNKS)]

    class Ranks(TR.TimedCommitSearch):
        high = 0

        def _commit(self):
            nodes = [int(n) for n in self.node]
            super()._commit()
            kept = {int(n) for n in self.node}
            Ranks.high = max([Ranks.high] + [r for r, n in enumerate(nodes) if n in kept])

    probe = Ranks(BLANK, 100, 7, max_pending=3, **knobs)
    for a, b, _ in steps:
        probe.step(x[0, a:b])
    assert Ranks.high >= 64, Ranks.high
    ref, _, _ = run_commit_case(x, steps, 3, 5, 100, 7, dev, **knobs)
    assert ref[0].dropped >= 100


# ---- 4. without forcing: C + finish is one-shot, bit for bit; committed values are monotone ----------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_without_forcing_commit_plus_finish_is_one_shot_bit_for_bit(dev, arpa, mode):
    x = random_logits(SEED[mode])
    objs = device_objects(mode, arpa, dev)
    xt, Lt = torch.from_numpy(x).to(dev), torch.from_numpy(LENGTHS).to(dev)
    want = one_shot(mode, objs, xt, Lt, return_times=True)
    wtk, wct, (wtf, wtl) = want[0].cpu(), want[1].cpu(), [t.cpu() for t in want[-1]]
    committed_any = 0
    for chunks in (CHUNKS, (4, 2)):
        st = stream_state(mode, objs, dev, max_frames=None, max_pending=64, max_chunk_frames=5, commit_log=64, times=True)
        prev = [[] for _ in range(B)]
        for a, b in CR.chunk_ends(T, chunks):
            L = np.clip(LENGTHS - a, 0, b - a)
            beam_ctc_stream_step(st, xt[:, a:b].contiguous(), BLANK, torch.from_numpy(L).to(dev), n_best=N)
            ids, total, frames, logps = beam_ctc_stream_committed(st, [0] * B, times=True)
            now = [list(zip(ids[u], frames[u], logps[u])) for u in range(B)]
            assert all(n[:len(p)] == p for n, p in zip(now, prev))         # monotone: what is logged stays as it was logged
            prev = now
        fin = beam_ctc_stream_finish(st, n_best=N)
        ftk, fct, ftf, ftl = fin[0].cpu(), fin[1].cpu(), fin[5][0].cpu(), fin[5][1].cpu()
        committed_any += len(prev[0])
        for u in range(B):
            for r in range(int(fin[4][u])):
                n, c = int(fct[u, r]), len(prev[u])
                assert c + n == int(wct[u, r])
                assert [t for t, _, _ in prev[u]] + ftk[u, r, :n].tolist() == wtk[u, r, :c + n].tolist()
                assert [f for _, f, _ in prev[u]] + ftf[u, r, :n].tolist() == wtf[u, r, :c + n].tolist()
                got = torch.tensor([p for _, _, p in prev[u]] + ftl[u, r, :n].tolist(), dtype=torch.float32)
                assert torch.equal(got, wtl[u, r, :c + n]), (mode, chunks, u, r)
    assert committed_any > 0, "nothing was committed before the finish: the case proves nothing"


# ---- 5. BeamCTCDecoder.words and BeamCTCStream(times=True) ----------------------------------------------------------------------------
def test_decoder_words_and_stream_words_rejoin(dev):
    from conformer_amd.decode import token_words
    dec = BeamCTCDecoder(VOCAB, BLANK, skip_ids=(UNK,), beam_width=W, max_candidates=K, beam_prune_logp=-10.0)
    x = random_logits(2, B=2, T=24)
    xt = torch.from_numpy(x).to(dev)
    want = dec.words(xt, frame_seconds=0.02)
    out = beam_ctc_decode(xt, BLANK, beam_width=W, max_candidates=K, return_times=True)
    for b in range(2):
        n = int(out[1][b, 0])
        assert want[b] == token_words(dec, out[0][b, 0, :n].tolist(), out[-1][0][b, 0, :n].tolist(), out[-1][1][b, 0, :n].tolist(),
                                      0.02)
        assert " ".join(w.text for w in want[b]) == dec(xt)[b] and len(want[b]) >= 1
        assert all(w.end == w.end_frame * 0.02 and w.start_frame < w.end_frame for w in want[b])
    # a committing stream without forcing: popped words + finish_words are the one-shot words; partial_words speaks of the same text
    s = dec.stream(2, None, dev, max_pending=64, max_chunk_frames=5, times=True, frame_seconds=0.02)
    got, popped_any = [[], []], 0
    for a, b in CR.chunk_ends(24, CHUNKS):
        s.step(xt[:, a:b])
        assert [" ".join(w.text for w in ws) for ws in s.partial_words()] == s.partial_text()
        for u, ws in enumerate(s.pop_committed_words()):
            got[u] += ws
            popped_any += len(ws)
    tail = s.finish_words()
    assert popped_any > 0 and [got[u] + tail[u] for u in range(2)] == want
    # reset_slots: utterance 1 starts again, its frames count from 0 again and its held tail is gone
    s.reset()
    s.step(xt[:, :5])
    s.pop_committed_words()
    s.reset_slots([1])
    assert s.held[1] == [] and counter(s.state) == [5, 0]
    s.step(xt[:, 5:9], torch.tensor([0, 4]))
    assert counter(s.state) == [5, 4]
    one = dec.stream(1, None, dev, max_pending=64, max_chunk_frames=5, times=True, frame_seconds=0.02)
    one.step(xt[1:2, 5:9])
    assert s.finish_words(only=[1])[1] == one.finish_words()[0]


# ---- 6. SlotTranscriber(times=True) -------------------------------------------------------------------------------------------------
SLOT_VOCAB = ["<pad>"] + [chr(ord("a") + i) for i in range(14)] + ["|", "<unk>"]


def tiny_model(seed, dev):
    from model.conformer import Conformer
    from oracle import conformer_oracle as O
    P = O.make_params(vocab=len(SLOT_VOCAB), n_mel=80, n_blocks=2, d=32, n_heads=4, ksize=31, lstm_hidden=24, seed=seed)
    m = Conformer(len(SLOT_VOCAB), 80, 2, 32, 4, 31, 24, 1, 0.0)
    m.load_state_dict(P, strict=True)
    return m.to(dev).eval()


def test_slot_transcriber_words_count_from_the_slots_own_open(dev):
    from conformer_amd.slots import SlotTranscriber
    m = tiny_model(71, dev)
    dec = BeamCTCDecoder(SLOT_VOCAB, 0, skip_ids=(16,), beam_width=16)
    kw = dict(left_context=8, max_chunk_mel_frames=64, max_pending=4)
    tr, tr0 = SlotTranscriber(m, dec, 2, None, times=True, **kw), SlotTranscriber(m, dec, 2, None, **kw)
    assert tr0.beam.state.times is None and not tr0.beam.times              # times=False: nothing is allocated
    k_cap = tr.commit[1]
    g = torch.Generator().manual_seed(5)
    mel = torch.randn(2, 80, 4 * 64, generator=g).mul(3.0).to(dev)
    # slot 0 from step 0 on; slot 1 is opened at step 2 (late) and takes the mel frames slot 0 took from the start
    sched = [[64, 0], [64, 0], [64, 64], [40, 64], [0, 50]]
    pos, fed, popped = [0, 0], {0: [], 1: []}, {0: [], 1: []}
    for i, fr in enumerate(sched):
        if i == 0:
            tr.open(0), tr0.open(0)
        if i == 2:
            tr.open(1), tr0.open(1)
        chunk = torch.zeros(2, 80, 64, device=dev)
        for s in range(2):
            chunk[s, :, :fr[s]] = mel[0, :, pos[s]:pos[s] + fr[s]]          # both slots hear the same audio
            pos[s] += fr[s]
        logits, k = tr.step(chunk, fr)
        tr0.step(chunk, fr)
        for s in range(2):
            if k[s]:
                fed[s].append(logits[s:s + 1, :k[s]].clone())
        for s, ws in tr.pop_committed_words().items():
            popped[s] += ws
        assert {s: " ".join(w.text for w in ws) for s, ws in tr.partial_words().items()} == tr.partial_text()
    words = {s: popped[s] + tr.close_words(s) for s in range(2)}
    texts0 = {s: tr0.close(s) for s in range(2)}
    assert not any(tr.is_open) and int(tr.beam.state.total.sum()) == 0
    for s in range(2):
        assert " ".join(w.text for w in words[s]) == texts0[s] and len(words[s]) >= 1       # the times=False transcript, unchanged
        n_frames = sum(f.shape[1] for f in fed[s])
        assert all(0 <= w.start_frame < w.end_frame <= n_frames for w in words[s])          # frames of the slot's own stream
        # a one-utterance search over the slot's own logits: the same Words exactly
        ref = dec.stream(1, None, dev, max_pending=4, max_chunk_frames=k_cap, times=True)
        for c in fed[s]:
            ref.step(c)
        assert ref.finish_words()[0] == words[s], s
    # slot 1 heard a prefix of slot 0's audio two steps later: its words carry ITS frames, not the batch's
    one = SlotTranscriber(m, dec, 1, None, times=True, **kw)
    one.open(0)
    p = 0
    for fr in (64, 64, 50):
        one.step(mel[:1, :, p:p + fr].contiguous(), [fr])
        p += fr
    solo = one.close_words(0)
    assert [(w.text, w.start_frame, w.end_frame) for w in solo] == [(w.text, w.start_frame, w.end_frame) for w in words[1]]
    # (the two runs' logits agree to ~1e-5 relative, tests/test_stream_slots_gpu.py; a mean log-probability then to far below 1e-3)
    assert all(abs(a.score - b.score) < 1e-3 for a, b in zip(solo, words[1]))
