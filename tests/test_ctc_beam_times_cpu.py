"""Host-side checks of the beam search's timestamps: the two float64 statements of the rule against each other, the word
assembly of BeamCTCStream over a fake search state, the fourth header and its binding, argument validation of the new C entries
(it happens before any HIP call, so it runs without a GPU) and the Python refusals."""
import ctypes
import math
import os
import types

import numpy as np
import pytest
import torch

from conformer_amd import _lib, build, decode
from conformer_amd.align import Word
from tests import ctc_beam_commit_restatement as CR
from tests import ctc_beam_restatement as R
from tests import ctc_beam_times_restatement as TR

OK, BAD_SHAPE, UNSUPPORTED, NULL = 0, -1, -2, -3
CHUNKS = [1, 5, 3]
NAMES = {"cfm_ctc_beam_times_bytes", "cfm_ctc_beam_times_reset", "cfm_ctc_beam_stream_step_times_f32",
         "cfm_ctc_beam_stream_finish_times_f32", "cfm_ctc_beam_stream_commit_times"}
KW = dict(beam_width=6, max_candidates=4)


def logits(seed, T=24, V=7):
    return (3 * np.random.default_rng(seed).normal(size=(T, V))).astype(np.float32)


def live_values(x, n_best):
    """statement 1 on the plain search: the final hypotheses and their value tuples"""
    T = x.shape[0]
    sets = TR.live_sets(lambda lg, **kw: R.beam_search(lg, 0, **KW, **kw), x, T, KW["beam_width"])
    vals = TR.times_from_live_sets(sets, R.log_softmax64(x))
    hyps, _ = R.beam_search(x, 0, n_best=n_best, **KW)
    return hyps, [vals[-1][seq] for seq, _ in hyps], sets


def check_invariants(seq, vals, consumed, token_min_logp=-5.0):
    frames = [f for f, _ in vals]
    assert len(vals) == len(seq)
    assert all(a < b for a, b in zip(frames, frames[1:]))                  # strictly increasing
    assert all(f >= i for i, f in enumerate(frames))
    assert all(0 <= f < consumed for f in frames)
    assert all(p >= token_min_logp for _, p in vals)


# ---- the two statements ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_the_two_statements_agree_without_commit(seed):
    x = logits(seed)
    hyps, vals, sets = live_values(x, 6)
    for chunks in ([24], CHUNKS):
        got, gvals, _ = TR.timed_commit_search(x, chunks, 0, None, n_best=6, **KW)
        assert got == hyps and gvals == vals
    for (seq, _), v in zip(hyps, vals):
        check_invariants(seq, v, 24)
        lp = R.log_softmax64(x)
        assert all(p == lp[f, c] for c, (f, p) in zip(seq, v))
    assert sum(len(s) for s, _ in hyps) > 6


@pytest.mark.parametrize("seed", range(4))
def test_the_two_statements_agree_with_a_commit_that_forces_nothing(seed):
    x = logits(seed)
    hyps, vals, _ = live_values(x, 6)
    for chunks in (CHUNKS, [2, 7]):
        got, gvals, cs = TR.timed_commit_search(x, chunks, 0, 10 ** 6, n_best=6, **KW)
        assert cs.forced == 0 and cs.dropped == 0 and len(cs.C) > 0
        assert got == hyps and gvals == vals                               # the commit changed no value of a survivor
        logged = [e for step in cs.log_steps for e in step]
        assert [e[0] for e in logged] == list(cs.C)
        assert [(f, p) for _, f, p in logged] == list(vals[0][:len(cs.C)])  # the log took y_0's values, each exactly once


@pytest.mark.parametrize("M", [1, 3])
def test_forced_commits_keep_the_invariants_and_never_rewrite_the_log(M):
    forced = 0
    for seed in range(4):
        x = logits(seed)
        got, gvals, cs = TR.timed_commit_search(x, CHUNKS, 0, M, n_best=1, **KW)
        forced += cs.forced
        logged = [e for step in cs.log_steps for e in step]
        assert len(cs.log_steps) == len(CR.chunk_ends(24, CHUNKS))
        assert [(f, p) for _, f, p in logged] == list(gvals[0][:len(logged)])
        check_invariants(got[0][0], gvals[0], 24)
    assert forced >= 3


def test_a_pruned_prefix_that_re_enters_gets_the_later_frame():
    """TR.reentry_logits: (1, 2) is live after frame 1, cut at frame 2 and found again at frame 3."""
    x = TR.reentry_logits(T=4)
    kw = dict(beam_width=4, max_candidates=4)
    sets = TR.live_sets(lambda lg, **k: R.beam_search(lg, 0, **kw, **k), x, 4, 4)
    assert (1, 2) in sets[1] and (1, 2) not in sets[2] and (1,) in sets[2] and sets[3][0] == (1, 2)
    assert (3, (1, 2)) in TR.reentries(sets)
    vals = TR.times_from_live_sets(sets, R.log_softmax64(x))
    assert [f for f, _ in vals[1][(1, 2)]] == [0, 1] and [f for f, _ in vals[3][(1, 2)]] == [0, 3]
    got, gvals, _ = TR.timed_commit_search(x, [1, 2], 0, None, n_best=4, **kw)
    assert got[0][0] == (1, 2) and gvals == [vals[-1][seq] for seq, _ in got]


# ---- word assembly on the host (a fake search state: the rings and totals are CPU tensors the test writes) ----------------------
VOCAB = ["_", "a", "b", "|", "<unk>"]
A, Bt, D, U = 1, 2, 3, 4


class FakeSource:
    """Stands in for the device state: commit(b, triples) appends to utterance b's rings as the commit kernel does."""

    def __init__(self, B, L=8):
        self.st = types.SimpleNamespace(B=B, log=torch.zeros(B, L, dtype=torch.int32), total=torch.zeros(B, dtype=torch.int64),
                                        log_frames=torch.full((B, L), -1, dtype=torch.int64),
                                        log_logp=torch.full((B, L), -math.inf), committed=None)
        self.L = L

    def commit(self, b, triples):
        for tok, f, p in triples:
            at = int(self.st.total[b]) % self.L
            self.st.log[b, at], self.st.log_frames[b, at], self.st.log_logp[b, at] = tok, f, p
            self.st.total[b] += 1


@pytest.fixture
def fake(monkeypatch):
    src = FakeSource(2)
    resets = []
    monkeypatch.setattr(decode, "beam_ctc_stream_init", lambda *a, **kw: src.st)
    monkeypatch.setattr(decode, "beam_ctc_stream_reset_slots", lambda st, idx: resets.extend(idx.tolist()))
    dec = decode.BeamCTCDecoder(VOCAB, blank_id=0, skip_ids=(U,), beam_width=4)
    s = dec.stream(2, None, "cpu", max_pending=4, max_chunk_frames=4, times=True, frame_seconds=0.5)
    assert s.times and s.commit and s.held == [[], []]
    return src, s, resets, dec


def test_a_word_split_across_three_commits_and_doubled_delimiters(fake):
    src, s, _, _ = fake
    src.commit(0, [(A, 0, -0.5)])
    assert s.pop_committed_words() == [[], []] and s.held[0] == [(A, 0, -0.5)] and s.popped == [1, 0]
    assert s.pop_committed() == [[], []]                                   # held tokens are popped: never handed out as ids
    src.commit(0, [(Bt, 2, -1.5)])
    assert s.pop_committed_words() == [[], []] and len(s.held[0]) == 2
    src.commit(0, [(D, 5, -0.1), (D, 6, -0.1), (A, 9, -0.25)])            # the ring of 8 holds them; doubled delimiter
    words = s.pop_committed_words()
    assert words == [[Word("ab", 0, 3, 0.0, 1.5, -1.0)], []]               # frames 0 and 2: [0, 3), mean(-0.5, -1.5)
    assert s.held[0] == [(A, 9, -0.25)] and s.popped == [5, 0]
    assert s.committed_text() == ["a", ""]                                 # the texts still begin with the held tokens


def test_skip_ids_only_and_the_ring_wrapping(fake):
    src, s, _, _ = fake
    src.commit(0, [(U, 1, -2.0), (A, 2, -1.0), (D, 3, -0.5)])
    src.commit(1, [(Bt, 0, -0.5), (D, 1, -0.5)])
    assert s.pop_committed_words(only=[0]) == [[Word("a", 1, 3, 0.5, 1.5, -1.5)], []]   # <unk>: span and score, no characters
    assert s.popped == [3, 0]                                              # utterance 1 was not read
    src.commit(0, [(Bt, 10 + i, -1.0) for i in range(6)] + [(D, 20, -0.5)])            # positions 3..9 wrap the ring of 8
    assert s.pop_committed_words() == [[Word("bbbbbb", 10, 16, 5.0, 8.0, -1.0)], [Word("b", 0, 1, 0.0, 0.5, -0.5)]]
    src.commit(1, [(A, 30 + i, -1.0) for i in range(9)])                   # more than the ring since the last pop
    with pytest.raises(RuntimeError, match=r"utterance\(s\) \[1\]"):
        s.pop_committed_words()
    assert s.pop_committed_words(only=[0]) == [[], []]                     # utterance 0 is not held up
    s.discard_committed(only=[1])
    assert s.pop_committed_words() == [[], []]


def test_partial_and_finish_with_a_held_tail_and_reset_slots(fake, monkeypatch):
    src, s, resets, dec = fake
    src.commit(0, [(A, 0, -0.5), (D, 1, -0.5), (Bt, 2, -1.0)])
    assert s.pop_committed_words() == [[Word("a", 0, 1, 0.0, 0.5, -0.5)], []] and s.held[0] == [(Bt, 2, -1.0)]
    assert s.partial_words() == [[], []]                                   # nothing stepped yet
    src.commit(0, [(A, 4, -3.0)])
    # the latest step: its best is relative to the prefix before it, of which it committed 1 token (utterance 0) / 0
    pad = lambda rows, fill, dt: torch.tensor([[r + [fill] * (4 - len(r))] for r in rows], dtype=dt)
    s.last = (pad([[A, Bt], [A]], -1, torch.int64), torch.tensor([[2], [1]]), None, None, None,
              (pad([[4, 6], [7]], -1, torch.int64), pad([[-3.0, -2.0], [-0.25]], -math.inf, torch.float32)))
    s.last_committed, s.fresh = torch.tensor([1, 0], dtype=torch.int32), set()
    assert s.partial_words() == [[Word("bab", 2, 7, 1.0, 3.5, -2.0)], [Word("a", 7, 8, 3.5, 4.0, -0.25)]]
    assert s.partial_text() == ["bab", "a"]
    assert s.held[0] == [(Bt, 2, -1.0)] and s.popped == [3, 0]             # nothing moved
    fin = (pad([[D, A], []], -1, torch.int64), torch.tensor([[2], [0]]), None, None, None,
           (pad([[8, 9], []], -1, torch.int64), pad([[-0.5, -1.0], []], -math.inf, torch.float32)))
    monkeypatch.setattr(decode, "beam_ctc_stream_finish", lambda st, n_best=1: fin)
    assert s.finish_words(only=[0]) == [[Word("ba", 2, 5, 1.0, 2.5, -2.0), Word("a", 9, 10, 4.5, 5.0, -1.0)], []]
    assert not s.finished
    s.reset_slots([0])
    assert resets == [0] and s.held[0] == [] and s.popped[0] == 0 and 0 in s.fresh
    src.st.total[0] = 0                                                    # (what the device reset does)
    assert s.finish_words() == [[Word("a", 9, 10, 4.5, 5.0, -1.0)], []] and s.finished
    with pytest.raises(RuntimeError, match="reset"):
        s.finish_words()


def test_streams_without_times_or_commit_refuse_the_word_calls(monkeypatch):
    monkeypatch.setattr(decode, "beam_ctc_stream_init", lambda *a, **kw: FakeSource(1).st)
    dec = decode.BeamCTCDecoder(VOCAB, blank_id=0, beam_width=4)
    plain = dec.stream(1, None, "cpu", max_pending=4, max_chunk_frames=4)
    for call in (plain.pop_committed_words, plain.partial_words, plain.finish_words):
        with pytest.raises(RuntimeError, match="times=True"):
            call()
    assert plain.held == [[]] and plain.pop_committed() == [[]]            # the id path is the one it was
    ending = dec.stream(1, 10, "cpu", times=True)
    with pytest.raises(RuntimeError, match="without max_pending"):
        ending.pop_committed_words()


# ---- header and binding ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def buf():
    raw = (ctypes.c_char * 4096)()
    a = ctypes.addressof(raw)
    return raw, (a + 15) // 16 * 16


def test_times_header_is_bound_from_its_own_table(lib):
    """what every header shares (record, names, binding, rebuild message, build) is asserted in test_abi_binding_cpu"""
    header = _lib.HEADERS["conformer_hip_times.h"]
    sigs, params = header.signatures, header.params
    assert set(sigs) == NAMES and not NAMES & set(_lib.SIGNATURES)
    assert sigs["cfm_ctc_beam_times_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    # the *_times entries take the plain entries' lists, then the four times arguments, then the stream
    for plain, timed in (("cfm_ctc_beam_stream_step_f32", "cfm_ctc_beam_stream_step_times_f32"),
                         ("cfm_ctc_beam_stream_finish_f32", "cfm_ctc_beam_stream_finish_times_f32")):
        assert params[timed] == _lib.PARAMS[plain][:-1] + ["times", "times_bytes", "token_frames", "token_logp", "stream"]
    assert params["cfm_ctc_beam_stream_commit_times"] == (_lib.PARAMS["cfm_ctc_beam_stream_commit"][:-1]
                                                          + ["times", "times_bytes", "log_frames", "log_logp", "stream"])
    assert lib.cfm_abi_version() == _lib.ABI_VERSION


def test_times_bytes(lib):
    f = lib.cfm_ctc_beam_times_bytes
    base = dict(B=3, T=24, W=8, M=0)
    for name, values in (("B", (1, 2, 3, 64)), ("T", (9, 24, 100)), ("W", (1, 8, 100, 256)), ("M", (0, 1, 8))):
        sizes = [f(*{**base, name: v}.values()) for v in values]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes), (name, sizes)
    # the counter and one 8-byte record per tree node, each rounded to 256 bytes
    assert f(3, 24, 8, 0) == 256 + -(-3 * (1 + 24 * 8) * 8 // 256) * 256
    for args in ((0, 24, 8, 0), (3, 0, 8, 0), (3, 24, 0, 0), (3, 24, 257, 0), (3, 24, 8, -1), (3, 24, 8, 24), (3, 1 << 23, 256, 0)):
        assert f(*args) == 0, args


def _step(lib, p, **kw):
    a = dict(logits=p, lengths=None, B=2, Tc=4, V=5, blank=0, W=4, K=4, tmin=-5.0, prune=-10.0, N=1, lm=None, alpha=0.0, beta=0.0,
             unk=0.0, sb=0, hw=None, hww=0.0, state=p, state_bytes=1 << 40, T_max=20, t_used=0, tokens=p, counts=p, scores=p,
             am=None, num=p, times=p, times_bytes=1 << 40, tf=p, tl=p, stream=None)
    a.update(kw)
    return lib.cfm_ctc_beam_stream_step_times_f32(*a.values())


def _finish(lib, p, **kw):
    a = dict(B=2, W=4, K=4, N=1, lm=None, alpha=0.0, beta=0.0, unk=0.0, sb=0, hw=None, hww=0.0, state=p, state_bytes=1 << 40,
             T_max=20, tokens=p, counts=p, scores=p, am=None, num=p, times=p, times_bytes=1 << 40, tf=p, tl=p, stream=None)
    a.update(kw)
    return lib.cfm_ctc_beam_stream_finish_times_f32(*a.values())


def _commit(lib, p, **kw):
    a = dict(B=2, M=4, k=16, W=4, K=4, lm=0, hw=0, lengths=None, state=p, state_bytes=1 << 40, log=p, L=20, total=p,
             committed=None, times=p, times_bytes=1 << 40, lf=p, ll=p, stream=None)
    a.update(kw)
    return lib.cfm_ctc_beam_stream_commit_times(*a.values())


def test_times_entries_reject_bad_arguments_before_any_launch(lib, buf):
    _, p = buf
    need = lib.cfm_ctc_beam_times_bytes(2, 20, 4, 0)
    for fn in (_step, _finish):
        for name in ("times", "tf", "tl", "state", "tokens"):
            assert fn(lib, p, **{name: None}) == NULL, (fn.__name__, name)
        assert fn(lib, p, times_bytes=need - 1) == BAD_SHAPE
        assert fn(lib, p, W=0) == UNSUPPORTED and fn(lib, p, B=0) == BAD_SHAPE
        assert fn(lib, p, state_bytes=8) == BAD_SHAPE
    assert _step(lib, p, Tc=0) == BAD_SHAPE and _step(lib, p, t_used=18) == BAD_SHAPE
    needc = lib.cfm_ctc_beam_times_bytes(2, 20, 4, 4)
    assert needc > need
    for name in ("times", "lf", "ll", "state", "log", "total"):
        assert _commit(lib, p, **{name: None}) == NULL, name
    assert _commit(lib, p, times_bytes=needc - 1) == BAD_SHAPE and _commit(lib, p, times_bytes=need) == BAD_SHAPE
    assert _commit(lib, p, M=0) == BAD_SHAPE and _commit(lib, p, L=19) == BAD_SHAPE and _commit(lib, p, W=257) == UNSUPPORTED
    r = lib.cfm_ctc_beam_times_reset
    assert r(2, None, 0, None, 1 << 20, None) == NULL
    assert r(0, None, 0, p, 1 << 20, None) == BAD_SHAPE and r(2, None, 1, p, 1 << 20, None) == BAD_SHAPE
    assert r(2, p, 0, p, 1 << 20, None) == BAD_SHAPE and r(2, p, 3, p, 1 << 20, None) == BAD_SHAPE
    assert r(2, None, 0, p, 8, None) == BAD_SHAPE


# ---- Python refusals (raised before the model, the decoder or a device is used) -----------------------------------------------
def test_python_refusals():
    from conformer_amd.slots import SlotTranscriber
    from conformer_amd.transcribe import StreamingTranscriber
    x = torch.zeros(1, 4, 5)
    dec = decode.BeamCTCDecoder(VOCAB, blank_id=0, beam_width=4)
    with pytest.raises(ValueError, match="return_times"):
        decode.beam_ctc_decode(x, 0, return_times=1)
    with pytest.raises(ValueError, match="return_times"):
        decode.beam_ctc_lm_decode(x, 0, None, vocab=VOCAB, return_times="yes")
    with pytest.raises(ValueError, match="return_times"):
        decode.beam_ctc_hotword_decode(x, 0, ["a"], vocab=VOCAB, return_times=None)
    with pytest.raises(ValueError, match="times"):
        decode.beam_ctc_stream_init(2, 10, "cpu", times=1)
    with pytest.raises(ValueError, match="times"):
        dec.stream(2, 10, "cpu", times="on")
    for bad in (0, -0.04, math.inf, math.nan, "0.04", True):
        with pytest.raises(ValueError, match="frame_seconds"):
            dec.stream(2, 10, "cpu", times=True, frame_seconds=bad)
        with pytest.raises(ValueError, match="frame_seconds"):
            dec.words(x, frame_seconds=bad)
    for cls in (StreamingTranscriber, SlotTranscriber):
        with pytest.raises(ValueError, match="times"):
            cls(None, None, 2, 100, times=1)
        with pytest.raises(ValueError, match="frame_seconds"):
            cls(None, None, 2, 100, times=True, frame_seconds=0.0)
