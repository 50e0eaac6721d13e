"""Host-side checks of the streaming (resumable) beam search and the carried LSTM entries: argument validation happens before
any HIP call, so it runs without a GPU; the stream buffer size; BeamCTCStream's life cycle (its device calls replaced)."""
import ctypes

import pytest
import torch

from conformer_amd import _lib, build, decode

OK, BAD_SHAPE, UNSUPPORTED, NULL, ALIGN = 0, -1, -2, -3, -6


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def buf():
    """a 16-byte aligned host address with room for every pointer argument (nothing is launched, nothing dereferenced)"""
    raw = (ctypes.c_char * 4096)()
    a = ctypes.addressof(raw)
    return raw, (a + 15) // 16 * 16


def test_state_bytes_monotone_and_zero_when_invalid(lib):
    f = lib.cfm_ctc_beam_stream_state_bytes
    for lm in (0, 1):
        for hw in (0, 1):
            sizes_t = [f(3, T, 16, 8, lm, hw) for T in (1, 2, 7, 100, 1000)]
            assert all(s > 0 for s in sizes_t) and sizes_t == sorted(sizes_t) and len(set(sizes_t)) == len(sizes_t)
            sizes_w = [f(3, 50, W, 8, lm, hw) for W in (1, 2, 16, 100, 256)]
            assert all(s > 0 for s in sizes_w) and sizes_w == sorted(sizes_w) and len(set(sizes_w)) == len(sizes_w)
            # the state of the modes only adds: plain <= lm, hw <= lm + hw
            assert f(3, 50, 16, 8, 0, 0) <= f(3, 50, 16, 8, lm, hw) <= f(3, 50, 16, 8, 1, 1)
            # at least the one-shot workspace for T_max frames
            assert f(3, 50, 16, 8, lm, hw) > lib.cfm_ctc_beam_workspace_bytes(3, 50, 16, 8)
    for args in ((0, 5, 4, 4), (2, 0, 4, 4), (2, 5, 0, 4), (2, 5, 257, 4), (2, 5, 4, 0), (2, 5, 4, 33), (2, 1 << 24, 256, 4)):
        assert f(*args, 0, 0) == 0 and f(*args, 1, 1) == 0


def _step(lib, p, **kw):
    a = dict(logits=p, lengths=None, B=2, Tc=5, V=7, blank=0, W=4, K=4, tmin=-5.0, prune=-10.0, N=2, lm=None, alpha=1.0,
             beta=1.0, unk=-10.0, sb=1, hw=None, hww=1.0, state=p, state_bytes=1 << 40, T_max=20, t_used=0, tokens=p,
             counts=p, scores=p, am=None, num_hyps=p, stream=None)
    a.update(kw)
    return lib.cfm_ctc_beam_stream_step_f32(*a.values())


def _finish(lib, p, **kw):
    a = dict(B=2, W=4, K=4, N=2, lm=None, alpha=1.0, beta=1.0, unk=-10.0, sb=1, hw=None, hww=1.0, state=p, state_bytes=1 << 40,
             T_max=20, tokens=p, counts=p, scores=p, am=None, num_hyps=p, stream=None)
    a.update(kw)
    return lib.cfm_ctc_beam_stream_finish_f32(*a.values())


def test_stream_step_rejects_bad_arguments_before_any_launch(lib, buf):
    _, p = buf
    for name in ("logits", "state", "tokens", "counts", "scores", "num_hyps"):
        assert _step(lib, p, **{name: None}) == NULL, name
    assert _step(lib, p, W=0) == UNSUPPORTED and _step(lib, p, W=257) == UNSUPPORTED
    assert _step(lib, p, K=0) == UNSUPPORTED and _step(lib, p, K=33) == UNSUPPORTED
    assert _step(lib, p, N=0) == BAD_SHAPE and _step(lib, p, N=5) == BAD_SHAPE
    assert _step(lib, p, V=1) == BAD_SHAPE and _step(lib, p, blank=7) == BAD_SHAPE
    assert _step(lib, p, V=(1 << 23) + 1) == UNSUPPORTED
    assert _step(lib, p, B=0) == BAD_SHAPE and _step(lib, p, Tc=0) == BAD_SHAPE and _step(lib, p, T_max=0) == BAD_SHAPE
    # a chunk that could carry an utterance past T_max
    assert _step(lib, p, Tc=21) == BAD_SHAPE
    assert _step(lib, p, Tc=6, t_used=15) == BAD_SHAPE
    assert _step(lib, p, Tc=1, t_used=20) == BAD_SHAPE
    assert _step(lib, p, t_used=-1) == BAD_SHAPE
    # NaN knobs, non-finite LM / hotword knobs, a buffer smaller than the state
    assert _step(lib, p, tmin=float("nan")) == BAD_SHAPE and _step(lib, p, prune=float("nan")) == BAD_SHAPE
    assert _step(lib, p, alpha=float("inf")) == BAD_SHAPE and _step(lib, p, hww=float("nan")) == BAD_SHAPE
    need = lib.cfm_ctc_beam_stream_state_bytes(2, 20, 4, 4, 0, 0)
    assert _step(lib, p, state_bytes=need - 1) == BAD_SHAPE
    need_lm = lib.cfm_ctc_beam_stream_state_bytes(2, 20, 4, 4, 1, 0)
    assert _step(lib, p, state_bytes=need, lm=p) == BAD_SHAPE and need_lm > need


def test_stream_init_and_finish_reject_bad_arguments_before_any_launch(lib, buf):
    _, p = buf
    init = lib.cfm_ctc_beam_stream_init
    assert init(2, 20, 4, 4, None, 1, None, None, 1 << 40, None) == NULL
    assert init(0, 20, 4, 4, None, 1, None, p, 1 << 40, None) == BAD_SHAPE
    assert init(2, 0, 4, 4, None, 1, None, p, 1 << 40, None) == BAD_SHAPE
    assert init(2, 20, 0, 4, None, 1, None, p, 1 << 40, None) == UNSUPPORTED
    assert init(2, 20, 4, 33, None, 1, None, p, 1 << 40, None) == UNSUPPORTED
    need = lib.cfm_ctc_beam_stream_state_bytes(2, 20, 4, 4, 0, 1)
    assert init(2, 20, 4, 4, None, 1, p, p, need - 1, None) == BAD_SHAPE
    for name in ("state", "tokens", "counts", "scores", "num_hyps"):
        assert _finish(lib, p, **{name: None}) == NULL, name
    assert _finish(lib, p, lm=p) == NULL and _finish(lib, p, hw=p) == NULL        # am_scores required with LM / hotwords
    assert _finish(lib, p, W=300) == UNSUPPORTED and _finish(lib, p, K=0) == UNSUPPORTED
    assert _finish(lib, p, N=5) == BAD_SHAPE and _finish(lib, p, B=0) == BAD_SHAPE
    assert _finish(lib, p, state_bytes=lib.cfm_ctc_beam_stream_state_bytes(2, 20, 4, 4, 0, 0) - 1) == BAD_SHAPE
    assert _finish(lib, p, hww=float("inf"), am=p, hw=p) == BAD_SHAPE


def test_carried_lstm_entries_reject_bad_arguments(lib, buf):
    _, p = buf
    f32, frag, m16 = lib.cfm_lstm_fwd_carry_f32, lib.cfm_lstm_fwd_frag_carry_f32, lib.cfm_lstm_fwd_mfma16_carry_f32
    assert f32(p, p, None, p, None, p, None, None, 2, 3, 8, None) == NULL            # h_state
    assert f32(p, p, None, p, p, None, None, None, 2, 3, 8, None) == NULL            # c_state
    assert f32(p, p, None, p, p, p, None, None, 2, 3, 6, None) == BAD_SHAPE          # H % 4
    assert f32(p, p, None, p, p + 4, p, None, None, 2, 3, 8, None) == ALIGN          # h_state read as float4
    assert frag(p, p, None, p, p, p, None, None, None, 2, 3, 16, None) == NULL       # scratch
    assert frag(p, p, None, p, p, p, p, None, None, 2, 3, 20, None) == BAD_SHAPE     # H % 16
    assert m16(1, p, p, None, p, None, p, p, None, None, 2, 3, 16, None) == NULL
    assert m16(1, p, p, None, p, p, p, p, None, None, 2, 0, 16, None) == BAD_SHAPE


def test_lstm_forward_state_is_checked():
    from conformer_amd import ops
    with pytest.raises(Exception):
        ops.lstm_forward(torch.zeros(2, 3, 8), torch.zeros(32, 8), torch.zeros(32, 8), torch.zeros(32),
                         state=(torch.zeros(2, 8), torch.zeros(2, 8)))


def test_stream_life_cycle(monkeypatch):
    """step after finish raises until reset(); finish twice raises; partial_text before a step is empty.  The device calls are
    replaced by stand-ins that record the call order."""
    calls = []

    class FakeState:
        B, t_max, t_used = 2, 10, 0

    def fake_init(batch, max_frames, device, **kw):
        calls.append("init")
        return FakeState()

    def fake_step(st, x, blank, lengths, **kw):
        calls.append("step")
        return (torch.full((2, 1, 10), -1, dtype=torch.int64), torch.zeros(2, 1, dtype=torch.int64), torch.zeros(2, 1), None,
                torch.ones(2, dtype=torch.int64))

    def fake_finish(st, n_best=1):
        calls.append("finish")
        tokens = torch.full((2, 1, 10), -1, dtype=torch.int64)
        tokens[0, 0, :2] = torch.tensor([1, 2])
        return tokens, torch.tensor([[2], [0]]), torch.zeros(2, 1), None, torch.ones(2, dtype=torch.int64)

    monkeypatch.setattr(decode, "beam_ctc_stream_init", fake_init)
    monkeypatch.setattr(decode, "beam_ctc_stream_reset", lambda st: calls.append("reset"))
    monkeypatch.setattr(decode, "beam_ctc_stream_step", fake_step)
    monkeypatch.setattr(decode, "beam_ctc_stream_finish", fake_finish)
    dec = decode.BeamCTCDecoder(["_", "a", "b", "|"], blank_id=0, beam_width=4)
    s = dec.stream(2, 10, device="cpu")
    assert isinstance(s, decode.BeamCTCStream)
    assert s.partial_text() == ["", ""]
    lengths = torch.tensor([3, 0])
    s.step(torch.zeros(2, 3, 4), lengths)
    assert s.partial_text() == ["", ""]
    assert s.finish() == ["ab", ""]
    with pytest.raises(RuntimeError, match="after finish"):
        s.step(torch.zeros(2, 3, 4))
    with pytest.raises(RuntimeError):
        s.finish()
    s.reset()
    s.step(torch.zeros(2, 3, 4))
    assert s.finish(decode_func=str.upper) == ["AB", ""]
    assert calls == ["init", "step", "finish", "reset", "step", "finish"]


# ---- per-utterance operation (independent streams): the device calls replaced as above, B = 3 --------------------------------
VOCAB4 = ["_", "a", "b", "|"]


@pytest.fixture
def stream3(monkeypatch):
    """(stream, calls): a BeamCTCStream over 3 utterances whose step n returns, for every utterance, n tokens `a` (step 1: "a",
    step 2: "aa") and whose finish returns "ab", "b", "ba"; calls records (name, what the stand-in was given)."""
    import types
    calls = []

    def fake_step(st, x, blank, lengths, **kw):
        calls.append(("step", kw))
        n = sum(1 for c in calls if c[0] == "step")
        tokens = torch.full((3, 1, 10), -1, dtype=torch.int64)
        tokens[:, 0, :n] = 1
        return tokens, torch.full((3, 1), n, dtype=torch.int64), torch.zeros(3, 1), None, torch.ones(3, dtype=torch.int64)

    def fake_finish(st, n_best=1):
        calls.append(("finish", None))
        tokens = torch.tensor([[[1, 2, -1]], [[2, -1, -1]], [[2, 1, -1]]])
        return tokens, torch.tensor([[2], [1], [2]]), torch.zeros(3, 1), None, torch.ones(3, dtype=torch.int64)

    monkeypatch.setattr(decode, "beam_ctc_stream_init", lambda *a, **kw: types.SimpleNamespace(B=3, t_max=10, t_used=0))
    monkeypatch.setattr(decode, "beam_ctc_stream_reset", lambda st: calls.append(("reset", None)))
    monkeypatch.setattr(decode, "beam_ctc_stream_reset_slots", lambda st, idx: calls.append(("reset_slots", idx.tolist())))
    monkeypatch.setattr(decode, "beam_ctc_stream_step", fake_step)
    monkeypatch.setattr(decode, "beam_ctc_stream_finish", fake_finish)
    return decode.BeamCTCDecoder(VOCAB4, blank_id=0, beam_width=4).stream(3, 10, device="cpu"), calls


def test_reset_slots_marks_fresh_until_the_next_step(stream3):
    s, calls = stream3
    s.popped = [5, 6, 7]
    s.step(torch.zeros(3, 2, 4))
    assert s.partial_text() == ["a", "a", "a"]
    s.reset_slots([1])
    assert calls[-1] == ("reset_slots", [1])
    assert s.partial_text() == ["a", "", "a"]                     # `last` still holds the previous occupant's row 1
    assert s.partial_text(only=[1, 2]) == ["", "", "a"]
    assert s.popped == [5, 0, 7]
    s.step(torch.zeros(3, 2, 4))
    assert s.partial_text() == ["aa", "aa", "aa"] and s.popped == [5, 0, 7]
    s.reset()                                                      # every utterance fresh, as before the first step
    assert s.partial_text() == ["", "", ""] and s.popped == [0, 0, 0]


def test_finish_of_some_utterances_does_not_end_the_stream(stream3):
    s, calls = stream3
    s.step(torch.zeros(3, 2, 4))
    assert s.finish(only=[2]) == ["", "", "ba"] and not s.finished
    assert s.finish(decode_func=str.upper, only=[0, 1]) == ["AB", "B", ""]
    s.step(torch.zeros(3, 2, 4))                                   # does not raise
    assert s.finish() == ["ab", "b", "ba"] and s.finished
    with pytest.raises(RuntimeError, match="twice"):
        s.finish()
    with pytest.raises(RuntimeError, match="twice"):
        s.finish(only=[0])
    with pytest.raises(RuntimeError, match="after finish"):
        s.step(torch.zeros(3, 2, 4))
    assert [c[0] for c in calls] == ["step", "finish", "finish", "step", "finish"]


def test_step_passes_t_used_through(stream3):
    s, calls = stream3
    s.step(torch.zeros(3, 2, 4))
    s.step(torch.zeros(3, 2, 4), torch.tensor([2, 0, 1]), t_used=7)
    assert [kw["t_used"] for name, kw in calls if name == "step"] == [None, 7]


def test_pop_committed_of_some_utterances(monkeypatch):
    """Commit mode over a state of three commit logs (the stand-in of tests/test_ctc_beam_commit_cpu.py): utterance 1 lapped
    its ring of 20."""
    import types
    log = torch.arange(60, dtype=torch.int32).reshape(3, 20)
    state = types.SimpleNamespace(B=3, log=log, total=torch.tensor([3, 45, 23]))
    monkeypatch.setattr(decode, "beam_ctc_stream_init", lambda *a, **kw: state)
    s = decode.BeamCTCDecoder(VOCAB4, blank_id=0, beam_width=4).stream(3, None, "cpu", max_pending=4, max_chunk_frames=16)
    s.popped = [0, 0, 5]
    with pytest.raises(RuntimeError, match=r"utterance\(s\) \[1\]"):
        s.pop_committed()
    assert s.popped == [0, 0, 5]
    assert s.pop_committed(only=[0, 2]) == [[0, 1, 2], [], [40 + p % 20 for p in range(5, 23)]]
    assert s.popped == [3, 0, 23]
    assert s.pop_committed(only=[0, 2]) == [[], [], []] and s.committed_text(only=[0]) == ["", "", ""]
    s.discard_committed(only=[1])
    assert s.popped == [3, 45, 23] and s.pop_committed() == [[], [], []]
    plain = decode.BeamCTCDecoder(VOCAB4, blank_id=0, beam_width=4).stream(3, 10, "cpu")
    for call in (plain.pop_committed, plain.discard_committed, plain.committed_text):
        with pytest.raises(RuntimeError, match="without max_pending"):
            call(only=[0])
