"""Host-side checks of the committed-prefix streaming search: the float64 restatement against the one-shot restatement, the
extension header and its binding, the size of the commit state, argument validation of the new C entries (it happens before
any HIP call, so it runs without a GPU) and the Python refusals."""
import ctypes
import os

import numpy as np
import pytest

from conformer_amd import _lib, build, decode
from tests import ctc_beam_commit_restatement as CR
from tests import ctc_beam_restatement as R

OK, BAD_SHAPE, UNSUPPORTED, NULL = 0, -1, -2, -3
CHUNKS = [1, 7, 3, 16, 2, 11, 5, 15]
NAMES = {"cfm_ctc_beam_commit_state_bytes", "cfm_ctc_beam_stream_commit", "cfm_ctc_beam_commit_reset_slots"}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def buf():
    """a 16-byte aligned host address with room for every pointer argument (nothing is launched, nothing dereferenced)"""
    raw = (ctypes.c_char * 4096)()
    a = ctypes.addressof(raw)
    return raw, (a + 15) // 16 * 16


def logits(seed, T=60, V=7):
    return (3 * np.random.default_rng(seed).normal(size=(T, V))).astype(np.float32)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_restatement_without_forcing_is_the_one_shot_search(seed):
    x = logits(seed)
    kw = dict(beam_width=8, max_candidates=4)
    one, _ = R.beam_search(x, 0, n_best=8, **kw)
    plain, cs, _ = CR.commit_search(x, CHUNKS, 0, None, n_best=8, **kw)
    assert plain == one and cs.C == () and cs.forced == cs.natural == cs.dropped == 0
    big, cs, steps = CR.commit_search(x, CHUNKS, 0, 10 ** 6, n_best=8, **kw)
    assert big == one and cs.dropped == 0 and cs.forced == 0
    assert len(cs.C) > 0 and cs.natural > 0                       # the commit is not vacuous: text became final on the way
    for seq, _ in big:
        assert seq[:len(cs.C)] == cs.C
    assert all(len(s) <= 8 for _, s in steps)


@pytest.mark.parametrize("M", [1, 2, 4, 8])
def test_committed_prefix_is_monotone_and_pending_is_bounded(M):
    forced = dropped = 0
    for seed in range(4):
        final, cs, steps = CR.commit_search(logits(seed), CHUNKS, 0, M, beam_width=8, max_candidates=4)
        prev = ()
        for C, surv in steps:
            assert C[:len(prev)] == prev
            prev = C
            assert 1 <= len(surv) <= 8 and all(len(seq) <= M for seq, _ in surv)
        assert final[0][0][:len(prev)] == prev and len(final[0][0]) - len(prev) <= M
        forced += cs.forced
        dropped += cs.dropped
    assert forced >= 3 and dropped >= 10


def test_forced_commits_depend_on_the_chunking():
    x = logits(0)
    a, _, _ = CR.commit_search(x, CHUNKS, 0, 1, beam_width=8, max_candidates=4)
    b, _, _ = CR.commit_search(x, [60], 0, 1, beam_width=8, max_candidates=4)
    one, _ = R.beam_search(x, 0, 8, max_candidates=4)
    assert b[0][0] == one[0][0]          # one step: the commit comes after the last frame and changes nothing the finish returns
    assert a[0][0] != one[0][0]


# ---- header and binding ------------------------------------------------------------------------------------------------------
def test_commit_header_is_bound_from_its_own_table(lib):
    """what every header shares (record, names, binding, rebuild message, build) is asserted in test_abi_binding_cpu"""
    sigs = _lib.HEADERS["conformer_hip_commit.h"].signatures
    assert set(sigs) == NAMES and not NAMES & set(_lib.SIGNATURES) and len(_lib.SIGNATURES) == 144
    assert sigs["cfm_ctc_beam_commit_state_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 7)
    assert _lib.ABI_VERSION == 4 and lib.cfm_abi_version() == 4            # nothing existing moved
    with pytest.raises(_lib.ConformerHipError, match="argument 2 .`max_pending`."):
        _lib.call("cfm_ctc_beam_stream_commit", 1, "x", 1, 1, 1, 0, 0, None, None, 0, None, 0, None, None, None)


# ---- the state size ----------------------------------------------------------------------------------------------------------
def test_commit_state_bytes(lib):
    f = lib.cfm_ctc_beam_commit_state_bytes
    base = dict(B=3, M=8, k=16, W=16, K=8)
    for lm in (0, 1):
        for hw in (0, 1):
            for name, values in (("B", (1, 2, 3, 64)), ("M", (1, 2, 8, 64, 1000)), ("k", (1, 2, 16, 160)),
                                 ("W", (1, 2, 16, 100, 256)), ("K", (1, 8, 32))):
                sizes = [f(*{**base, name: v}.values(), lm, hw) for v in values]
                assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes), (name, sizes)
            assert f(3, 8, 16, 16, 8, 0, 0) <= f(3, 8, 16, 16, 8, lm, hw) <= f(3, 8, 16, 16, 8, 1, 1)
            # the stream state of the tree's M + k_cap frames, and the scratch behind it
            assert f(3, 8, 16, 16, 8, lm, hw) > lib.cfm_ctc_beam_stream_state_bytes(3, 24, 16, 8, lm, hw)
    for args in ((0, 8, 16, 4, 4), (2, 0, 16, 4, 4), (2, 8, 0, 4, 4), (2, 8, 16, 0, 4), (2, 8, 16, 257, 4), (2, 8, 16, 4, 0),
                 (2, 8, 16, 4, 33), (2, 1 << 23, 16, 256, 4), (2, 2 ** 31 - 8, 16, 1, 4)):
        assert f(*args, 0, 0) == 0 and f(*args, 1, 1) == 0
    # nothing in it is a stream length: cfg-5's search (W = 100, K = 16, 160 frames per step) at max_pending = 64 stays far
    # below the state of a 20000-mel-frame stream (4999 frames), which the plain stream state grows with
    cfg5 = f(1, 64, 160, 100, 16, 0, 0)
    assert _lib.PARAMS["cfm_ctc_beam_commit_state_bytes"] == ["B", "max_pending", "max_chunk_frames", "W", "K", "lm", "hw"]
    assert 10 * cfg5 < lib.cfm_ctc_beam_stream_state_bytes(1, 4999, 100, 16, 0, 0)
    assert lib.cfm_ctc_beam_stream_state_bytes(1, 9999, 100, 16, 0, 0) > lib.cfm_ctc_beam_stream_state_bytes(1, 4999, 100, 16, 0, 0)


# ---- argument validation before any launch -----------------------------------------------------------------------------------
def _commit(lib, p, **kw):
    a = dict(B=2, M=4, k=16, W=4, K=4, lm=0, hw=0, lengths=None, state=p, state_bytes=1 << 40, log=p, L=20, total=p,
             committed=None, stream=None)
    a.update(kw)
    return lib.cfm_ctc_beam_stream_commit(*a.values())


def test_commit_rejects_bad_arguments_before_any_launch(lib, buf):
    _, p = buf
    for name in ("state", "log", "total"):
        assert _commit(lib, p, **{name: None}) == NULL, name
    assert _commit(lib, p, B=0) == BAD_SHAPE
    assert _commit(lib, p, M=0) == BAD_SHAPE and _commit(lib, p, M=-3) == BAD_SHAPE
    assert _commit(lib, p, k=0) == BAD_SHAPE
    assert _commit(lib, p, W=0) == UNSUPPORTED and _commit(lib, p, W=257) == UNSUPPORTED
    assert _commit(lib, p, K=0) == UNSUPPORTED and _commit(lib, p, K=33) == UNSUPPORTED
    assert _commit(lib, p, M=1 << 30, L=2 ** 31 - 1, W=256) == UNSUPPORTED            # T_tree * W past int32
    assert _commit(lib, p, M=2 ** 31 - 1, k=2 ** 31 - 1) == UNSUPPORTED               # M + k_cap itself
    assert _commit(lib, p, L=19) == BAD_SHAPE and _commit(lib, p, L=0) == BAD_SHAPE   # a call could lap the ring
    need = lib.cfm_ctc_beam_commit_state_bytes(2, 4, 16, 4, 4, 0, 0)
    assert _commit(lib, p, state_bytes=need - 1) == BAD_SHAPE
    # a buffer of the stream state alone (no scratch), and the plain state where the LM state is needed
    assert _commit(lib, p, state_bytes=lib.cfm_ctc_beam_stream_state_bytes(2, 20, 4, 4, 0, 0)) == BAD_SHAPE
    assert _commit(lib, p, state_bytes=need, lm=1) == BAD_SHAPE and _commit(lib, p, state_bytes=need, hw=1) == BAD_SHAPE


def test_commit_reset_slots_rejects_bad_arguments_before_any_launch(lib, buf):
    _, p = buf
    f = lib.cfm_ctc_beam_commit_reset_slots
    assert f(2, None, 1, p, None) == NULL and f(2, p, 1, None, None) == NULL
    assert f(0, p, 1, p, None) == BAD_SHAPE and f(2, p, 0, p, None) == BAD_SHAPE and f(2, p, 3, p, None) == BAD_SHAPE


# ---- Python refusals (raised before the model, the decoder or a device is used) -----------------------------------------------
def test_python_refusals():
    from conformer_amd.slots import SlotTranscriber
    from conformer_amd.transcribe import StreamingTranscriber
    init = decode.beam_ctc_stream_init
    with pytest.raises(ValueError, match="max_chunk_frames"):
        init(2, None, "cpu", max_pending=4)
    with pytest.raises(ValueError, match="max_pending"):
        init(2, None, "cpu", max_chunk_frames=16)
    with pytest.raises(ValueError, match="max_frames"):
        init(2, 100, "cpu", max_pending=4, max_chunk_frames=16)
    with pytest.raises(ValueError, match="max_pending"):
        init(2, None, "cpu")
    with pytest.raises(ValueError, match=">= 1"):
        init(2, None, "cpu", max_pending=0, max_chunk_frames=16)
    with pytest.raises(ValueError, match=">= 1"):
        init(2, None, "cpu", max_pending=4, max_chunk_frames=0)
    dec = decode.BeamCTCDecoder(["_", "a", "b", "|"], blank_id=0, beam_width=4)
    with pytest.raises(ValueError, match="max_chunk_frames"):
        dec.stream(2, None, "cpu", max_pending=4)
    with pytest.raises(ValueError, match="max_frames"):
        dec.stream(2, 50, "cpu", max_pending=4, max_chunk_frames=16)
    for cls in (StreamingTranscriber, SlotTranscriber):
        with pytest.raises(ValueError, match="max_pending"):                 # no end, bounded history, but an unbounded search
            cls(None, None, 2, None, left_context=8, max_chunk_mel_frames=64)
        with pytest.raises(ValueError, match="left_context"):
            cls(None, None, 2, None)
        with pytest.raises(ValueError, match="left_context"):                # k_cap is the windowed stream's
            cls(None, None, 2, 4000, max_pending=4)
        with pytest.raises(ValueError, match="left_context"):
            cls(None, None, 2, None, max_pending=4)
        with pytest.raises(ValueError, match=">= 1"):
            cls(None, None, 2, None, left_context=8, max_chunk_mel_frames=64, max_pending=0)



# ---- reading the commit log (host logic; the state's tensors stand in on the CPU) -------------------------------------------------
def _log_state(totals, L=20):
    import types

    import torch
    log = torch.arange(len(totals) * L, dtype=torch.int32).reshape(len(totals), L)
    return types.SimpleNamespace(B=len(totals), log=log, total=torch.tensor(totals, dtype=torch.int64))


def test_committed_reads_only_the_utterances_asked_for():
    st = _log_state([3, 45, 23])                                   # utterance 1 lapped its ring of 20 since position 0
    with pytest.raises(RuntimeError, match=r"utterance\(s\) \[1\]"):
        decode.beam_ctc_stream_committed(st, [0, 0, 5])
    ids, total = decode.beam_ctc_stream_committed(st, [0, 0, 5], only=[0, 2])
    assert total == [3, 45, 23] and ids[1] == []
    assert ids[0] == [0, 1, 2] and ids[2] == [40 + p % 20 for p in range(5, 23)]          # the ring wraps at 20
    assert decode.beam_ctc_stream_committed(st, [0, 30, 23], only=[1])[0][1] == [20 + p % 20 for p in range(30, 45)]
    assert decode.beam_ctc_stream_committed(st, [0, 0, 0], only=[])[0] == [[], [], []]


def test_a_lapped_slot_raises_for_itself_alone_and_close_still_frees_it(monkeypatch):
    import torch

    from conformer_amd import slots

    class Enc:
        is_open = [True, True]

        def _check_slot(self, s, want_open):
            assert self.is_open[s] == want_open
            return s

        def close(self, s):
            self.is_open[s] = False

    reset = []
    monkeypatch.setattr(decode, "beam_ctc_stream_init", lambda *a, **kw: _log_state([3, 45]))
    monkeypatch.setattr(decode, "beam_ctc_stream_reset_slots", lambda st, idx: reset.extend(idx.tolist()))
    dec = decode.BeamCTCDecoder(["_", "a", "b", "|"] + ["c"] * 36, blank_id=0, beam_width=4)
    tr = object.__new__(slots.SlotTranscriber)
    tr.S, tr.encoder = 2, Enc()
    tr.beam = dec.stream(2, None, "cpu", max_pending=4, max_chunk_frames=16)
    assert isinstance(tr.beam, decode.BeamCTCStream)
    tokens = torch.tensor([[[1, 2, -1]], [[2, -1, -1]]])
    monkeypatch.setattr(decode, "beam_ctc_stream_finish", lambda st, n_best=1: (tokens, torch.tensor([[2], [1]]), None, None, None))
    with pytest.raises(RuntimeError, match=r"utterance\(s\) \[1\]"):
        tr.pop_committed()
    assert tr.beam.popped == [0, 0]                                # nothing popped
    tr.discard_committed(1)                                        # the way out that keeps the slot open
    assert tr.beam.popped == [0, 45] and tr.pop_committed() == {0: [0, 1, 2], 1: []}
    tr.beam.popped = [0, 0]
    assert tr.close(0) == dec.text([0, 1, 2, 1, 2]) and reset == [0]              # slot 0 is not held up by slot 1
    with pytest.raises(RuntimeError, match=r"utterance\(s\) \[1\]"):
        tr.close(1)
    assert reset == [0, 1] and tr.encoder.is_open == [False, False]               # freed all the same
