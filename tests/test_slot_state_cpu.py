"""CPU side of conformer_amd/_slot_state.py: the chunk arithmetic of frame_chunks, the open/close registry, the slot lists and
the frame-duration check that the per-slot objects share."""
import math

import pytest
import torch

from conformer_amd._slot_state import OpenSlots, SlotFollower, frame_chunks, positive_seconds

CAP = 8


@pytest.mark.parametrize("k_max", [1, 7, 8, 9, 19])
def test_frame_chunks_tile_the_step_and_split_every_count(k_max):
    k = torch.tensor([0, k_max, k_max // 2, (k_max + 1) // 2, max(0, k_max - 1), min(1, k_max)], dtype=torch.int64)
    before = k.clone()
    chunks = list(frame_chunks(k, k_max, CAP))
    covered = [t for t0, n, _ in chunks for t in range(t0, t0 + n)]
    assert covered == list(range(k_max))                                      # [0, k_max), every frame exactly once
    total = torch.zeros_like(k)
    for t0, n, kk in chunks:
        assert 1 <= n <= CAP and kk.dtype == torch.int64 and kk.shape == k.shape
        assert bool((kk >= 0).all()) and bool((kk <= n).all())
        # a slot's frames inside the window [t0, t0 + n): the count the launch of that window has to see
        assert kk.tolist() == [min(max(int(v) - t0, 0), n) for v in before]
        total += kk
    assert torch.equal(total, before) and torch.equal(k, before)              # nothing lost, and k itself is not written
    if k_max <= CAP:
        assert len(chunks) == 1 and chunks[0][2] is k                         # the identity: no device operation was added
    else:
        assert all(kk is not k for _, _, kk in chunks)


def test_frame_chunks_of_an_empty_step():
    assert list(frame_chunks(torch.zeros(3, dtype=torch.int64), 0, CAP)) == []


class _Registry(OpenSlots):
    def __init__(self, S):
        self.S = S
        self._free_all()


def test_open_slots_accepts_open_close_reopen_and_refuses_the_rest():
    r = _Registry(3)
    assert r.is_open == [False] * 3
    assert r._check_slot(1, want_open=False) == 1
    r._mark_open(1)
    assert r.is_open == [False, True, False]
    with pytest.raises(RuntimeError, match="slot 1 is already open"):
        r._check_slot(1, want_open=False)
    assert r._check_slot(1.0, want_open=True) == 1                            # (int() is applied, as before)
    r._mark_closed(1)
    with pytest.raises(RuntimeError, match="slot 1 is free"):
        r._check_slot(1, want_open=True)
    with pytest.raises(RuntimeError, match="slot 0 is free"):
        r._check_slot(0, want_open=True)
    assert r._check_slot(1, want_open=False) == 1                             # reopen
    r._mark_open(1)
    for s in (-1, 3):
        for want in (False, True):
            with pytest.raises(ValueError, match=rf"slot {s} out of range \[0, 3\)"):
                r._check_slot(s, want_open=want)
    r._mark_open(2)
    held = r.is_open
    r._free_all()
    assert r.is_open == [False] * 3 and held == [False, True, True]           # a new list, as `reset` always made one


def test_the_three_registries_use_the_one_implementation():
    from conformer_amd.resample import StreamingResampler
    from conformer_amd.slots import SlotStreamingEncoder
    from conformer_amd.stream_frontend import StreamingAudioFrontend
    for cls in (SlotStreamingEncoder, StreamingAudioFrontend, StreamingResampler):
        assert cls._check_slot is OpenSlots._check_slot and "is_open" not in vars(cls)


def test_slot_list():
    f = object.__new__(SlotFollower)
    f.S = 3
    assert f._slot_list(None) == [0, 1, 2] and f._slot_list() == [0, 1, 2]
    assert f._slot_list([2, 0, 2]) == [2, 0, 2] and f._slot_list(()) == []
    assert f._slot_list(torch.tensor([1])) == [1]
    for bad in ([3], [0, -1], [1, 7]):
        with pytest.raises(ValueError, match=r"slots \[.*\] outside \[0, 3\)"):
            f._slot_list(bad)
    with pytest.raises(ValueError) as e:
        f._slot_list([0, 5])
    assert str(e.value) == "slots [0, 5] outside [0, 3)"


def test_the_four_followers_use_the_one_skeleton():
    from conformer_amd.confidence import StreamingConfidence
    from conformer_amd.endpoint import StreamingEndpointer
    from conformer_amd.kws import StreamingKeywordSpotter
    from conformer_amd.vad import StreamingVad
    for cls in (StreamingEndpointer, StreamingConfidence, StreamingKeywordSpotter, StreamingVad):
        assert issubclass(cls, SlotFollower) and cls._what
        for name in ("reset", "reset_slots", "_slot_list", "_slot_index", "_frame_counts", "_pitches"):
            assert name not in vars(cls), (cls.__name__, name)


@pytest.mark.parametrize("name", ["frame_seconds", "mel_seconds"])
def test_positive_seconds(name):
    assert positive_seconds("Who", name, 0.04) == 0.04
    got = positive_seconds("Who", name, 1)
    assert got == 1.0 and isinstance(got, float)
    for bad in (0, 0.0, -0.01, -1, math.inf, -math.inf, math.nan, True, False, "0.04", None):
        with pytest.raises(ValueError) as e:
            positive_seconds("Who", name, bad)
        assert str(e.value) == f"Who: {name} must be a positive finite number, got {bad!r}"


def test_slot_counts_keep_each_class_s_acceptance_and_message():
    f = object.__new__(SlotFollower)
    f._init_slots("Who", 2.0, strict=False)                                   # endpointing and confidence: whatever int() takes
    assert f.S == 2 and isinstance(f.S, int)
    with pytest.raises(ValueError, match="Who: slots must be >= 1, got 0"):
        f._init_slots("Who", 0, strict=False)
    f._init_slots("Who", 65535, strict=True, max_slots=65535)                 # keyword spotting and VAD: a true int of the grid
    assert f.S == 65535
    for bad in (0, 65536, True, 2.0, "2"):
        with pytest.raises(ValueError) as e:
            f._init_slots("Who", bad, strict=True, max_slots=65535)
        assert str(e.value) == f"Who: slots must be 1 to 65535, got {bad!r}"


def test_a_cpu_device_or_input_is_refused_in_the_class_s_own_words():
    from conformer_amd import _lib

    class F(SlotFollower):
        _what = "this only exists as a gfx950 kernel"

    f = object.__new__(F)
    with pytest.raises(_lib.ConformerHipError) as e:
        f._init_device("Who", "cpu")
    assert str(e.value) == "Who: device cpu; this only exists as a gfx950 kernel (no CPU fallback)"
    with pytest.raises(_lib.ConformerHipError) as e:
        f._device_input(torch.zeros(1, 2, 3), "logits")
    assert str(e.value) == ("logits: expected a tensor on a HIP device, got cpu; this only exists as a gfx950 kernel "
                            "(no CPU fallback)")
    with pytest.raises(_lib.ConformerHipError, match="no CPU fallback"):
        f._device_input([[0.0]], "mel_chunk")
