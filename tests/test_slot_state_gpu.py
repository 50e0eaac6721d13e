"""The skeleton the four per-slot stream followers share (conformer_amd/_slot_state.py) on the MI355X: resets that touch the
slots asked for and nothing else, the three ways of giving the frame counts, and counts that differ per slot.

Every comparison is bit for bit: a slot's state depends on its own frames alone, and a reset writes constants."""
import math

import pytest
import torch

from conformer_amd.confidence import ConfidenceConfig, StreamingConfidence
from conformer_amd.endpoint import EndpointConfig, EndpointRule, StreamingEndpointer
from conformer_amd.kws import Keywords, StreamingKeywordSpotter
from conformer_amd.vad import StreamingVad, VadConfig

pytestmark = pytest.mark.gpu

S, K, V, N_MEL = 3, 5, 8, 8


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class Case:
    """One of the four classes: how to make a fresh object, every device tensor it keeps per slot (`tensors`), those a reset
    writes (`armed`: the others are dead once these say "frame 0"), and the layout of its input."""

    def __init__(self, make, tensors, armed, frames_last, takes_none):
        self.make, self.tensors, self.armed, self.frames_last, self.takes_none = make, tensors, armed, frames_last, takes_none

    def input(self, dev, seed=5):
        g = torch.Generator().manual_seed(seed)
        shape = (S, N_MEL, K) if self.frames_last else (S, K, V)
        return (torch.randn(shape, generator=g) * 3.0).to(dev)

    def cut(self, x, n, poison=None):
        """x with `n` frames per slot; poison: per slot the frames it brings, everything behind them NaN."""
        x = (x[:, :, :n] if self.frames_last else x[:, :n]).clone()
        for b, k in enumerate(poison or ()):
            if self.frames_last:
                x[b, :, k:] = math.nan
            else:
                x[b, k:] = math.nan
        return x

    def snapshot(self, obj, names=None):
        return {n: getattr(obj, n).clone() for n in (names or self.tensors)}


CASES = {
    # frame_seconds = 1: a rule of 2 s is 2 frames, so rules fire inside the 5 frames
    "endpoint": Case(lambda dev: StreamingEndpointer(S, 0, EndpointConfig([EndpointRule(2.0, 0.0, 0.0, False), EndpointRule(1.0)],
                                                                          0.3), 1.0, dev),
                     ["state"], ["state"], False, True),
    # a ring of 4 columns: the 5 frames take two launches, the second with the counts clamped to its window
    "confidence": Case(lambda dev: StreamingConfidence(S, 0, ConfidenceConfig(), 4, dev),
                       ["conf", "ids", "total"], ["conf", "ids", "total"], False, True),
    "kws": Case(lambda dev: StreamingKeywordSpotter(S, Keywords([[1, 2], [3], [4, 4]], blank_id=0, vocab_size=V, threshold=8.0),
                                                    1.0, 4, None, dev),
                ["state", "counts", "detections"], ["state", "counts"], False, True),
    "vad": Case(lambda dev: StreamingVad(S, N_MEL, VadConfig(1.0, None, 3.0, 2.0, 1.0, 1.0), 1.0, 4, dev),
                ["state", "ring", "segments"], ["state"], True, False),
}


def _same(a, b, names, slots):
    """bit for bit (NaN included): compared as bytes"""
    for n in names:
        for s in slots:
            x, y = a[n][s].contiguous().view(-1).view(torch.uint8), b[n][s].contiguous().view(-1).view(torch.uint8)
            if not torch.equal(x, y):
                return False
    return True


_FULL: dict = {}


def _full(name, dev):
    """(the input, the state after one step of K frames in every slot), made once per class and left unchanged"""
    if name not in _FULL:
        c = CASES[name]
        x = c.input(dev)
        obj = c.make(dev)
        obj.step(x, [K] * S)
        _FULL[name] = (x, c.snapshot(obj))
    return _FULL[name]


@pytest.mark.parametrize("name", list(CASES))
def test_reset_slots_touches_the_slots_asked_for_and_reset_all_of_them(dev, name):
    c = CASES[name]
    x, full = _full(name, dev)
    fresh = c.snapshot(c.make(dev))
    assert not _same(full, fresh, c.armed, range(S))                          # the step has left something to reset
    obj = c.make(dev)
    obj.step(x, [K] * S)
    before = c.snapshot(obj)
    assert _same(before, full, c.tensors, range(S))
    obj.reset_slots([])                                                       # nothing asked for, nothing done
    assert _same(c.snapshot(obj), before, c.tensors, range(S))
    obj.reset_slots([1])
    after = c.snapshot(obj)
    assert _same(after, before, c.tensors, [0, 2])
    assert _same(after, fresh, c.armed, [1])
    assert _same(after, before, [n for n in c.tensors if n not in c.armed], [1])   # (a reset writes the armed tensors alone)
    with pytest.raises(ValueError, match=r"slots \[3\] outside \[0, 3\)"):
        obj.reset_slots([3])
    assert _same(c.snapshot(obj), after, c.tensors, range(S))
    obj.reset()
    assert _same(c.snapshot(obj), fresh, c.armed, range(S))
    obj.step(x, [K] * S)                                                      # and an armed slot is a new one: the same bits again
    assert _same(c.snapshot(obj), full, c.armed, range(S))


@pytest.mark.parametrize("name", list(CASES))
def test_the_ways_of_giving_the_frame_counts_leave_the_same_bits(dev, name):
    c = CASES[name]
    x, full = _full(name, dev)                                                # (made with the host list [K] * S)
    ways = [torch.full((S,), K, dtype=torch.int64, device=dev), torch.full((S,), K, dtype=torch.int64), tuple([K] * S)]
    if c.takes_none:
        ways.append(None)
    for k in ways:
        obj = c.make(dev)
        if k is None:
            obj.step(x)
            obj.step(c.cut(x, 0))                                             # (an empty step is no step)
        else:
            obj.step(x, k)
        assert _same(c.snapshot(obj), full, c.tensors, range(S)), type(k)
    if not c.takes_none:
        with pytest.raises((TypeError, RuntimeError)):                        # the VAD has no "all of them": as before
            c.make(dev).step(x, None)
    for bad in ([K] * (S + 1), torch.full((S - 1,), K, dtype=torch.int64, device=dev)):
        with pytest.raises(ValueError, match=f"expected {S} frame counts"):
            c.make(dev).step(x, bad)


@pytest.mark.parametrize("name", list(CASES))
def test_counts_per_slot_are_honoured(dev, name):
    c = CASES[name]
    x, full = _full(name, dev)
    ks = [K, 0, 2]
    obj = c.make(dev)
    obj.step(c.cut(x, K, poison=ks), ks)                                      # what lies behind a slot's count is never read
    got = c.snapshot(obj)
    assert _same(got, full, c.tensors, [0])
    assert _same(got, c.snapshot(c.make(dev)), c.tensors, [1])
    two = c.make(dev)
    two.step(c.cut(x, 2), [2] * S)
    assert _same(got, c.snapshot(two), c.armed, [2])
    assert not _same(got, full, c.armed, [2])
