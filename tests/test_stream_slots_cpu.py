"""Independent streams (conformer_amd/slots.py), CPU side: the new C entries refuse bad arguments before any HIP call, and the
host bookkeeping of a step (per-slot encoder frames and mel tails) reproduces streaming.chunk_ends on random schedules."""
import ctypes
import os
import random

import pytest

from conformer_amd.slots import slot_plan
from conformer_amd.streaming import chunk_ends

OK = 0


@pytest.fixture(scope="module")
def lib():
    from conformer_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


_BUF = (ctypes.c_float * 4096)()                              # host memory the refused calls never touch


@pytest.fixture(scope="module")
def ptr():
    return (ctypes.addressof(_BUF) + 15) // 16 * 16


def _slots_call(lib, p, **kw):
    a = dict(q=p, k=p, v=p, ld=3 * 64, pos=p, ldp=64, u=p, vb=p, qb=p, qc=p, lengths=p, ctx=p, ldo=64, B=2, T=100, H=4, dh=16,
             q_max=8, nsplit=1, ws=None)
    a.update(kw)
    return lib.cfm_relpos_attention_slots_f32(a["q"], a["k"], a["v"], a["ld"], a["pos"], a["ldp"], a["u"], a["vb"], a["qb"],
                                              a["qc"], a["lengths"], a["ctx"], a["ldo"], a["B"], a["T"], a["H"], a["dh"],
                                              a["q_max"], a["nsplit"], a["ws"], None)


def test_attention_slots_validates_without_gpu(lib, ptr):
    p = ptr
    for name in ("q", "pos", "qb", "qc", "lengths", "ctx"):
        assert _slots_call(lib, p, **{name: None}) == -3, name                   # NULL
    assert _slots_call(lib, p, q_max=0) == -1                                    # q_max < 1
    assert _slots_call(lib, p, q_max=101) == -1                                  # q_max > T
    assert _slots_call(lib, p, nsplit=0) == -1                                   # nsplit out of range
    assert _slots_call(lib, p, nsplit=17, ws=p) == -1
    assert _slots_call(lib, p, nsplit=2, ws=None) == -1                          # key split without a workspace
    assert _slots_call(lib, p, nsplit=2, ws=p, ldo=68) == -1                     # key split needs ldo == H*dh
    assert _slots_call(lib, p, dh=18, ldo=72, ld=216) == -1                      # dh % 4
    assert _slots_call(lib, p, dh=68, H=1, ldo=68, ld=204) == -2                 # dh > 64
    assert _slots_call(lib, p, ldo=60) == -1                                     # ldo < H*dh
    assert _slots_call(lib, p, B=0) == -1
    assert _slots_call(lib, p, q=p + 4) == -6                                    # misaligned


def test_beam_reset_slots_validates_without_gpu(lib, ptr):
    p = ptr
    nbytes = lib.cfm_ctc_beam_stream_state_bytes(4, 50, 8, 4, 0, 0)
    assert nbytes > 0

    def call(B=4, T=50, W=8, K=4, slots=p, n=1, state=p, size=nbytes):
        return lib.cfm_ctc_beam_stream_reset_slots(B, T, W, K, None, 1, None, slots, n, state, size, None)
    assert call(slots=None) == -3 and call(state=None) == -3
    assert call(n=0) == -1 and call(n=5) == -1                                   # 1 <= n_slots <= B
    assert call(size=nbytes - 1) == -1                                           # buffer too small
    assert call(W=0) == -2 and call(K=0) == -2
    assert call(B=0) == -1


def test_slot_plan_is_chunk_ends():
    """Per slot, the k of each step summed up are the encoder-frame boundaries of chunk_ends over that slot's own chunking,
    and the tail is what is left of the buffered frames (0..6)."""
    rng = random.Random(7)
    for trial in range(200):
        S = rng.randint(1, 6)
        chunks = [[] for _ in range(S)]
        tails, got = [0] * S, [0] * S
        for _ in range(rng.randint(1, 12)):
            frames = [rng.choice([0, 0, 1, 3, 6, 7, rng.randint(0, 200)]) for _ in range(S)]
            ks, tails2 = slot_plan(tails, frames)
            for b in range(S):
                assert 0 <= tails2[b] <= 6
                assert tails2[b] == tails[b] + frames[b] - 4 * ks[b]
                if frames[b]:
                    chunks[b].append(frames[b])
                got[b] += ks[b]
            tails = tails2
        for b in range(S):
            T = sum(chunks[b])
            ends = chunk_ends(T, chunks[b])
            assert got[b] == (ends[-1] if ends else 0) == max(0, ((T - 1) // 2 - 1) // 2), (trial, b)


def test_slot_plan_matches_streaming_step_rule():
    # a slot that only buffers (< 7 frames) produces nothing until the 7th frame arrives
    ks, tails = slot_plan([0, 0, 6, 3], [6, 7, 1, 640])
    assert ks == [0, 1, 1, 160] and tails == [6, 3, 3, 3]
