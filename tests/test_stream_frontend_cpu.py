"""CPU side of the streaming audio front end (conformer_amd/stream_frontend.py): the host arithmetic of frame_plan over the
chunkings of the contract, the numpy restatement (tests/stream_frontend_restatement.py) against the frames of the whole
reflect-padded utterance bit for bit, and the host-side refusals, which need no device because they come before it is touched.
The device side is tests/test_stream_frontend_gpu.py."""
import numpy as np
import pytest
import torch

from tests import stream_frontend_restatement as R

N_FFT = 400
HOPS = [40, 100, 128, 160, 200, 400]
LENGTHS = [201, 202, 359, 360, 361, 400, 1000, 4959, 4960]


def wave(L, seed=0):
    return np.random.default_rng(1000 * seed + L).standard_normal(L).astype(np.float32)


def cases():
    for hop in HOPS:
        for L in LENGTHS:
            for i, chunks in enumerate(R.chunkings(L, seed=hop * 10007 + L)):
                yield hop, L, chunks, bool((i + L) & 1)


@pytest.mark.parametrize("hop", HOPS)
def test_plan_arithmetic(hop):
    """frame_plan's totals are E(n) mid-stream and L // hop + 1 at the flush, the tail stays below n_fft, p0 never moves back,
    and every value of the device row equals the restatement's."""
    from conformer_amd.stream_frontend import frame_plan, frames_so_far
    pad, worst_tail, n_cases = N_FFT // 2, 0, 0
    for h, L, chunks, with_last in cases():
        if h != hop:
            continue
        n_cases += 1
        ref = R.Stream(hop, N_FFT)
        received = emitted = p0 = 0
        steps = [(c, with_last and i == len(chunks) - 1) for i, c in enumerate(chunks)] + ([] if with_last else [(0, True)])
        for c, flush in steps:
            p = frame_plan(received, c, flush, emitted, hop, N_FFT)
            want = ref.step(np.zeros(c), flush)["row"]
            assert p.row(c, flush) == want, (hop, L, received, c, flush)
            assert p.tail_len == received - p0
            received, emitted = received + c, emitted + p.frames
            assert p.frames >= 0
            if flush:
                assert emitted == L // hop + 1 and p.new_tail_len == 0
            else:
                assert emitted == frames_so_far(received, hop, N_FFT) == (0 if received <= pad else (received - pad) // hop + 1)
                assert p.new_tail_len <= N_FFT - 1
                assert received - p.new_tail_len >= p0
                p0 = received - p.new_tail_len
                worst_tail = max(worst_tail, p.new_tail_len)
                # a later flush can reflect: the pad + 1 last samples are still there
                assert p.new_tail_len >= min(received, pad + 1)
        assert received == L
    assert n_cases >= 3 * len(LENGTHS) and 0 < worst_tail <= N_FFT - 1


@pytest.mark.parametrize("hop", HOPS)
def test_segments_are_the_offline_frames_bit_for_bit(hop):
    n = 0
    for h, L, chunks, with_last in cases():
        if h != hop:
            continue
        x = wave(L)
        got, steps = R.run_stream(x, chunks, with_last, hop, N_FFT, np.float32)
        want = R.offline_frames(x, hop, N_FFT)
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (L // hop + 1, N_FFT), (hop, L, chunks)
        assert np.array_equal(got, want), (hop, L, chunks)
        assert max(len(s["tail_out"]) for s in steps) <= N_FFT - 1
        n += 1
    assert n >= 3 * len(LENGTHS)


@pytest.mark.parametrize("L,chunks,with_last", [
    (361, [1] * 361, True),                     # one sample per step
    (361, [1] * 361, False),
    (201, [201], True),                         # both reflections in one frame
    (400, [200, 200], False),                   # nothing until the empty flush step, which emits all three frames
    (4960, [5000], True),
], ids=["ones_flush_with_last", "ones_empty_flush", "L201_one_step", "L400_empty_flush", "one_chunk"])
def test_named_streams(L, chunks, with_last):
    chunks = [min(c, L) for c in chunks]
    x = wave(L, 1)
    got, steps = R.run_stream(x, chunks, with_last)
    assert np.array_equal(got, R.offline_frames(x.astype(np.float64), 160, N_FFT))
    if L == 201:
        (s,) = steps
        assert s["row"] == (0, 201, 200, 2, 1, 0, 201, 0)
        f0 = s["frames"][0]
        assert np.array_equal(f0[:200], x[200:0:-1]) and np.array_equal(f0[200:], x[:200])      # x[200] .. x[1] | x[0] .. x[199]
        f1 = s["frames"][1]                                              # virtual -40 .. 359: 40 reflected, 201 samples, 159 reflected
        assert np.array_equal(f1[:40], x[40:0:-1]) and np.array_equal(f1[40:241], x) and np.array_equal(f1[241:], x[199:40:-1])
    if L == 400 and not with_last:
        assert [s["row"][3] for s in steps] == [0, 2, 1]                 # E(200) = 0, E(400) = 2, the flush adds frame 2
        assert steps[1]["row"][2] == 200 and steps[2]["row"][:2] == (280, 0)           # the tail from p0 = 2 hop - pad on


def test_restatement_agrees_with_the_float64_oracle_frames():
    """The frames the end-to-end reference (oracle.frontend_oracle.log_mel_numpy64) is built on are the restatement's."""
    from oracle import frontend_oracle as FO
    x = wave(1000, 2)
    frames, _ = FO._frames_and_basis(x[None], 160)
    got, _ = R.run_stream(x, [7, 201, 0, 160, 632], False)
    assert np.array_equal(got, frames[0])


def _front_end(hop=160, slots=3, max_chunk=640):
    from conformer_amd.frontend import ConformerAudioFrontend
    from conformer_amd.stream_frontend import StreamingAudioFrontend
    return StreamingAudioFrontend(ConformerAudioFrontend(hop_length=hop, device="cpu"), slots, max_chunk)


@pytest.mark.parametrize("hop", [150, 161, 2, 404])
def test_unsupported_hops_are_refused_at_construction(hop):
    with pytest.raises(NotImplementedError):
        _front_end(hop)


def test_host_refusals_raise_before_the_device_and_change_nothing():
    from conformer_amd._lib import ConformerHipError
    from conformer_amd.stream_frontend import frame_plan
    fe = _front_end()
    fe.open(0)
    fe.open(2)
    fe.received[0], fe.emitted[0] = 1000, 6                             # (as after 1000 samples)
    before = (list(fe.is_open), list(fe.received), list(fe.emitted))
    z = torch.zeros(3, 640)
    for exc, args in [
        (RuntimeError, (z, [10, 5, 0])),                                # samples for free slot 1
        (RuntimeError, (z, [10, 0, 0], [1])),                           # flush of a free slot
        (ValueError, (z, [10, 0, 0], [3])),                             # no such slot
        (ValueError, (torch.zeros(3, 641), [641, 0, 0])),               # above max_chunk_samples
        (ValueError, (z, [641, 0, 0])),                                 # more than the tensor holds
        (ValueError, (z, [-1, 0, 0])),
        (ValueError, (z, [10, 0])),                                     # two counts for three slots
        (ValueError, (torch.zeros(2, 640), [10, 0, 0])),
        (ValueError, (z, [0, 0, 200], [2])),                            # a flush with L = 200 <= pad
        (ValueError, (z, [0, 0, 0], [2])),                              # ... and with L = 0
    ]:
        with pytest.raises(exc):
            fe.step(*args)
        assert (fe.is_open, fe.received, fe.emitted) == before, args
    with pytest.raises(RuntimeError):
        fe.open(0)
    with pytest.raises(RuntimeError):
        fe.close(1)
    with pytest.raises(ValueError):
        fe.open(3)
    with pytest.raises(ValueError):
        frame_plan(150, 50, True, 0, 160, N_FFT)
    assert frame_plan(150, 51, True, 0, 160, N_FFT).frames == 2
    # a valid step of host tensors gets past every check above and stops at the device check: there is no CPU path
    with pytest.raises(ConformerHipError):
        fe.step(z, [10, 0, 0])
    assert (fe.is_open, fe.received, fe.emitted) == before
    fe.close(2)
    fe.reset()
    assert fe.is_open == [False] * 3


def test_the_entry_is_bound_from_its_own_header():
    """what every header shares (record, names, binding, rebuild message, build) is asserted in test_abi_binding_cpu"""
    from conformer_amd import _lib
    header = _lib.HEADERS["conformer_hip_stream_frontend.h"]
    assert set(header.signatures) == {"cfm_stream_stage_f32"}
    assert _lib.PARAMS["cfm_stream_stage_f32"] == header.params["cfm_stream_stage_f32"] == [
        "samples", "ld_samples", "n_max", "tail_in", "tail_out", "table", "xp", "S", "f_max", "hop", "n_fft", "stream"]
    assert "cfm_stream_stage_f32" not in _lib.SIGNATURES
