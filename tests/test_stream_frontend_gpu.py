"""The streaming audio front end (conformer_amd/stream_frontend.py) on the MI355X.

Pinned here: cfm_stream_stage_f32 against the numpy restatement bit for bit (every float of every pitch, the slack and the tails
written, nothing behind them), its clamping of a corrupt table and its refusals; whole streams under staggered opens, slot
reuse, zero-count steps and both kinds of flush against the float64 log-mel of each utterance ALONE at the offline front end's
end-to-end bound; neighbour independence; SlotTranscriber.step_audio and StreamingTranscriber.step_audio against step() fed by
a second front end; and the refusals, which leave the state as it was.

Streams are rows of the offline end-to-end cases' noise (tests/test_frontend_cpu.py asserts that no reference element of those
waves sits at the floor); the restatement and the CPU half of these tests are tests/stream_frontend_restatement.py and
tests/test_stream_frontend_cpu.py.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import conformer_oracle as O
from oracle import frontend_oracle as FO
from tests import stream_frontend_restatement as R
from tests import test_frontend_cpu as C
from tests.test_frontend_stages_gpu import carved, e2e_check, status
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
OK, BAD_SHAPE, UNSUPPORTED, NULL, ALIGN = 0, -1, -2, -3, -6
HOP, N_FFT = 160, 400
VOCAB = ["<pad>"] + [chr(ord("a") + i) for i in range(14)] + ["|", "<unk>"]
UNK = 16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conformer_amd import _lib
    assert _lib.load().cfm_device_check() == 0, "not a gfx950 device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def utterance(name, row):
    """(float32 samples, the float64 log-mel (80, L // hop + 1) of that stream alone): computed once, shared, never changed."""
    L = int(name[1:])
    w = C.e2e_wave(name, 3, L)[row].numpy()
    ref = FO.log_mel_numpy64(w[None])[0]
    ref.setflags(write=False)
    return w, ref


def front_end(dev, slots, max_chunk):
    from conformer_amd.frontend import ConformerAudioFrontend
    from conformer_amd.stream_frontend import StreamingAudioFrontend
    return StreamingAudioFrontend(ConformerAudioFrontend(device=dev), slots, max_chunk)


# ---- 1. the staging kernel ---------------------------------------------------------------------------------------------------
def stage(dev, samples, tail_in, table, S, f_max, n_max=None, hop=HOP):
    """One cfm_stream_stage_f32 launch into NaN-filled carved buffers: (xp, tail_out) on the host, bands checked."""
    from conformer_amd import _lib, ops
    pitch = (f_max + (N_FFT + hop - 1) // hop) * hop
    xp, xband = carved(S * pitch + N_FFT, dev)
    tails, tband = carved(S * R.TAIL_LD, dev)
    sd, td = torch.from_numpy(samples).to(dev), torch.from_numpy(tail_in).to(dev)
    tab = torch.from_numpy(table).to(dev)
    _lib.call("cfm_stream_stage_f32", sd.data_ptr(), sd.shape[1], sd.shape[1] if n_max is None else n_max, td.data_ptr(),
              tails.data_ptr(), tab.data_ptr(), xp.data_ptr(), S, f_max, hop, N_FFT, ops._stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(xband).all()) and bool(torch.isnan(tband).all()), "a write behind the end of xp or of the tails"
    return xp.cpu().numpy(), tails.view(S, R.TAIL_LD).cpu().numpy()


@pytest.mark.parametrize("hop", [160, 40, 200, 400])
def test_staging_bit_exact(dev, hop):
    """At hop 160 one row each: lead 200, lead 40, lead 0, a flush with 1 frame, a flush with 2 frames (and the lead), 0 new
    samples, a free slot, and a 201-sample stream flushed in its first step (both reflections in one frame).  The same streams
    at the smallest hop, at hop = n_fft - pad (from where the tail is held by the pad + 1 samples a flush reflects) and at
    hop = n_fft."""
    # (samples fed before the step, the step's samples, flush)
    rows = [(0, 500, False), (250, 400, False), (1000, 700, False), (390, 10, True), (300, 20, True), (777, 0, False), None,
            (0, 201, True)]
    S, N = len(rows), 700
    rng = np.random.default_rng(11)
    samples = rng.standard_normal((S, N)).astype(np.float32)              # (columns behind a slot's count: noise, never read)
    tail_in = np.full((S, R.TAIL_LD), 9.0, np.float32)                    # (floats behind a slot's tail length: never read)
    steps = []
    for b, r in enumerate(rows):
        if r is None:
            steps.append(None)
            continue
        before, n_new, flush = r
        st = R.Stream(hop, N_FFT, np.float32)
        st.step(rng.standard_normal(before).astype(np.float32))
        tail_in[b, :len(st.tail)] = st.tail
        steps.append(st.step(samples[b, :n_new], flush))
    f_max = max(s["row"][3] for s in steps if s is not None)
    want_xp, want_tails, table = R.staged(steps, f_max, hop, N_FFT)
    if hop == 160:
        assert [tuple(t[2:5]) for t in table] == [(200, 2, 0), (40, 2, 0), (0, 4, 0), (0, 1, 1), (40, 2, 1), (0, 0, 0), (0, 0, 0),
                                                  (200, 2, 1)]
    assert table[5][0] == table[5][7] > 0 and table[5][6] == 0            # 0 new samples: the tail goes across unchanged
    xp, tails = stage(dev, samples, tail_in, table, S, f_max, hop=hop)
    assert np.isfinite(xp).all() and np.isfinite(tails).all(), "a float of a pitch, the slack or a tail row was never written"
    assert np.array_equal(xp, want_xp)
    assert np.array_equal(tails, want_tails)
    assert np.array_equal(tails[5, :table[5][0]], tail_in[5, :table[5][0]]) and not tails[6].any() and not tails[3].any()


def test_staging_clamps_a_corrupt_table(dev):
    """Table values out of range are clamped before they index anything: the launch stays inside its buffers (bands untouched,
    everything written and finite) and the rows that are in range come out as without the neighbours' junk."""
    S, N, f_max = 6, 320, 3
    rng = np.random.default_rng(12)
    samples = rng.standard_normal((S, N)).astype(np.float32)
    tail_in = rng.standard_normal((S, R.TAIL_LD)).astype(np.float32)
    st = R.Stream(HOP, N_FFT, np.float32)
    st.step(tail_in[0, :300].copy())                                       # E = 1, the tail is all 300 samples
    assert len(st.tail) == 300 and np.array_equal(st.tail, tail_in[0, :300])
    good = st.step(samples[0], False)
    big = 1 << 30
    table = np.array([good["row"],
                      (big, big, big, big, 0, big, big, big),
                      (-5, -5, -5, -5, -5, -5, -5, -5),
                      (0, 0, 0, 3, 1, 0, 0, 0),                           # frames asked of an empty slot
                      (512, N, 0, big, 1, 512, -big, big),
                      (100, 10, 400, 3, 0, 0, 200, 512)], np.int32)
    xp, tails = stage(dev, samples, tail_in, table, S, f_max)
    assert np.isfinite(xp).all() and np.isfinite(tails).all()
    pitch = (f_max + 3) * HOP
    want = np.zeros(pitch, np.float32)
    want[:len(good["segment"])] = good["segment"]
    assert np.array_equal(xp[:pitch], want) and np.array_equal(tails[0, :len(good["tail_out"])], good["tail_out"])
    assert not xp[2 * pitch:4 * pitch].any() and not tails[2].any() and not tails[3].any() and not xp[S * pitch:].any()


def test_stage_refusals(dev):
    S, N, f_max = 2, 64, 2
    smp = torch.zeros(S * N, device=dev)
    tin, tab = torch.zeros(S * 512, device=dev), torch.zeros(S * 8, device=dev, dtype=torch.int32)
    xp, xband = carved(S * 5 * 160 + 400, dev)
    tout, tband = carved(S * 512, dev)
    s, i, o, t, x = smp.data_ptr(), tin.data_ptr(), tout.data_ptr(), tab.data_ptr(), xp.data_ptr()
    name = "cfm_stream_stage_f32"
    assert status(name, None, N, N, i, o, t, x, S, f_max, 160, 400) == NULL
    assert status(name, s, N, N, None, o, t, x, S, f_max, 160, 400) == NULL
    assert status(name, s, N, N, i, None, t, x, S, f_max, 160, 400) == NULL
    assert status(name, s, N, N, i, o, None, x, S, f_max, 160, 400) == NULL
    assert status(name, s, N, N, i, o, t, None, S, f_max, 160, 400) == NULL
    assert status(name, s, N, N, i, o, t, x + 4, S, f_max, 160, 400) == ALIGN
    assert status(name, s, N, N, i, o, t, x, 0, f_max, 160, 400) == BAD_SHAPE
    assert status(name, s, N, N, i, o, t, x, -1, f_max, 160, 400) == BAD_SHAPE
    assert status(name, s, N, N, i, o, t, x, S, f_max, 150, 400) == BAD_SHAPE           # hop % 4
    assert status(name, s, N, N, i, o, t, x, S, f_max, 404, 400) == BAD_SHAPE           # hop > n_fft
    assert status(name, s, N, N, i, o, t, x, S, f_max, 0, 400) == BAD_SHAPE
    assert status(name, s, N, N, i, o, t, x, S, -1, 160, 400) == BAD_SHAPE
    assert status(name, s, N - 1, N, i, o, t, x, S, f_max, 160, 400) == BAD_SHAPE       # ld_samples < n_max
    assert status(name, s, N, -1, i, o, t, x, S, f_max, 160, 400) == BAD_SHAPE
    assert status(name, s, N, N, i, o, t, x, S, f_max, 160, 516) == UNSUPPORTED         # a tail row holds 512 floats
    assert status(name, s, N, N, i, i, t, x, S, f_max, 160, 400) == UNSUPPORTED         # the tails in place
    assert status(name, s, N, N, i, i + 4 * 512, t, x, S, f_max, 160, 400) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(xp).all()) and bool(torch.isnan(tout).all())                # the refused calls wrote nothing
    assert status(name, s, N, N, i, o, t, x, S, f_max, 160, 400) == OK
    assert status(name, None, 0, 0, i, o, t, x, S, f_max, 160, 400) == OK               # no samples at all: null is allowed
    torch.cuda.synchronize()
    assert not xp.any() and not tout.any() and bool(torch.isnan(xband).all()) and bool(torch.isnan(tband).all())


# ---- 2. whole streams ----------------------------------------------------------------------------------------------------------
UTTS = [("L10400", 0), ("L201", 0), ("L4960", 0), ("L400", 0), ("L5120", 1), ("L400", 1)]
# every step: closes (slot list), then opens ({slot: utterance}), the samples each slot takes, the slots flushed with the step
SCHEDULE = [
    dict(open={0: 0, 1: 1, 3: 3}, samples={0: 1, 1: 201, 3: 200}, flush=[1]),      # L = 201 in one step, flushed with it
    dict(open={2: 5}, samples={0: 159, 2: 300, 3: 200}),                           # slot 2: a stream that is dropped below
    dict(samples={0: 160, 3: 0}, flush=[3]),                                       # L = 400: a flush with no samples
    dict(close=[2], open={1: 4, 2: 2, 3: 5}, samples={0: 161, 1: 0, 2: 201, 3: 400}),   # slots 1, 2, 3 reused
    dict(samples={0: 5600, 1: 640, 2: 1}, flush=[3]),                              # 35 frames: past the mel kernel's 32-frame tile
    dict(samples={0: 0, 1: 4480, 2: 4758}, flush=[1]),
    dict(samples={}),                                                              # nobody brings anything
    dict(samples={0: 4319, 2: 0}, flush=[0, 2]),
]


def drive(fe, S, schedule, dev, seed=0):
    """Run a schedule on a StreamingAudioFrontend: {utterance: its frames (80, T) concatenated} and {utterance: its chunks}.
    Columns of `samples` a slot does not take hold noise."""
    g = torch.Generator().manual_seed(2000 + seed)
    owner, pos, got, chunks = [None] * S, {}, {}, {}
    for st in schedule:
        for s in st.get("close", []):
            fe.close(s)
            owner[s] = None
        for s, u in st.get("open", {}).items():
            assert not fe.is_open[s]
            fe.open(s)
            owner[s], pos[u], got[u], chunks[u] = u, 0, [], []
        counts = [0] * S
        N = max([0] + list(st["samples"].values()))
        x = torch.randn(S, N, generator=g)
        for s, n in st["samples"].items():
            u = owner[s]
            w = utterance(*UTTS[u])[0]
            x[s, :n] = torch.from_numpy(w[pos[u]:pos[u] + n])
            pos[u] += n
            counts[s] = n
            chunks[u].append(n)
        flush = st.get("flush", [])
        mel, frames = fe.step(x.to(dev), counts, flush)
        assert mel.shape == (S, 80, max(frames)) and bool(torch.isfinite(mel).all())
        for s in range(S):
            if owner[s] is not None and frames[s]:
                got[owner[s]].append(mel[s, :, :frames[s]].cpu())
        for s in flush:
            assert not fe.is_open[s]                                      # a flushed slot is free
            owner[s] = None
    return {u: torch.cat(f, dim=1).numpy() for u, f in got.items() if f}, chunks


def test_whole_streams_against_float64(dev):
    fe = front_end(dev, 4, 5600)
    got, chunks = drive(fe, 4, SCHEDULE, dev)
    assert sorted(got) == list(range(len(UTTS)))
    assert {1, 159, 160, 161, 201, 5600} <= set(chunks[0] + chunks[1]) and 0 in chunks[0] and 0 in chunks[2]
    for u, (name, row) in enumerate(UTTS):
        w, ref = utterance(name, row)
        assert sum(chunks[u]) == len(w)
        assert got[u].shape == ref.shape == (80, len(w) // HOP + 1), (u, got[u].shape)
        e2e_check(got[u], ref, f"stream {name} row {row} chunks {chunks[u]}")
    assert fe.is_open == [False] * 4


@pytest.mark.parametrize("name,flush_with_last", [("hop100", True), ("hop128", False), ("hop200", True)])
def test_other_hops_against_float64(dev, name, flush_with_last):
    """The supported hops besides 160 that the offline end-to-end cases carry (hop200: hop = n_fft - pad), two rows of the
    case's noise as two streams with different chunkings, the same bound."""
    from conformer_amd.frontend import ConformerAudioFrontend
    from conformer_amd.stream_frontend import StreamingAudioFrontend
    (_, B, L, cfg), = [c for c in C.E2E_CASES if c[0] == name]
    hop = cfg["hop_length"]
    w = C.e2e_wave(name, B, L).numpy()
    ref = FO.log_mel_numpy64(w[:2], **C.oracle_kwargs(cfg))
    fe = StreamingAudioFrontend(ConformerAudioFrontend(device=dev, **cfg), 2, 3000)
    fe.open(0), fe.open(1)
    steps = [(201, 1), (0, 200), (1, 0), (2000, 3000), (2918, 1919)] + ([] if flush_with_last else [(0, 0)])
    assert [sum(c) for c in zip(*steps)] == [L, L]
    got, pos = [[], []], [0, 0]
    for i, counts in enumerate(steps):
        x = torch.zeros(2, max(counts))
        for s, n in enumerate(counts):
            x[s, :n] = torch.from_numpy(w[s, pos[s]:pos[s] + n])
            pos[s] += n
        mel, frames = fe.step(x.to(dev), counts, [0, 1] if i == len(steps) - 1 else [])
        for s in range(2):
            got[s].append(mel[s, :, :frames[s]].cpu())
    got = np.stack([torch.cat(g, dim=1).numpy() for g in got])
    assert got.shape == ref.shape == (2, 80, L // hop + 1)
    e2e_check(got, ref, f"streams {name}")


# ---- 3. neighbours -------------------------------------------------------------------------------------------------------------
def test_neighbours_do_not_matter(dev):
    """Utterance 0 in slot 1 with the same chunks in two schedules: other neighbours, other f_max per step (the GEMM and the mel
    kernel tile differently), the same frames within the bound of 'same arithmetic, different tiling'."""
    mine = [201, 0, 159, 5600, 1, 4439]
    a = [dict(open={1: 0}, samples={1: mine[0]})] + [dict(samples={1: n}) for n in mine[1:5]] + \
        [dict(samples={1: mine[5]}, flush=[1])]
    b = [dict(open={1: 0, 0: 4, 2: 2}, samples={1: mine[0], 0: 5120, 2: 7}, flush=[0]),
         dict(open={0: 3}, samples={1: mine[1], 0: 400, 2: 2000}, flush=[0]),
         dict(samples={1: mine[2], 2: 2953}, flush=[2]),
         dict(open={2: 1}, samples={1: mine[3], 2: 201}),
         dict(close=[2], samples={1: mine[4]}),
         dict(open={0: 5}, samples={1: mine[5], 0: 400}, flush=[0, 1])]
    ga, _ = drive(front_end(dev, 3, 5600), 3, a, dev, seed=1)
    gb, _ = drive(front_end(dev, 3, 5600), 3, b, dev, seed=2)
    assert ga[0].shape == gb[0].shape == (80, 66)
    r = rel_l2(torch.from_numpy(ga[0]), torch.from_numpy(gb[0]))
    print(f"neighbours rel_l2={r:.3e}")
    assert r < 1e-5
    for u in (3, 4, 5):                                                   # and the neighbours of run b are right themselves
        e2e_check(gb[u], utterance(*UTTS[u])[1], f"neighbour {UTTS[u]}")


# ---- 4. transcribers -----------------------------------------------------------------------------------------------------------
def _model(d, heads, seed, dev, hidden=24, n_blocks=2):
    from model.conformer import Conformer
    P = O.make_params(vocab=len(VOCAB), n_mel=80, n_blocks=n_blocks, d=d, n_heads=heads, ksize=31, lstm_hidden=hidden,
                      seed=seed, dtype=torch.float64)
    m = Conformer(len(VOCAB), 80, n_blocks, d, heads, 31, hidden, 1, 0.0)
    m.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in P.items()}, strict=True)
    return m.to(dev).eval(), P


def _decoder():
    from conformer_amd.decode import BeamCTCDecoder
    return BeamCTCDecoder(VOCAB, 0, skip_ids=(UNK,), beam_width=16)


def _samples(S, counts, starts, utts, dev):
    N = max([0] + list(counts))
    x = torch.zeros(S, N)
    for s, n in enumerate(counts):
        if n:
            x[s, :n] = torch.from_numpy(utterance(*UTTS[utts[s]])[0][starts[s]:starts[s] + n])
    return x.to(dev)


def test_slot_transcriber_step_audio(dev):
    from conformer_amd.slots import SlotTranscriber
    m, _ = _model(32, 4, 71, dev)
    dec = _decoder()
    S = 3
    tr = SlotTranscriber(m, dec, S, 200, audio=front_end(dev, S, 5600))
    ref, fe = SlotTranscriber(m, dec, S, 200), front_end(dev, S, 5600)
    with pytest.raises(ValueError):
        SlotTranscriber(m, dec, S, 200, audio=front_end(dev, 2, 5600))
    with pytest.raises(RuntimeError):
        ref.step_audio(torch.zeros(S, 10, device=dev), [0] * S)           # no front end given
    utts = [0, 4, 2]                                                       # L10400, L5120, L4960
    steps = [dict(open=[0, 1], counts=[5600, 161, 0]), dict(counts=[0, 4959, 0], flush=[1]),
             dict(open=[2], counts=[1, 0, 201]), dict(counts=[4799, 0, 4759], flush=[0]), dict(counts=[0, 0, 0], flush=[2])]
    starts, n_logits = [0] * S, 0
    for st in steps:
        for s in st.get("open", []):
            tr.open(s), ref.open(s), fe.open(s)
        x = _samples(S, st["counts"], starts, utts, dev)
        starts = [a + c for a, c in zip(starts, st["counts"])]
        got, k = tr.step_audio(x, st["counts"], st.get("flush", []))
        mel, frames = fe.step(x, st["counts"], st.get("flush", []))
        want, k2 = ref.step(mel, frames)
        assert k == k2 and got.shape == want.shape
        if max(k):
            n_logits += 1
            assert rel_l2(got, want) < 1e-5, rel_l2(got, want)
    assert n_logits >= 3 and starts == [10400, 5120, 4960]
    assert tr.is_open == [True] * S and tr.audio.is_open == [False] * S    # flushed, not closed: the text is still to be read
    texts = [tr.close(s) for s in range(S)]
    assert texts == [ref.close(s) for s in range(S)]
    tr.open(1)                                                             # and the slot serves again, front end included
    assert tr.audio.is_open == [False, True, False] and tr.audio.received[1] == 0
    tr.close(1)                                                            # (no flush: the close drops the front end's stream)
    assert tr.audio.is_open == [False] * S


def test_streaming_transcriber_step_audio(dev):
    from conformer_amd.transcribe import StreamingTranscriber
    m, _ = _model(32, 4, 91, dev)
    dec = _decoder()
    B = 2
    tr = StreamingTranscriber(m, dec, B, 200, audio=front_end(dev, B, 5600))
    ref, fe = StreamingTranscriber(m, dec, B, 200), front_end(dev, B, 5600)
    with pytest.raises(ValueError):
        StreamingTranscriber(m, dec, B, 200, audio=front_end(dev, 3, 5600))
    for s in range(B):
        fe.open(s)
    x = torch.stack([torch.from_numpy(utterance("L10400", r)[0]) for r in (1, 2)]).to(dev)
    chunks, t0 = [201, 159, 5600, 0, 4440], 0
    for i, c in enumerate(chunks):
        last = i == len(chunks) - 1
        got = tr.step_audio(x[:, t0:t0 + c], flush=last)
        mel, frames = fe.step(x[:, t0:t0 + c], [c] * B, range(B) if last else ())
        assert len(set(frames)) == 1 and mel.shape[2] == frames[0]
        want = ref.step(mel)
        assert got.shape == want.shape
        if want.shape[1]:
            assert rel_l2(got, want) < 1e-5
        t0 += c
    assert t0 == 10400 and ref.encoder.frames == tr.encoder.frames > 0
    assert tr.finish() == ref.finish()
    tr.reset()
    assert tr.audio.is_open == [True] * B and tr.audio.received == [0] * B


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_alone(dev):
    w, ref = utterance("L4960", 1)
    chunks = [300, 1, 2000, 2659]

    def run(refuse):
        fe = front_end(dev, 2, 3000)
        fe.open(0)
        out, t0 = [], 0
        for i, c in enumerate(chunks):
            if refuse:
                z = torch.zeros(2, 3000, device=dev)
                state = (list(fe.is_open), list(fe.received), list(fe.emitted), fe.tails[0].data_ptr())
                for exc, args in [(RuntimeError, (z, [10, 5])), (RuntimeError, (z, [10, 0], [1])),
                                  (ValueError, (torch.zeros(2, 3001, device=dev), [3001, 0])), (ValueError, (z, [3001, 0])),
                                  (ValueError, (z, [0, 0], [0])) if i == 0 else (ValueError, (z, [10], [0]))]:
                    with pytest.raises(exc):
                        fe.step(*args)
                    assert (fe.is_open, fe.received, fe.emitted, fe.tails[0].data_ptr()) == state
            x = torch.zeros(2, c, device=dev)
            x[0] = torch.from_numpy(w[t0:t0 + c]).to(dev)
            mel, frames = fe.step(x, [c, 0], [0] if i == len(chunks) - 1 else [])
            out.append(mel[0, :, :frames[0]])
            t0 += c
        return torch.cat(out, dim=1).cpu()

    plain, refused = run(False), run(True)
    assert plain.shape == refused.shape == ref.shape
    assert rel_l2(refused, plain) <= 1e-6                  # the same launches on the same data
    e2e_check(refused.numpy(), ref, "after refusals")


def test_a_refusal_of_the_encoder_leaves_the_front_end_alone(dev):
    """step_audio checks the front end's step AND the encoder's before either enqueues: mel frames past max_mel_frames raise
    with the front end's tail, counts and slots as they were."""
    from conformer_amd.slots import SlotTranscriber
    m, _ = _model(32, 4, 71, dev)
    w = utterance("L10400", 0)[0]
    tr = SlotTranscriber(m, _decoder(), 2, 40, audio=front_end(dev, 2, 6000))
    ref = SlotTranscriber(m, _decoder(), 2, 40, audio=front_end(dev, 2, 6000))
    tr.open(0), ref.open(0)

    def x(t0, n):
        s = torch.zeros(2, n, device=dev)
        s[0] = torch.from_numpy(w[t0:t0 + n]).to(dev)
        return s

    a, _ = tr.step_audio(x(0, 3000), [3000, 0])
    b, _ = ref.step_audio(x(0, 3000), [3000, 0])
    state = (list(tr.audio.received), list(tr.audio.emitted), list(tr.encoder.mel_seen))
    with pytest.raises(RuntimeError):
        tr.step_audio(x(3000, 6000), [6000, 0])            # 18 + 38 mel frames > 40
    assert (tr.audio.received, tr.audio.emitted, tr.encoder.mel_seen) == state
    a2, ka = tr.step_audio(x(3000, 3200), [3200, 0], [0])
    b2, kb = ref.step_audio(x(3000, 3200), [3200, 0], [0])
    assert ka == kb and ka[0] > 0 and rel_l2(a, b) <= 1e-6 and rel_l2(a2, b2) <= 1e-6
    assert tr.close(0) == ref.close(0)
