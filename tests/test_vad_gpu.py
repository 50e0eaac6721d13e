"""Voice activity detection on the MI355X (conformer_amd/vad.py, cfm3_vad_energy_f32 and cfm3_vad_scan_f32).

The float64 restatement (tests/vad_restatement.py) is the yardstick.  Energies: within 5e-5 nats absolute (<= 128 positive fp32
terms in any order err by < 1e-5 relative with the exp's ulps, plus one rounding of a result of magnitude <= ~20).  Integers:
state words, flags and segments equal the restatement on inputs whose every frame keeps both decision margins >= 1e-3, twenty
times the energy tolerance; the margin is asserted here, in float64, on the cast inputs.  Any chunking gives the same bits, with
no margin at all.  Measured on an MI355X: energies 2e-8 .. 5e-7 from float64; the seeded inputs keep margins >= 0.04."""
import math

import numpy as np
import pytest
import torch

from conformer_amd import _lib
from conformer_amd.vad import SCAN_FRAMES, StreamingVad, VadConfig, speech_segments
from tests import vad_restatement as R

pytestmark = pytest.mark.gpu

ETOL, MARGIN, SNR = 5e-5, 1e-3, 1.0
SNR_DB = SNR * 10.0 / math.log(10.0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _config(smooth=5, Wn=128, onset=3, hangover=8, band=None, min_energy=-math.inf, snr_db=SNR_DB):
    """times in frames: the objects below run at mel_seconds = 1"""
    return VadConfig(snr_db, band, float(Wn), float(smooth), float(onset), float(hangover), min_energy)


def _kw(cfg):
    p = cfg.check(1.0, 128)
    return dict(smooth=p.smooth, noise_window=p.noise_window, snr=p.snr, min_energy=p.min_energy, onset=p.onset,
                hangover=p.hangover, band=cfg.band)


def _feed(vad, slots, parts, dev, fill=math.nan):
    """slots: per slot its (n_mel, T_b) frames; parts: per slot the frame counts of the steps.  Columns behind frames[b] hold
    `fill`.  Returns per slot the concatenated energies and flags the steps left in vad.energy / vad.flags."""
    pos = [0] * len(slots)
    es, fs = [[] for _ in slots], [[] for _ in slots]
    for i in range(len(parts[0])):
        ks = [p[i] for p in parts]
        x = torch.full((len(slots), slots[0].shape[0], max(ks)), fill)
        for b, f in enumerate(slots):
            x[b, :, :ks[b]] = f[:, pos[b]:pos[b] + ks[b]]
            pos[b] += ks[b]
        vad.step(x.to(dev), torch.tensor(ks, dtype=torch.int64, device=dev))
        e, fl = vad.energy.cpu(), vad.flags.cpu()
        for b in range(len(slots)):
            es[b].append(e[b, :ks[b]])
            fs[b].append(fl[b, :ks[b]])
    assert pos == [f.shape[1] for f in slots]
    return [torch.cat(e) for e in es], [torch.cat(f) for f in fs]


def _cut(T, step):
    return [step] * (T // step) + ([T % step] if T % step else [])


def _pad(parts):
    n = max(len(p) for p in parts)
    return [p + [0] * (n - len(p)) for p in parts]


def _snapshot(vad):
    return vad.state.cpu().clone(), vad.ring.cpu().clone(), vad.segments.cpu().clone()


# ---- energies ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [(130, 0, 1), (63, 0, 65), (64, 130, 0)], ids=str)
@pytest.mark.parametrize("n_mel, band", [(80, None), (80, (3, 20)), (23, None), (23, (3, 20))], ids=str)   # 23: odd rows are off
def test_energies_equal_the_restatement(dev, n_mel, band, counts):                                         # 8-byte alignment
    rng = np.random.default_rng(n_mel + sum(counts))
    slots = [torch.from_numpy((rng.standard_normal((n_mel, T)) * 3.0 - 4.0).astype(np.float32)) for T in counts]
    cfg = _config(band=band)
    vad = StreamingVad(3, n_mel, cfg, 1.0, device=dev)
    es, _ = _feed(vad, slots, [[T] for T in counts], dev)
    for b, T in enumerate(counts):
        want = R.run(slots[b].numpy(), **_kw(cfg))[1]
        err = np.abs(es[b].numpy().astype(np.float64) - want).max() if T else 0.0
        print(f"n_mel {n_mel} band {band} T {T}: max |e - float64| = {err:.3e}")
        assert err <= ETOL and np.abs(want).max(initial=0.0) < 20.0
    assert torch.isnan(vad.energy.cpu()[1 if counts[1] == 0 else 2]).sum() == 0          # (zeros where nothing was written)


# ---- integers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("onset", [1, 3])
@pytest.mark.parametrize("hangover", [1, 8])
@pytest.mark.parametrize("smooth, Wn", [(1, 7), (5, 128), (16, 512)])
@pytest.mark.parametrize("n_mel, band, min_energy", [(80, None, -math.inf), (23, (3, 20), -2.0)], ids=str)
def test_integers_equal_the_restatement(dev, n_mel, band, min_energy, smooth, Wn, hangover, onset):
    counts = (700, 0, 333)                                    # (700 > 512 + 16: the window slides off the stream's start)
    slots = [torch.from_numpy(R.margin_levels(1000 + b, n_mel, T, SNR)) for b, T in enumerate(counts)]      # committed seeds
    cfg = _config(smooth, Wn, onset, hangover, band, min_energy)
    vad = StreamingVad(3, n_mel, cfg, 1.0, device=dev)
    es, fs = _feed(vad, slots, [[T] for T in counts], dev)
    state, _, segments = _snapshot(vad)
    for b, T in enumerate(counts):
        st, e, fl, mg = R.run(slots[b].numpy(), **_kw(cfg))
        if T:
            assert mg.min() >= MARGIN, (b, float(mg.min()))    # float64, on the cast inputs
            assert np.abs(es[b].numpy() - e).max() <= ETOL
            assert fl.any() and not fl.all()
        assert np.array_equal(fs[b].numpy().astype(bool), fl)
        assert tuple(state[b, :6].tolist()) == st.words() and state[b, 6:].tolist() == [0, 0]
        assert [tuple(r) for r in segments[b, :len(st.segments)].tolist()] == st.segments
    got = vad.finish()
    assert [r.segments for r in got] == [R.run(s.numpy(), **_kw(cfg))[0].finish() for s in slots]
    assert vad.state.cpu().abs().sum() == 0                   # finish arms the slots again


# ---- chunk invariance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smooth, Wn", [(1, 7), (5, 128), (16, 512)])
def test_any_chunking_gives_the_same_bits(dev, smooth, Wn):
    """whole / thirds / 64-frame steps / single frames (cuts inside every smoothing window and inside Wn), no margin needed:
    Gaussian frames around the threshold"""
    counts = (700, 0, 333)
    rng = np.random.default_rng(smooth)
    slots = [torch.from_numpy((rng.standard_normal((23, T)) * 1.5).astype(np.float32)) for T in counts]
    cfg = _config(smooth, Wn, 2, 3, (3, 20), snr_db=2.0)
    outs = []
    for cut in ("whole", "thirds", 64, 1):
        parts = _pad([[T] if cut == "whole" else [T // 3, T // 3, T - 2 * (T // 3)] if cut == "thirds" else _cut(T, cut)
                      for T in counts])
        vad = StreamingVad(3, 23, cfg, 1.0, max_segments=256, device=dev)
        es, fs = _feed(vad, slots, parts, dev)
        outs.append((es, fs, _snapshot(vad)))
    assert outs[0][1][0].any() and not outs[0][1][0].all() and int(outs[0][2][0][0, 5]) >= 2
    for es, fs, snap in outs[1:]:
        for b in range(3):
            assert torch.equal(es[b].view(torch.int32), outs[0][0][b].view(torch.int32))
            assert torch.equal(fs[b], outs[0][1][b])
        for got, want in zip(snap, outs[0][2]):
            assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got,
                               want.view(torch.int32) if want.dtype == torch.float32 else want)
    ring = R.run(slots[0].numpy(), **_kw(cfg))[0].ring()
    assert np.abs(outs[0][2][1][0].numpy() - ring).max() <= ETOL and torch.equal(outs[0][2][1][1], torch.zeros(Wn + smooth - 1))


def test_a_slot_that_crosses_the_scan_launch_split(dev):
    """4 100 frames in one step are one energy launch and two scan launches (4 096 + 4); the same stream in 1 000-frame steps"""
    T = SCAN_FRAMES + 4
    rng = np.random.default_rng(4100)
    slots = [torch.from_numpy((rng.standard_normal((8, n)) * 1.5).astype(np.float32)) for n in (T, 5)]
    cfg = _config(5, 128, 2, 3, snr_db=2.0)
    outs = []
    for parts in ([[T], [5]], _pad([_cut(T, 1000), [5]])):
        vad = StreamingVad(2, 8, cfg, 1.0, max_segments=2048, device=dev)
        es, fs = _feed(vad, slots, parts, dev)
        outs.append((es, fs, _snapshot(vad)))
    for b in range(2):
        assert torch.equal(outs[0][0][b].view(torch.int32), outs[1][0][b].view(torch.int32))
        assert torch.equal(outs[0][1][b], outs[1][1][b])
    for got, want in zip(outs[0][2], outs[1][2]):
        assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got,
                           want.view(torch.int32) if want.dtype == torch.float32 else want)
    st, e, fl, _ = R.run(slots[0].numpy(), **_kw(cfg))
    assert outs[0][2][0][0, 0] == T and np.abs(outs[0][0][0].numpy() - e).max() <= ETOL
    agree = (outs[0][1][0].numpy().astype(bool) == fl).mean()
    assert agree > 0.99 and len(st.segments) > 50             # (no margin here: a rare frame may sit on the threshold)


# ---- safety --------------------------------------------------------------------------------------------------------------------
def test_untouched_slots_and_sentinels_around_every_buffer(dev):
    """a k = 0 slot between two live ones: its state, ring and segments keep their bytes, as do the rows of a guard slot in front
    of and behind every buffer the kernels write (the object runs on the middle rows of larger tensors)"""
    S, n_mel, k_max = 3, 23, 70
    cfg = _config(5, 128, 2, 3, snr_db=2.0)
    vad = StreamingVad(S, n_mel, cfg, 1.0, max_segments=4, device=dev)
    big = {}
    for name in ("state", "ring", "segments"):
        t = getattr(vad, name)
        big[name] = torch.full((S + 2, *t.shape[1:]), 0x5A5A5A5A if t.dtype == torch.int32 else -7.25, dtype=t.dtype, device=dev)
        big[name][1:S + 1][[0, 2]] = 0
        setattr(vad, name, big[name][1:S + 1])
    vad._buffers[k_max] = (torch.full((S + 2, k_max), -7.25, device=dev)[1:S + 1],
                           torch.full((S + 2, k_max), 0x5A, dtype=torch.uint8, device=dev)[1:S + 1])
    before = {name: t.cpu().clone() for name, t in big.items()}
    rng = np.random.default_rng(70)
    x = torch.from_numpy((rng.standard_normal((S, n_mel, k_max)) * 1.5).astype(np.float32))
    ks = [k_max, 0, 33]
    for b in range(S):
        x[b, :, ks[b]:] = math.nan                              # never read
    vad.step(x.to(dev), ks)
    torch.cuda.synchronize()
    for name, t in big.items():
        now = t.cpu()
        for row in (0, 2, S + 1):                               # the guards and the k = 0 slot
            assert torch.equal(now[row].view(torch.int32), before[name][row].view(torch.int32)), (name, row)
    energy, flags = (t._base.cpu() for t in vad._buffers[k_max])
    assert (energy[[0, 2, S + 1]] == -7.25).all() and (flags[[0, 2, S + 1]] == 0x5A).all()
    assert (energy[3, 33:] == -7.25).all() and (flags[3, 33:] == 0x5A).all()
    assert torch.isfinite(energy[1]).all() and torch.isfinite(energy[3, :33]).all()
    assert vad.state.cpu()[:, 0].tolist() == [k_max, 0x5A5A5A5A, 33]
    assert (vad.segments.cpu()[0, min(int(vad.state[0, 5]), 4):] == 0).all()   # nothing behind the closed segments


def test_special_values_are_not_speech_and_do_not_lower_the_floor(dev):
    x = R.levels(5, 8, [(20, 0.0), (10, 3.0), (20, 0.0)])
    x[2, 4], x[:, 6], x[5, 8] = math.nan, -math.inf, math.inf
    cfg = _config(2, 16, 2, 3)
    vad = StreamingVad(1, 8, cfg, 1.0, device=dev)
    es, fs = _feed(vad, [torch.from_numpy(x)], [[50]], dev)
    st, e, fl, _ = R.run(x, **_kw(cfg))
    assert torch.isposinf(es[0][[4, 6, 8]]).all() and not fs[0][[4, 6, 8]].any()
    assert np.array_equal(fs[0].numpy().astype(bool), fl) and fl[20:30].all() and fl.sum() == 10
    assert tuple(vad.state.cpu()[0, :6].tolist()) == st.words()
    assert vad.finish()[0].segments == [(20, 30)]


def test_max_segments_overflow_raises_and_writes_nothing_past_the_buffer(dev):
    x = R.levels(3, 4, [(1, 0.0)] + [(2, 3.0), (2, 0.0)] * 10)
    cfg = _config(1, 64, 2, 2)
    vad = StreamingVad(2, 4, cfg, 1.0, max_segments=3, device=dev)
    guard = torch.full((2 * 3 * 2 + 8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    vad.segments = guard[:12].view(2, 3, 2)                     # slot 1's rows lie behind slot 0's, the guard behind slot 1's
    vad.step(torch.from_numpy(np.stack([x, x])).to(dev), [41, 17])
    assert vad.state.cpu()[:, 5].tolist() == [10, 4]            # the counter goes on counting
    assert (guard.cpu()[12:] == 0x5A5A5A5A).all()
    assert guard.cpu()[:12].view(2, 3, 2).tolist() == [[[1, 3], [5, 7], [9, 11]]] * 2
    with pytest.raises(RuntimeError, match=r"\(0, 10\).*read more often or raise max_segments"):
        vad.read()
    assert vad.state.cpu()[:, 5].tolist() == [0, 0]
    again = vad.read([1])
    assert again[0] is None and again[1].segments == [] and again[1].in_speech is False


def test_read_clears_the_count_and_reports_seconds(dev):
    x = R.levels(3, 4, [(1, 0.0), (4, 3.0), (6, 0.0), (5, 3.0)])
    vad = StreamingVad(1, 4, VadConfig(SNR_DB, None, 0.64, 0.01, 0.02, 0.02), 0.01, device=dev)
    vad.step(torch.from_numpy(x)[None].to(dev), [16])
    got = vad.read()[0]
    assert got.in_speech and got.segments == [(1, 5)] and got.seconds == [(0.01, 0.05)]
    assert vad.read()[0].segments == [] and vad.read()[0].in_speech
    assert vad.finish()[0].segments == [(11, 16)]


# ---- the rest of the interface -------------------------------------------------------------------------------------------------
def test_a_step_is_capturable_and_replays(dev):
    slots = [torch.from_numpy(R.margin_levels(1000 + b, 23, 64, SNR)) for b in range(2)]
    cfg = _config(5, 128, 1, 2, (3, 20))
    eager = StreamingVad(2, 23, cfg, 1.0, device=dev)
    x = torch.stack(slots).to(dev)
    k = torch.tensor([64, 40], dtype=torch.int64, device=dev)
    eager.step(x, k)
    eager.step(x.flip(2).contiguous(), k)
    want = _snapshot(eager)
    fresh = StreamingVad(2, 23, cfg, 1.0, device=dev)
    static = x.clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fresh.step(static, k)                                   # warm-up outside the capture: the buffers of k_max = 64
    torch.cuda.current_stream().wait_stream(stream)
    fresh.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fresh.step(static, k)
    fresh.reset()
    graph.replay()
    static.copy_(x.flip(2))
    graph.replay()
    torch.cuda.synchronize()
    for got, w in zip(_snapshot(fresh), want):
        assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got,
                           w.view(torch.int32) if w.dtype == torch.float32 else w)
    assert int(want[0][0, 0]) == 128 and int(want[0][1, 0]) == 80


def test_speech_segments_is_one_fresh_object_and_finish(dev):
    counts = [700, 333, 64]
    slots = [torch.from_numpy(R.margin_levels(1000 + b, 80, T, SNR)) for b, T in enumerate(counts)]
    cfg = VadConfig(SNR_DB, None, 1.28, 0.05, 0.03, 0.08)
    x = torch.zeros(3, 80, 700)
    for b, s in enumerate(slots):
        x[b, :, :counts[b]] = s
    lengths = torch.tensor(counts, dtype=torch.int64)
    vad = StreamingVad(3, 80, cfg, 0.01, max_segments=700 // 11 + 1, device=dev)
    vad.step(x.to(dev), lengths)
    want = [r.segments for r in vad.finish()]
    assert speech_segments(x.to(dev), lengths.to(dev), config=cfg) == want
    assert speech_segments([s.to(dev) for s in slots], config=cfg) == want
    p = cfg.check(0.01, 80)
    assert (p.smooth, p.noise_window, p.onset, p.hangover) == (5, 128, 3, 8)
    assert want == [R.run(s.numpy(), smooth=5, noise_window=128, snr=p.snr, min_energy=-math.inf, onset=3, hangover=8)[0].finish()
                    for s in slots] and all(len(w) >= 2 for w in want[:2])


def test_host_tensors_and_wrong_dtypes_are_refused(dev):
    vad = StreamingVad(2, 8, _config(), 1.0, device=dev)
    with pytest.raises(_lib.ConformerHipError, match="no CPU fallback"):
        vad.step(torch.zeros(2, 8, 4), [4, 4])
    with pytest.raises(_lib.ConformerHipError, match="float32"):
        vad.step(torch.zeros(2, 8, 4, dtype=torch.float16, device=dev), [4, 4])
    with pytest.raises(_lib.ConformerHipError, match="float32"):
        vad.step(torch.zeros(2, 8, 4, dtype=torch.float64, device=dev), [4, 4])
    with pytest.raises(_lib.ConformerHipError, match="int64"):
        vad.step(torch.zeros(2, 8, 4, device=dev), torch.tensor([4, 4], dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="expected"):
        vad.step(torch.zeros(2, 9, 4, device=dev), [4, 4])
    with pytest.raises(ValueError, match="2 frame counts"):
        vad.step(torch.zeros(2, 8, 4, device=dev), [4])
    with pytest.raises(_lib.ConformerHipError, match="no CPU fallback"):
        StreamingVad(2, 8, _config(), 1.0, device="cpu")
    with pytest.raises(_lib.ConformerHipError, match="no CPU fallback"):
        speech_segments(torch.zeros(1, 8, 40), config=_config(), mel_seconds=1.0)
    assert vad.state.cpu().abs().sum() == 0
