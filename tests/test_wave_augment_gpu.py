"""Waveform augmentation on the device (conformer_amd/wave_augment.py, csrc/wave_augment.hip) against the float64 restatement
of tests/wave_augment_restatement.py.

Every call here writes into a (B, ld) window of a NaN-filled (B + 2, ld + MARGIN) buffer and reads rows whose samples behind
their length are NaN: a write outside the window, a column behind lengths' that is not zero, or a read behind a length fails
whichever test it happens in.

Bounds.  FIR: |y - y64| <= (K + 1) 2^-24 sum_k |h[k]| |x[t + d - k]|, the bound of a K-term fp32 sum in any order (a sequential
fp32 chain modelled on the CPU at K = 1000 reaches 4.0 2^-24 sum |h||x|); with integer data below 2^24 the sum is exact.  Mix:
|y - (a x + a g n)| <= 6 2^-24 (|a x| + |a g n|): c2 within one ulp of fp32(a g) is 3 units, the product 1, the sum 1, plus
slack.  Speed: the resampler's own (K + 2) 2^-24 sum |terms| (tests/test_resample_gpu.py)."""
import numpy as np
import pytest
import torch

from tests import wave_augment_restatement as W

pytestmark = pytest.mark.gpu
MARGIN = 5
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conformer_amd import _lib
    assert _lib.load().cfm_device_check() == 0, "not a gfx950 device"
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def ragged(rows, fill=np.nan):
    """(B, Lmax) float32 with `fill` behind every row's samples."""
    x = np.full((len(rows), max(1, max(len(r) for r in rows))), fill, np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return x


def apply_carved(wa, dev, x, lengths, plan):
    """wa.apply into a NaN-framed window: (wave' on the host, lengths')."""
    B, ld = x.shape[0], wa.output_width(x.shape[1], plan)
    frame = torch.full((B + 2, ld + MARGIN), float("nan"), device=dev, dtype=torch.float32)
    out = frame[1:B + 1, :ld]
    got, out_lengths = wa.apply(torch.from_numpy(x).to(dev), lengths, plan, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.shape == (B, ld)
    host = frame.cpu().numpy()
    assert np.isnan(host[0]).all() and np.isnan(host[-1]).all(), "a row before or behind the batch was written"
    assert np.isnan(host[:, ld:]).all(), "the margin behind ld was written"
    y = host[1:B + 1, :ld]
    assert np.isfinite(y).all(), "a column was not written, or a sample behind a row's length was read"
    assert out_lengths == wa.output_lengths(lengths, plan)
    for b, n in enumerate(out_lengths):
        assert not y[b, n:].any(), f"row {b}: not zero behind its length"
    return y, out_lengths


def plan_of(B, **fields):
    from conformer_amd.wave_augment import WavePlan
    base = dict(speed=[0] * B, rir=[-1] * B, clip=[-1] * B, offset=[0] * B, snr_db=[10.0] * B, gain_db=[0.0] * B)
    base.update(fields)
    return WavePlan(**base)


def ints(rng, n, lo=-8, hi=8):
    return rng.integers(lo, hi + 1, n).astype(np.float32)


def shaped_response(rng, K, mode):
    """Integer taps in [-7, 7] and one +-8 at d = 0, K - 1 or K // 2: the direct path."""
    h = ints(rng, K, -7, 7)
    d = (0, K - 1, K // 2)[mode]
    h[d] = 8.0 if rng.integers(2) else -8.0
    return h, d


# ---- 5. the FIR on integer data: bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("turn", range(6))
def test_fir_exact_on_integers(dev, turn):
    from conformer_amd import wave_augment as WA
    T, S = WA.FIR_TILE_T, WA.FIR_TILE_K
    Ks = [1, 2, S - 1, S, S + 1, 2 * S + 5]
    lengths = [1, T - 1, T, T + 1, 2 * T + 3, 0, 100, T + 1]
    rng = np.random.default_rng(50 + turn)
    hs, ds, rir = [], [], []
    for j in range(len(lengths)):
        h, d = shaped_response(rng, Ks[(turn + j) % 6], (turn + 2 * j) % 3)
        hs.append(h)
        ds.append(d)
        rir.append(j)
    rir[5], rir[7] = 3, -1                                                     # the empty row has a response, the last row has none
    bank = WA.RirBank(hs, normalize=False)
    assert bank.delays == ds and all(np.array_equal(t, h) for t, h in zip(bank.taps, hs))
    wa = WA.WaveAugment(speeds=None, p_reverb=1.0, rirs=bank, device=dev)
    rows = [ints(rng, L) for L in lengths]
    y, _ = apply_carved(wa, dev, ragged(rows), lengths, plan_of(len(lengths), rir=rir))
    for b, (x, r) in enumerate(zip(rows, rir)):
        want = x if r < 0 else W.reverb64(x, hs[r], ds[r])[0]
        assert np.array_equal(bits(y[b, :len(x)]), bits(want)), (b, len(x), len(hs[r]), ds[r])


def test_fir_exact_at_8192_taps(dev):
    from conformer_amd import wave_augment as WA
    rng = np.random.default_rng(8192)
    hs = [shaped_response(rng, 8192, mode) for mode in (2, 0)]
    bank = WA.RirBank([h for h, _ in hs], normalize=False)
    wa = WA.WaveAugment(speeds=None, p_reverb=1.0, rirs=bank, device=dev)
    rows = [ints(rng, 4096), ints(rng, 4096)]
    y, _ = apply_carved(wa, dev, ragged(rows), [4096, 4096], plan_of(2, rir=[0, 1]))
    for b in range(2):
        want, mass = W.reverb64(rows[b], *hs[b])
        assert mass.max() < 2 ** 24                                              # every partial sum is an exact integer
        assert np.array_equal(bits(y[b]), bits(want)), b


def test_unit_impulses_shift_exactly(dev):
    """The entry itself with a delay table of its own: a unit impulse at tap p with the direct path declared at d moves the row
    by d - p samples, whatever the other (zero) taps and the tiles do."""
    from conformer_amd import _lib, ops
    from conformer_amd import wave_augment as WA
    T, S = WA.FIR_TILE_T, WA.FIR_TILE_K
    K, L = 2 * S + 9, T + 77
    cases = [(0, 0), (1, 0), (S - 1, 0), (S, 3), (S + 1, K - 1), (2 * S + 8, 0), (5, K - 1), (S, S), (2 * S, 2 * S + 8)]
    rng = np.random.default_rng(6)
    x = rng.standard_normal((len(cases), L)).astype(np.float32)
    taps = np.zeros((len(cases), K), np.float32)
    for r, (p, _) in enumerate(cases):
        taps[r, p] = 1.0
    B = len(cases)
    rows = np.zeros((B, WA.ROW_COLS), np.int32)
    rows[:, 0], rows[:, 1] = L, np.arange(B)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xd, rd, hd = t(x), t(rows), t(taps.reshape(-1))
    od, dd = t(np.arange(B + 1, dtype=np.int32) * K), t(np.array([d for _, d in cases], np.int32))
    y = torch.full((B, L + MARGIN), float("nan"), device=dev, dtype=torch.float32)
    _lib.call("cfm3_wave_fir_f32", xd.data_ptr(), L, rd.data_ptr(), hd.data_ptr(), od.data_ptr(), dd.data_ptr(), B, B * K, K,
              y.data_ptr(), L + MARGIN, L, B, ops._stream())
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    assert np.isnan(y[:, L:]).all()
    for r, (p, d) in enumerate(cases):
        want = np.zeros(L, np.float32)
        s = d - p                                                            # y[t] = x[t + s]
        if s >= 0:
            want[:L - s] = x[r, s:]
        else:
            want[-s:] = x[r, :L + s]
        assert np.array_equal(bits(y[r, :L]), bits(want)), (p, d)


# ---- 6. the FIR on random data: the rounding bound ----------------------------------------------------------------------------
def test_fir_rounding_bound(dev, capsys):
    from conformer_amd import wave_augment as WA
    S, L = WA.FIR_TILE_K, 300
    rng = np.random.default_rng(66)
    hs = [(rng.standard_normal(K) * np.exp(-np.arange(K) / (K / 6.0))).astype(np.float32) for K in (S + 1, 1000)]
    bank = WA.RirBank(hs)
    wa = WA.WaveAugment(speeds=None, p_reverb=1.0, rirs=bank, device=dev)
    rows = [rng.standard_normal(L).astype(np.float32) for _ in range(4)]
    rir = [0, 1, 1, 0]
    y, _ = apply_carved(wa, dev, ragged(rows), [L] * 4, plan_of(4, rir=rir))
    worst = 0.0
    for b, r in enumerate(rir):
        K = bank.sizes[r]
        want, mass = W.reverb64(rows[b], bank.taps[r], bank.delays[r])
        ratio = np.abs(y[b].astype(np.float64) - want) / (U * mass)
        worst = max(worst, float(ratio.max()))
        assert (ratio <= K + 1).all(), (b, K, float(ratio.max()))
    with capsys.disabled():
        print(f"\nFIR rounding: worst |y - y64| / (2^-24 sum |h||x|) = {worst:.3f} (bound K + 1 = {S + 2} and 1001)")


# ---- 7. the mix ----------------------------------------------------------------------------------------------------------------
def mix_cases(rng):
    """(x, clip index, offset, snr_db, gain_db) per row and the clips."""
    from conformer_amd import wave_augment as WA
    clips = [rng.standard_normal(n).astype(np.float32) for n in (7, 1, 13, 50)] + [np.zeros(9, np.float32)]
    n = lambda L: rng.standard_normal(L).astype(np.float32)
    rows = [(n(100), 0, 3, 10.0, 0.0),                     # N_c < L, several wraps
            (n(50), 1, 0, 10.0, 0.0),                      # N_c = 1
            (n(WA.MIX_TILE + 1), 2, 12, 10.0, 0.0),        # s = N_c - 1, one sample in the second workgroup
            (n(1), 3, 49, 10.0, 0.0),                      # L = 1
            (n(255), 3, 0, 10.0, 0.0), (n(256), 3, 1, 10.0, 0.0), (n(257), 3, 2, 10.0, 0.0),       # around the block size
            (n(WA.POWER_CHUNK + 1), 3, 7, 10.0, 2.0),      # a second chunk of the powers
            (np.zeros(40, np.float32), 0, 0, 10.0, 0.0),   # silent x: g = 0
            (n(40), 4, 0, 10.0, 0.0),                      # silent noise: g = 0
            (n(300), 0, 1, -5.0, 0.0), (n(300), 3, 5, 30.0, -3.0),
            (n(300), -1, 0, 10.0, -6.0),                   # gain only
            (n(300), -1, 0, 10.0, 0.0),                    # neither: not touched
            (n(0), 2, 0, 10.0, 0.0)]                       # an empty row
    return rows, clips


def check_mix(y, rows, clips):
    worst = 0.0
    for b, (x, c, s, snr, gain) in enumerate(rows):
        L = len(x)
        if c < 0 and gain == 0.0:
            assert np.array_equal(bits(y[b, :L]), bits(x)), f"row {b}: a skipped row changed"
            continue
        ax, agn, a, g = W.mix_terms(x, clips[c] if c >= 0 else None, s, snr, gain)
        assert g > 0 or c < 0 or not x.any() or not clips[c].any()
        err, scale = np.abs(y[b, :L].astype(np.float64) - (ax + agn)), U * (np.abs(ax) + np.abs(agn))
        assert (err <= 6 * scale).all(), (b, float((err / np.maximum(scale, 1e-300)).max()))
        if L and scale.max() > 0:
            worst = max(worst, float((err[scale > 0] / scale[scale > 0]).max()))
    return worst


def test_mix_against_float64(dev, capsys):
    from conformer_amd import wave_augment as WA
    rows, clips = mix_cases(np.random.default_rng(77))
    wa = WA.WaveAugment(speeds=None, p_noise=1.0, noise=WA.NoiseBank(clips), device=dev)
    plan = plan_of(len(rows), clip=[r[1] for r in rows], offset=[r[2] for r in rows], snr_db=[r[3] for r in rows],
                   gain_db=[r[4] for r in rows])
    x, lengths = ragged([r[0] for r in rows]), [len(r[0]) for r in rows]
    y, _ = apply_carved(wa, dev, x, lengths, plan)
    worst = check_mix(y, rows, clips)
    with capsys.disabled():
        print(f"\nmix: worst |y - (a x + a g n)| / (2^-24 (|a x| + |a g n|)) = {worst:.3f} (bound 6)")
    # in place behind a reverb with a unit response: the same bits
    both = WA.WaveAugment(speeds=None, p_reverb=1.0, rirs=WA.RirBank([np.ones(1)]), p_noise=1.0, noise=wa.noise, device=dev)
    z, _ = apply_carved(both, dev, x, lengths, plan._replace(rir=[0] * len(rows)))
    assert np.array_equal(bits(z), bits(y))


def test_rows_without_noise_read_no_clip(dev):
    """Every clip on the device is NaN; rows with a gain only and rows with nothing come out as if the bank were not there."""
    from conformer_amd import wave_augment as WA
    rng = np.random.default_rng(78)
    noise = WA.NoiseBank([np.ones(5), np.ones(300)])
    noise.on(dev)[0].fill_(float("nan"))
    wa = WA.WaveAugment(speeds=None, p_noise=1.0, noise=noise, device=dev)
    rows = [rng.standard_normal(L).astype(np.float32) for L in (300, 10, 257, 64)]
    gains = [-6.0, 0.0, 3.5, 0.0]
    got, _ = wa.apply(torch.from_numpy(ragged(rows)).to(dev), [300, 10, 257, 64], plan_of(4, gain_db=gains, clip=[-1, -1, -1, 1]))
    y = got.cpu().numpy()
    for b, x in enumerate(rows[:3]):
        want = (np.float32(10.0 ** (gains[b] / 20.0)) * x).astype(np.float32) if gains[b] else x
        assert np.array_equal(bits(y[b, :len(x)]), bits(want)) and not y[b, len(x):].any(), b
    assert np.isnan(y[3, :64]).all() and not y[3, 64:].any()                 # the one row that has a clip did read the bank


# ---- 8, 9, 10. the whole object --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole(dev):
    """A WaveAugment with every stage, a batch of four rows and a hand-made plan that uses all of them."""
    from conformer_amd import wave_augment as WA
    rng = np.random.default_rng(10)
    rirs = WA.RirBank([(rng.standard_normal(K) * np.exp(-np.arange(K) / 40.0)) for K in (300, 77)])
    noise = WA.NoiseBank([rng.standard_normal(n) for n in (500, 31)])
    wa = WA.WaveAugment(p_reverb=0.5, rirs=rirs, p_noise=0.5, noise=noise, snr_db=(5, 25), gain_db=(-3, 3), device=dev)
    lengths = [3000, 2500, 1, 2999]
    rows = [rng.standard_normal(L).astype(np.float32) for L in lengths]
    plan = plan_of(4, speed=[0, 2, 1, 0], rir=[1, -1, 0, 0], clip=[0, 1, -1, -1], offset=[17, 30, 0, 0],
                   snr_db=[8.0, 20.0, 10.0, 10.0], gain_db=[-2.0, 0.0, 0.0, 1.5])
    return wa, rows, lengths, plan


def test_all_four_stages_stage_by_stage(dev, whole):
    from conformer_amd import _lib
    wa, rows, lengths, plan = whole
    x = ragged(rows)
    B = len(rows)
    before = _lib.CALLS[0]
    full, full_lengths = apply_carved(wa, dev, x, lengths, plan)
    assert _lib.CALLS[0] - before == 5 + 1 + 2               # gather, 9:10, 11:10, scatter, the copy of (1, 1) | FIR | powers, mix
    # 1. speed alone, against the resampler's restatement at the resampler's tolerance
    y1, l1 = apply_carved(wa, dev, x, lengths, plan_of(B, speed=plan.speed))
    for b in range(B):
        num, den = wa.speeds[plan.speed[b]]
        want, mass, K = W.speed64(rows[b], num, den)
        assert l1[b] == len(want)
        if num == den:
            assert np.array_equal(bits(y1[b, :l1[b]]), bits(rows[b]))
        else:
            assert (np.abs(y1[b, :l1[b]].astype(np.float64) - want) <= (K + 2) * U * mass + 1e-30).all(), b
    same = [1] * B                                            # from here on the rows keep their length: speed (1, 1)
    ld = y1.shape[1]
    carry = lambda y, n: [y[b, :n[b]] for b in range(B)]
    # 2. the reverb alone on what the speed stage gave
    y2, l2 = apply_carved(wa, dev, ragged(carry(y1, l1) + [np.zeros(ld, np.float32)])[:B], l1, plan_of(B, speed=same, rir=plan.rir))
    assert l2 == l1
    for b, r in enumerate(plan.rir):
        if r < 0:
            assert np.array_equal(bits(y2[b, :l1[b]]), bits(y1[b, :l1[b]]))
        else:
            want, mass = W.reverb64(y1[b, :l1[b]], wa.rirs.taps[r], wa.rirs.delays[r])
            assert (np.abs(y2[b, :l1[b]].astype(np.float64) - want) <= (wa.rirs.sizes[r] + 1) * U * mass).all(), b
    # 3. the mix alone on what the reverb gave
    y3, l3 = apply_carved(wa, dev, ragged(carry(y2, l2) + [np.zeros(ld, np.float32)])[:B], l2,
                          plan._replace(speed=same, rir=[-1] * B))
    stage3 = [(y2[b, :l2[b]], plan.clip[b], plan.offset[b], plan.snr_db[b], plan.gain_db[b]) for b in range(B)]
    check_mix(y3, stage3, wa.noise.clips)
    # the three stages in one call: the same kernels on the same data
    assert full_lengths == l3 == wa.output_lengths(lengths, plan) and np.array_equal(bits(full), bits(y3))


def test_apply_is_deterministic_and_counts_its_launches(dev, whole):
    from conformer_amd import _lib
    wa, rows, lengths, plan = whole
    x = torch.from_numpy(ragged(rows, fill=0.0)).to(dev)
    a, la = wa.apply(x, lengths, plan)
    b, lb = wa.apply(x, lengths, plan)
    assert la == lb and a.dtype == torch.float32 and torch.equal(a, b)
    B = len(rows)
    for p, launches in [(plan_of(B, speed=[1] * B), 1),                                       # nothing drawn: the zero-filled copy
                        (plan_of(B, speed=[1] * B, gain_db=[0.0, 1.0, 0.0, 0.0]), 1),         # gain only: the mix
                        (plan_of(B, speed=[1] * B, clip=[-1, 0, -1, -1]), 2),                 # noise: powers and mix
                        (plan_of(B, speed=[1] * B, rir=[-1, -1, 1, -1]), 1),                  # reverb: the FIR
                        (plan_of(B, speed=[2] * B), 3),                                       # one factor: gather, resample, scatter
                        (plan_of(B, speed=[2, 2, 1, 1], rir=[0] * B), 5)]:
        before = _lib.CALLS[0]
        y, n = wa.apply(x, lengths, p)
        assert _lib.CALLS[0] - before == launches, (p, _lib.CALLS[0] - before)
        assert y.shape == (B, wa.output_width(x.shape[1], p)) and y.data_ptr() != x.data_ptr()
    y, n = wa.apply(x, lengths, plan_of(B, speed=[1] * B))
    want = x.clone()
    for b, L in enumerate(lengths):
        want[b, L:] = 0
    assert torch.equal(y, want) and n == lengths
    # a refused call has launched nothing
    before = _lib.CALLS[0]
    for bad in (plan._replace(rir=[1, -1, 0, 2]), plan._replace(offset=[17, 31, 0, 0]), plan._replace(speed=[0, 3, 1, 0])):
        with pytest.raises(ValueError, match="plan"):
            wa.apply(x, lengths, bad)
    with pytest.raises(ValueError, match="lengths"):
        wa.apply(x, [3000, 2500, 1, 3001], plan)
    with pytest.raises(ValueError, match="host lengths"):
        wa.apply(x, torch.tensor(lengths, device=dev), plan)
    with pytest.raises(ValueError, match="out"):
        wa.apply(x, lengths, plan, out=torch.empty(B, 7, device=dev))
    assert _lib.CALLS[0] == before


def test_front_end_and_pipeline_take_it(dev, whole):
    from conformer_amd.frontend import ConformerAudioFrontend
    from conformer_amd.pipeline import FrontendPipeline
    wa = whole[0]
    fe = ConformerAudioFrontend(device=dev)
    rng = np.random.default_rng(12)
    batches = [[torch.from_numpy(rng.standard_normal(L).astype(np.float32)) for L in Ls]
               for Ls in ([2400, 1801, 3000], [1600, 2222], [999, 2048, 1777, 1200])]
    wa.generator = torch.Generator().manual_seed(5)
    serial = [fe(audios, wave_augment=wa) for audios in batches]
    # the call is the padded batch through apply, then the log-mel
    wa.generator.manual_seed(5)
    for audios, (mels, frames) in zip(batches, serial):
        lengths = [a.numel() for a in audios]
        batch = torch.zeros(len(audios), max(lengths))
        for i, a in enumerate(audios):
            batch[i, :lengths[i]] = a
        w2, l2 = wa.apply(batch.to(dev), lengths, wa.draw(lengths))
        assert l2 != lengths                                       # (the seed draws a speed other than 1 somewhere in every batch)
        assert torch.equal(mels, fe.mel_spectrogram(w2)) and frames.tolist() == [v // fe.hop_length + 1 for v in l2]
    # the pipeline: the same batches under the same seed, sorted by the new lengths
    wa.generator.manual_seed(5)
    got = list(FrontendPipeline(batches, fe, wave_augment=wa))
    torch.cuda.synchronize()
    assert len(got) == 3
    for (mels, frames, order), (want, want_frames) in zip(got, serial):
        assert torch.equal(frames, want_frames.index_select(0, order)) and bool((frames[:-1] >= frames[1:]).all())
        assert torch.equal(mels, want.index_select(0, order))
    wa.generator = None
    # without the keyword nothing changes
    plain = fe(batches[0])
    assert torch.equal(plain[0], fe(batches[0], wave_augment=None)[0])
    assert plain[0].shape[2] == 3000 // fe.hop_length + 1
