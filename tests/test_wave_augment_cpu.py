"""Waveform augmentation, the half that needs no device: the float64 restatement against independent arithmetic, the banks,
`draw` and `check`, and the argument refusals of the four cfm3_wave_* entries, which return before any HIP call."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conformer_amd import _lib
from conformer_amd import wave_augment as WA
from tests import wave_augment_restatement as W


# ---- 1. the restatement against independent arithmetic ---------------------------------------------------------------------
@pytest.mark.parametrize("L,K,d", [(1, 1, 0), (7, 3, 0), (7, 3, 2), (50, 9, 4), (5, 12, 0), (5, 12, 11), (5, 12, 6), (300, 41, 17)])
def test_reverb_is_convolve_shifted_and_cropped(L, K, d):
    rng = np.random.default_rng(L * 100 + K)
    x, h = rng.standard_normal(L), rng.standard_normal(K)
    y, mass = W.reverb64(x, h, d)
    full = np.convolve(x, h)                                     # full[i] = sum_k h[k] x[i - k]
    assert np.allclose(y, full[d:d + L], rtol=0, atol=1e-12 * np.abs(mass).max())
    assert np.allclose(mass, np.convolve(np.abs(x), np.abs(h))[d:d + L], rtol=1e-12, atol=0)


def test_unit_impulse_shifts():
    x = np.arange(1.0, 11.0)
    for p, d, want in [(0, 0, x), (3, 0, np.r_[0, 0, 0, x[:7]]), (3, 3, x), (3, 5, np.r_[x[2:], 0, 0])]:
        h = np.zeros(6)
        h[p] = 1.0
        assert np.array_equal(W.reverb64(x, h, d)[0], want), (p, d)


@pytest.mark.parametrize("snr_db,gain_db", [(-5.0, 0.0), (30.0, 0.0), (12.5, -6.0), (0.0, 3.0)])
def test_mix_reaches_the_requested_snr(snr_db, gain_db):
    rng = np.random.default_rng(3)
    x, clip = rng.standard_normal(1000), rng.standard_normal(37)
    ax, agn, a, g = W.mix_terms(x, clip, 30, snr_db, gain_db)
    y = ax + agn
    assert a == 10.0 ** (gain_db / 20.0) and g > 0
    achieved = 10.0 * math.log10((x * x).sum() / ((y / a - x) ** 2).sum())
    assert abs(achieved - snr_db) < 1e-9
    assert np.array_equal(W.noise_of(clip, 30, 80), np.r_[clip[30:], clip, clip[:36]])
    # silence on either side: g = 0 and no NaN; no clip: the gain alone
    assert np.array_equal(W.mix64(np.zeros(9), clip, 0, 10.0, 0.0), np.zeros(9))
    assert np.array_equal(W.mix64(x, np.zeros(5), 0, 10.0, 0.0), x)
    assert np.array_equal(W.mix64(x, None, 0, 10.0, gain_db), a * x)


# ---- 2. the banks -------------------------------------------------------------------------------------------------------------
def test_rir_bank():
    rng = np.random.default_rng(0)
    hs = [rng.standard_normal(k).astype(np.float32) for k in (1, 5, 300)]
    hs[1][[1, 3]] = [-9.0, 9.0]                                  # two maxima of |h|: the first is the direct path
    bank = WA.RirBank([torch.from_numpy(h) for h in hs])
    assert len(bank) == 3 and bank.sizes == [1, 5, 300] and bank.k_max == 300 and bank.delays[1] == 1
    assert bank.offsets.tolist() == [0, 1, 6, 306] and bank.data.dtype == np.float32 and bank.offsets.dtype == np.int32
    for h, taps, d in zip(hs, bank.taps, bank.delays):
        assert d == W.direct_path(h)
        assert np.array_equal(taps, W.unit_norm(h).astype(np.float32))              # float64, rounded once
        assert abs(float((taps.astype(np.float64) ** 2).sum()) - 1.0) < len(h) * 2.0 ** -23
    raw = WA.RirBank(hs, normalize=False)
    assert all(np.array_equal(t.view(np.int32), h.view(np.int32)) for t, h in zip(raw.taps, hs)) and raw.delays == bank.delays


def test_bank_refusals():
    with pytest.raises(ValueError, match="all zero"):
        WA.RirBank([np.ones(3), np.zeros(4)])
    WA.RirBank([np.zeros(4)], normalize=False)                   # nothing to divide by, nothing refused
    with pytest.raises(ValueError, match=r"rirs\[1\] is empty"):
        WA.RirBank([np.ones(3), np.zeros(0)])
    with pytest.raises(ValueError, match="empty bank"):
        WA.RirBank([])
    with pytest.raises(ValueError, match=r"clips\[0\] is empty"):
        WA.NoiseBank([np.zeros(0)])
    with pytest.raises(ValueError, match="1-D"):
        WA.NoiseBank([np.zeros((2, 2, 2))])
    with pytest.raises(ValueError, match="NaN"):
        WA.NoiseBank([np.array([0.0, np.nan])])
    assert WA.FIR_MAX_TAPS >= 16384
    WA.RirBank([np.ones(WA.FIR_MAX_TAPS)])
    with pytest.raises(NotImplementedError, match=f"at most {WA.FIR_MAX_TAPS}"):
        WA.RirBank([np.ones(WA.FIR_MAX_TAPS + 1)])
    noise = WA.NoiseBank([np.arange(3.0), np.arange(5.0)])
    assert noise.sizes == [3, 5] and noise.offsets.tolist() == [0, 3, 8] and noise.data.tolist() == [0, 1, 2, 0, 1, 2, 3, 4]


def test_the_constants_come_from_the_header():
    c = _lib.OPEN_CONSTANTS["conformer_hip3_waveaug.h"]
    assert (WA.FIR_TILE_T, WA.FIR_TILE_K, WA.FIR_MAX_TAPS, WA.POWER_CHUNK, WA.MIX_TILE, WA.ROW_COLS) == tuple(
        c[k] for k in ("CFM3_WAVE_FIR_TILE_T", "CFM3_WAVE_FIR_TILE_K", "CFM3_WAVE_FIR_MAX_TAPS", "CFM3_WAVE_POWER_CHUNK",
                       "CFM3_WAVE_MIX_TILE", "CFM3_WAVE_ROW_COLS"))
    assert WA.FIR_TILE_T % 8 == 0 and WA.FIR_TILE_K % 16 == 0


# ---- 3. draw and check --------------------------------------------------------------------------------------------------------
def banks():
    rng = np.random.default_rng(1)
    return (WA.RirBank([rng.standard_normal(k) for k in (4, 9, 2)]), WA.NoiseBank([rng.standard_normal(k) for k in (1, 50, 7, 13)]))


def test_draw_is_reproducible_and_in_range():
    rirs, noise = banks()
    wa = WA.WaveAugment(p_reverb=1.0, rirs=rirs, p_noise=1.0, noise=noise, snr_db=(5, 25), gain_db=(-3, 6))
    wa.generator = torch.Generator().manual_seed(7)
    lengths = [100] * 200
    p = wa.draw(lengths)
    wa.generator.manual_seed(7)
    assert wa.draw(lengths) == p
    assert wa.draw(lengths) != p                                  # the stream moves on
    state = torch.get_rng_state()
    wa.draw(lengths)
    assert torch.equal(torch.get_rng_state(), state)              # a generator of its own leaves torch's alone
    assert isinstance(p, WA.WavePlan) and all(len(f) == 200 for f in p)
    assert set(p.speed) == {0, 1, 2} and set(p.rir) == {0, 1, 2} and set(p.clip) == {0, 1, 2, 3}
    assert all(0 <= s < noise.sizes[c] for s, c in zip(p.offset, p.clip)) and len(set(p.offset)) > 20
    assert all(5 <= v <= 25 for v in p.snr_db) and all(-3 <= v <= 6 for v in p.gain_db)
    assert max(p.snr_db) - min(p.snr_db) > 15 and max(p.gain_db) - min(p.gain_db) > 6
    assert wa.check(lengths, 100, p) == lengths
    # torch's default generator when none is set
    wa.generator = None
    torch.manual_seed(11)
    q = wa.draw([5, 5, 5])
    torch.manual_seed(11)
    assert wa.draw([5, 5, 5]) == q
    # a row's draws do not depend on the batch behind it
    torch.manual_seed(11)
    assert [f[:3] for f in wa.draw([5] * 6)] == [list(f) for f in q]


def test_probability_zero_skips_everything():
    rirs, noise = banks()
    for wa in (WA.WaveAugment(speeds=None), WA.WaveAugment(speeds=((1, 1),), p_reverb=0.0, rirs=rirs, p_noise=0.0, noise=noise)):
        p = wa.draw([3] * 50)
        assert set(p.speed) == {0} and set(p.rir) == {-1} and set(p.clip) == {-1} and set(p.offset) == {0}
        assert set(p.gain_db) == {0.0}
        assert wa.output_lengths([3, 0, 9], WA.WavePlan(*[f[:3] for f in p])) == [3, 0, 9]
        assert wa.output_width(9, p) == 9


def test_construction_refusals():
    rirs, noise = banks()
    with pytest.raises(ValueError, match="without a RirBank"):
        WA.WaveAugment(p_reverb=0.5)
    with pytest.raises(ValueError, match="without a NoiseBank"):
        WA.WaveAugment(p_noise=0.1, rirs=rirs)
    with pytest.raises(ValueError, match="probabilities"):
        WA.WaveAugment(p_noise=1.5, noise=noise)
    with pytest.raises(TypeError):
        WA.WaveAugment(p_noise=0.5, noise=[np.ones(3)])
    with pytest.raises(ValueError, match="snr_db"):
        WA.WaveAugment(snr_db=(25, 5))
    with pytest.raises(NotImplementedError, match="speed 1100:1 "):              # 1100 + 2 ceil(6 * 1100 / 0.99) taps > 1024
        WA.WaveAugment(speeds=((1, 1), (1100, 1)))
    with pytest.raises(NotImplementedError, match="speed 641:700"):             # 700 phases > 640
        WA.WaveAugment(speeds=((641, 700),))
    wa = WA.WaveAugment()
    assert wa.speeds == ((9, 10), (1, 1), (11, 10)) and wa.generator is None
    assert wa.output_lengths([160000, 1, 0], WA.WavePlan([0, 2, 0], *[[0] * 3] * 5)) == [177778, 1, 0]
    assert wa.output_width(160000, WA.WavePlan([1, 2], *[[0] * 2] * 5)) == 160000
    assert wa.output_width(160000, WA.WavePlan([2, 2], *[[0] * 2] * 5)) == 145455


def test_check_refuses_a_bad_plan():
    rirs, noise = banks()
    wa = WA.WaveAugment(p_reverb=0.5, rirs=rirs, p_noise=0.5, noise=noise)
    good = WA.WavePlan([0, 1], [-1, 2], [3, -1], [12, 0], [10.0, 10.0], [0.0, 1.0])
    assert wa.check([4, 0], 4, good) == [4, 0]
    assert wa.check(torch.tensor([4, 0]), 4, good) == [4, 0]
    for field, value in [("speed", [0, 3]), ("speed", [-1, 0]), ("rir", [-2, 0]), ("rir", [0, 3]), ("clip", [4, -1]),
                         ("clip", [-2, -1]), ("offset", [13, 0]), ("offset", [-1, 0]), ("offset", [12, 1]),
                         ("snr_db", [math.nan, 0.0]), ("gain_db", [0.0, math.inf]), ("gain_db", [0.0])]:
        with pytest.raises(ValueError, match="plan"):
            wa.check([4, 0], 4, good._replace(**{field: value}))
    for lengths in ([4, 5], [-1, 0], [4], []):
        with pytest.raises(ValueError, match="lengths|plan"):
            wa.check(lengths, 4, good)
    with pytest.raises(ValueError, match="plan"):
        wa.check([4, 0], 4, tuple(good))
    with pytest.raises(ValueError, match="plan.rir"):
        WA.WaveAugment().check([4, 0], 4, good._replace(clip=[-1, -1], offset=[0, 0]))     # no bank: only -1


# ---- 4. the C ABI: every refusal comes before the first HIP call ---------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from conformer_amd import build
    import os
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


def refusals(entry, good, cases):
    """`good` is a complete argument list with every pointer set; cases: ({index: value}, status)."""
    for change, status in cases:
        args = list(good)
        for i, v in change.items():
            args[i] = v
        assert entry(*args) == status, (change, status)


def test_argument_validation_without_gpu(lib):
    buf = (ctypes.c_double * 64)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    b = a + 64
    NULL, SHAPE, UNSUPPORTED, ALIGN = (_lib.CONSTANTS[k] for k in ("CFM_ERR_NULL", "CFM_ERR_BAD_SHAPE", "CFM_ERR_UNSUPPORTED",
                                                                   "CFM_ERR_ALIGN"))
    big = 1 << 30
    # x, ld_x, n_src, y, ld_y, W, n_dst, map, n, stream
    refusals(lib.cfm3_wave_copy_rows_f32, [a, 8, 2, b, 8, 8, 2, a, 2, None],
             [({i: None}, NULL) for i in (0, 3, 7)] +
             [({i: 0}, SHAPE) for i in (1, 2, 5, 6, 8)] + [({8: -1}, SHAPE), ({4: 7}, SHAPE), ({1: -4}, SHAPE)] +
             [({8: 65536}, UNSUPPORTED), ({5: big, 4: big}, UNSUPPORTED), ({1: big}, UNSUPPORTED), ({3: a}, UNSUPPORTED),
              ({0: None, 8: 0}, NULL), ({8: 0, 3: a}, SHAPE)])
    # x, ld_x, rows, taps, tap_offsets, tap_delays, R, n_taps, k_max, y, ld_y, W, B, stream
    refusals(lib.cfm3_wave_fir_f32, [a, 8, a, a, a, a, 1, 5, 5, b, 8, 8, 2, None],
             [({i: None}, NULL) for i in (0, 2, 3, 4, 5, 9)] +
             [({12: 0}, SHAPE), ({12: -3}, SHAPE), ({6: 0}, SHAPE), ({7: 0}, SHAPE), ({8: 0}, SHAPE), ({8: -1}, SHAPE), ({8: 6}, SHAPE),
              ({11: 0}, SHAPE), ({1: 0}, SHAPE), ({1: -8}, SHAPE), ({10: 7}, SHAPE)] +
             [({8: WA.FIR_MAX_TAPS + 1, 7: WA.FIR_MAX_TAPS + 1}, UNSUPPORTED), ({12: 65536}, UNSUPPORTED),
              ({11: big, 10: big}, UNSUPPORTED), ({1: big}, UNSUPPORTED), ({9: a}, UNSUPPORTED),
              ({0: None, 12: 0}, NULL), ({12: 0, 9: a}, SHAPE)])
    # x, ld_x, rows, noise, clip_offsets, N, n_noise, l_max, partial, B, stream
    refusals(lib.cfm3_wave_power_f64, [a, 8, a, a, a, 1, 5, 8, b, 2, None],
             [({i: None}, NULL) for i in (0, 2, 3, 4, 8)] +
             [({9: 0}, SHAPE), ({5: 0}, SHAPE), ({6: 0}, SHAPE), ({7: 0}, SHAPE), ({7: -2}, SHAPE), ({1: 0}, SHAPE)] +
             [({9: 65536}, UNSUPPORTED), ({7: big}, UNSUPPORTED), ({1: big}, UNSUPPORTED), ({8: b + 4}, ALIGN),
              ({9: 0, 8: b + 4}, SHAPE), ({9: 65536, 8: b + 4}, UNSUPPORTED)])
    # x, ld_x, rows, coef, noise, clip_offsets, N, n_noise, partial, l_max, y, ld_y, W, B, stream
    good = [a, 8, a, a, a, a, 1, 5, a, 8, b, 8, 8, 2, None]
    refusals(lib.cfm3_wave_mix_f32, good,
             [({i: None}, NULL) for i in (0, 2, 3, 4, 5, 8, 10)] +
             [({13: 0}, SHAPE), ({6: -1}, SHAPE), ({7: 0}, SHAPE), ({9: 0}, SHAPE), ({12: 0}, SHAPE), ({1: 0}, SHAPE), ({11: 7}, SHAPE)] +
             [({13: 65536}, UNSUPPORTED), ({12: big, 11: big}, UNSUPPORTED), ({9: big}, UNSUPPORTED), ({1: big}, UNSUPPORTED),
              ({10: a, 11: 16, 12: 8}, UNSUPPORTED),                       # in place needs one pitch
              ({3: a + 4}, ALIGN), ({8: a + 4}, ALIGN), ({13: 0, 3: a + 4}, SHAPE), ({0: None, 13: 0}, NULL)])
    # the gain-only form (N = 0) takes null noise, offsets and partial: it passes every check up to the launch, so only its
    # refusals are called here
    gain_only = [a, 8, a, a, None, None, 0, 0, None, 8, b, 8, 8, 2, None]
    refusals(lib.cfm3_wave_mix_f32, gain_only, [({13: 0}, SHAPE), ({3: None}, NULL), ({3: a + 4}, ALIGN)])
