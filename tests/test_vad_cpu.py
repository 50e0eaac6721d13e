"""Voice activity detection, the parts that need no GPU: VadConfig's refusals and its seconds -> frames conversion,
speech_islands case by case, the float64 restatement's own chunk invariance and the segment-count bound, and every refusal of
the two ABI entries (conformer_hip3_vad.h), which all return before any HIP call."""
import ctypes
import math

import numpy as np
import pytest

from conformer_amd import _lib
from conformer_amd.vad import (BAND_MAX, SCAN_FRAMES, SMOOTH_MAX, STATE_COLS, WINDOW_MAX, VadConfig, VadFrames, segment_bound,
                               speech_islands)
from tests import vad_restatement as R


@pytest.fixture(scope="module")
def lib():
    import os
    from conformer_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


# ---- VadConfig -------------------------------------------------------------------------------------------------------------------
def test_the_family_is_in_the_open_table():
    assert _lib.OPEN_CONSTANTS["conformer_hip3_vad.h"] == {
        "CFM3_VAD_STATE_COLS": 8, "CFM3_VAD_SCAN_FRAMES": 4096, "CFM3_VAD_SMOOTH_MAX": 16, "CFM3_VAD_WINDOW_MAX": 512,
        "CFM3_VAD_BAND_MAX": 128}
    assert (STATE_COLS, SCAN_FRAMES, SMOOTH_MAX, WINDOW_MAX, BAND_MAX) == (8, 4096, 16, 512, 128)
    assert _lib.OPEN_PARAMS["cfm3_vad_energy_f32"] == ["mel", "ld_slot", "ld_mel", "k", "k_max", "n_mel", "m_lo", "m_hi", "energy",
                                                       "ld_energy", "S", "stream"]
    assert _lib.OPEN_PARAMS["cfm3_vad_scan_f32"] == ["energy", "ld_energy", "k", "k_max", "smooth", "noise_window", "snr",
                                                     "min_energy", "onset", "hangover", "state", "ring", "flags", "ld_flags",
                                                     "segments", "max_segments", "S", "stream"]
    assert [_lib.OPEN_ENTRIES["cfm3_vad_scan_f32"][1][i] for i in (6, 7)] == [ctypes.c_float, ctypes.c_float]


def test_snr_db_has_no_default():
    with pytest.raises(TypeError):
        VadConfig()
    assert VadConfig(9.0)[1:] == (None, 3.0, 0.05, 0.05, 0.3, -math.inf, 0.2, 0.2, 0.5)


def test_seconds_to_frames():
    p = VadConfig(10.0).check(0.01, 80)
    assert p == VadFrames(0, 80, 5, 300, math.log(10.0), -math.inf, 5, 30, 20, 20, 50)
    assert VadConfig(3.0).check(0.01, 80).snr == pytest.approx(3.0 * math.log(10.0) / 10.0, rel=0, abs=1e-15)
    # round(seconds / mel_seconds), as EndpointRule.frames: 0.125 / 0.01 = 12.5 rounds to even, 0.135 / 0.01 to 14
    p = VadConfig(6.0, band=(3, 20), noise_window=5.12, smooth=0.125, onset=0.135, hangover=0.3, min_energy=-2.5,
                  pad_before=0.0, pad_after=0.016, min_gap=1.0).check(0.01, 23)
    assert p[:4] == (3, 20, 12, 512) and p[5:] == (-2.5, 14, 30, 0, 2, 100)
    assert VadConfig(6.0, hangover=0.0051).check(0.01, 80).hangover == 1
    assert VadConfig(6.0, noise_window=3.0, smooth=0.05).check(0.02, 80)[2:4] == (2, 150)       # (0.05 / 0.02 = 2.5 -> 2)


@pytest.mark.parametrize("kw, word", [
    (dict(snr_db=math.nan), "snr_db"), (dict(snr_db=math.inf), "snr_db"), (dict(snr_db="9"), "snr_db"), (dict(snr_db=True), "snr_db"),
    (dict(band=(3,)), "band"), (dict(band=(3.0, 20)), "band"), (dict(band=(5, 5)), "band"), (dict(band=(-1, 5)), "band"),
    (dict(band=(0, 81)), "band"), (dict(band="all"), "band"),
    (dict(noise_window=5.13), "noise_window"), (dict(noise_window=0.004), "noise_window"), (dict(noise_window=-1.0), "noise_window"),
    (dict(noise_window=math.inf), "noise_window"),
    (dict(smooth=0.17), "smooth"), (dict(smooth=0.0), "smooth"), (dict(smooth=math.nan), "smooth"),
    (dict(onset=0.0), "onset"), (dict(onset=-0.05), "onset"), (dict(hangover=0.004), "hangover"), (dict(hangover=True), "hangover"),
    (dict(min_energy=math.nan), "min_energy"), (dict(min_energy=math.inf), "min_energy"), (dict(min_energy="x"), "min_energy"),
    (dict(pad_before=-0.1), "pad_before"), (dict(pad_after=math.inf), "pad_after"), (dict(min_gap=math.nan), "min_gap"),
], ids=str)
def test_config_refusals(kw, word):
    with pytest.raises(ValueError, match=word):
        VadConfig(**{"snr_db": 9.0, **kw}).check(0.01, 80)


def test_config_refuses_bad_surroundings():
    with pytest.raises(ValueError, match="mel_seconds"):
        VadConfig(9.0).check(0.0, 80)
    with pytest.raises(ValueError, match="n_mel"):
        VadConfig(9.0).check(0.01, 0)
    with pytest.raises(ValueError, match="at most 128"):
        VadConfig(9.0).check(0.01, 129)
    assert VadConfig(9.0, band=(1, 129)).check(0.01, 200)[:2] == (1, 129)


# ---- speech_islands --------------------------------------------------------------------------------------------------------------
def test_islands_padding_clamps_to_the_recording():
    assert speech_islands([(10, 50)], 60, 20, 20, 0) == [(0, 60)]
    assert speech_islands([(100, 150)], 1000, 20, 30, 0) == [(80, 180)]
    assert speech_islands([(100, 150)], 160, 0, 30, 0) == [(100, 160)]


def test_islands_start_on_the_encoder_grid():
    assert speech_islands([(103, 150)], 1000, 0, 0, 0) == [(100, 150)]
    assert speech_islands([(103, 150)], 1000, 2, 0, 0) == [(100, 150)]      # 101 -> 100
    assert speech_islands([(103, 150)], 1000, 4, 0, 0) == [(96, 150)]       # 99 -> 96
    assert speech_islands([(104, 150)], 1000, 0, 0, 0) == [(104, 150)]
    assert all(a % 4 == 0 for a, _ in speech_islands([(i * 37 + 1, i * 37 + 9) for i in range(20)], 800, 3, 3, 0))


def test_islands_merge_below_min_gap_only():
    # islands (100, 200) and (240, 300): the gap is 40 frames
    assert speech_islands([(100, 200), (240, 300)], 1000, 0, 0, 40) == [(100, 200), (240, 300)]     # exactly min_gap: kept apart
    assert speech_islands([(100, 200), (240, 300)], 1000, 0, 0, 41) == [(100, 300)]                 # one short of it: merged
    assert speech_islands([(100, 200), (241, 300)], 1000, 0, 0, 41) == [(100, 300)]                 # (241 -> 240)
    assert speech_islands([(100, 200), (180, 300)], 1000, 0, 0, 0) == [(100, 300)]                  # overlapping
    assert speech_islands([(100, 200), (200, 300)], 1000, 0, 0, 0) == [(100, 300)]                  # touching
    assert speech_islands([(100, 200), (230, 300)], 1000, 20, 20, 0) == [(80, 320)]                 # the pads overlap
    assert speech_islands([(100, 300), (150, 160)], 1000, 0, 0, 0) == [(100, 300)]                  # nested


def test_islands_shorter_than_an_encoder_frame_are_extended():
    assert speech_islands([(0, 3)], 1000, 0, 0, 0) == [(0, 7)]                                      # at the start: at its end
    assert speech_islands([(500, 503)], 1000, 0, 0, 0) == [(500, 507)]
    assert speech_islands([(997, 1000)], 1000, 0, 0, 0) == [(992, 1000)]                            # 996 + 7 > 1000: back by 4
    assert speech_islands([(998, 1000)], 1001, 0, 0, 0) == [(992, 1001)]                            # the end first, then back
    assert speech_islands([(1, 3)], 5, 0, 0, 0) == [(0, 5)]                                         # a recording that has no 7
    assert speech_islands([(500, 503), (504, 600)], 1000, 0, 0, 0) == [(500, 600)]                  # grown into its neighbour
    assert speech_islands([(500, 503), (508, 600)], 1000, 0, 0, 0) == [(500, 507), (508, 600)]


def test_islands_of_nothing():
    assert speech_islands([], 1000, 20, 20, 50) == []
    assert speech_islands([], 0, 0, 0, 0) == []
    with pytest.raises(ValueError, match="no segment"):
        speech_islands([(5, 5)], 10, 0, 0, 0)
    with pytest.raises(ValueError, match="pad_before"):
        speech_islands([(5, 6)], 10, -1, 0, 0)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smooth, Wn", [(1, 7), (5, 128), (16, 512)])
def test_restatement_chunk_invariance(smooth, Wn):
    x = R.margin_levels(31, 23, 700, 1.0)
    kw = dict(smooth=smooth, noise_window=Wn, snr=1.0, min_energy=-2.0, onset=3, hangover=8, band=(3, 20))
    whole = R.run(x, **kw)
    assert whole[2].any() and not whole[2].all() and len(whole[0].segments) >= 2
    for step in (1, 5, 64):
        chunks = [step] * (700 // step) + ([700 % step] if 700 % step else [])
        st, e, fl, mg = R.run(x, chunks, **kw)
        assert np.array_equal(e, whole[1]) and np.array_equal(fl, whole[2]) and np.array_equal(mg, whole[3])
        assert st.words() == whole[0].words() and st.segments == whole[0].segments and st.finish() == whole[0].finish()
        assert np.array_equal(st.ring(), whole[0].ring())


def test_restatement_special_frames_are_not_speech_and_do_not_lower_the_floor():
    x = R.levels(5, 8, [(20, 0.0), (10, 3.0), (20, 0.0)]).astype(np.float64)
    x[2, 4], x[:, 6], x[5, 8] = math.nan, -math.inf, math.inf
    st, e, fl, mg = R.run(x, smooth=2, noise_window=16, snr=1.0, min_energy=-math.inf, onset=2, hangover=3)
    assert np.isposinf(e[[4, 6, 8]]).all() and not fl[[4, 6, 8]].any() and np.isinf(mg[[4, 6, 8]]).all()
    assert np.isfinite(e[np.setdiff1d(np.arange(50), [4, 6, 8])]).all()
    assert fl[20:30].all() and not fl[:20].any() and not fl[30:].any() and st.finish() == [(20, 30)]


@pytest.mark.parametrize("onset, hangover", [(1, 1), (3, 8), (2, 1)])
def test_segment_count_bound_on_the_densest_pattern(onset, hangover):
    """onset raw frames, hangover others, again and again: the most segments any input can close."""
    T = 20 * (onset + hangover) + onset
    pattern = [(onset, 3.0), (hangover, 0.0)] * 20 + [(onset, 3.0)]
    x = R.levels(3, 4, [(1, 0.0)] + pattern)[:, :T + 1]
    st = R.run(x, smooth=1, noise_window=64, snr=1.0, min_energy=-math.inf, onset=onset, hangover=hangover)[0]
    assert len(st.segments) == 20 and st.in_speech
    assert len(st.segments) <= segment_bound(T + 1, onset, hangover) == (T + 1) // (onset + hangover) + 1
    assert [b - a for a, b in st.segments] == [onset] * 20


# ---- the ABI's refusals, before any HIP call ------------------------------------------------------------------------------------
def test_argument_validation_without_gpu(lib):
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    NULL, SHAPE, UNSUPPORTED = (_lib.CONSTANTS[k] for k in ("CFM_ERR_NULL", "CFM_ERR_BAD_SHAPE", "CFM_ERR_UNSUPPORTED"))

    def call(entry, base, **kw):
        args = list(base)
        for k, v in kw.items():
            args[int(k[1:])] = v
        return entry(*args)

    # mel, ld_slot, ld_mel, k, k_max, n_mel, m_lo, m_hi, energy, ld_energy, S, stream
    energy = dict(entry=lib.cfm3_vad_energy_f32, base=[a, 80 * 64, 64, a, 64, 80, 0, 80, a, 64, 3, None])
    for i in (0, 3, 8):
        assert call(**energy, **{f"a{i}": None}) == NULL, i
    for bad in (dict(a10=0), dict(a10=-1), dict(a4=-1), dict(a5=0), dict(a6=-1), dict(a6=80), dict(a6=40, a7=40), dict(a7=81),
                dict(a2=63), dict(a1=80 * 64 - 1), dict(a1=-1), dict(a9=63)):
        assert call(**energy, **bad) == SHAPE, bad
    assert call(**energy, a5=200, a1=200 * 64, a7=129) == UNSUPPORTED and call(**energy, a10=65536) == UNSUPPORTED
    assert call(**energy, a0=None, a10=0) == NULL and call(**energy, a10=0, a7=200) == SHAPE      # the order
    assert call(**energy, a4=0, a0=None, a2=0, a1=0, a9=0) == 0                                  # k_max = 0: nothing launched
    # energy, ld_energy, k, k_max, smooth, noise_window, snr, min_energy, onset, hangover, state, ring, flags, ld_flags,
    # segments, max_segments, S, stream
    scan = dict(entry=lib.cfm3_vad_scan_f32, base=[a, 64, a, 64, 5, 300, 1.0, -math.inf, 5, 30, a, a, a, 64, a, 4, 3, None])
    for i in (0, 2, 10, 11, 12, 14):
        assert call(**scan, **{f"a{i}": None}) == NULL, i
    for bad in (dict(a16=0), dict(a3=-1), dict(a4=0), dict(a5=0), dict(a8=0), dict(a9=0), dict(a15=0), dict(a1=63), dict(a13=63),
                dict(a6=math.nan), dict(a7=math.nan), dict(a4=-3), dict(a8=-1)):
        assert call(**scan, **bad) == SHAPE, bad
    for bad in (dict(a3=4097, a1=4097, a13=4097), dict(a4=17), dict(a5=513), dict(a8=(1 << 24) + 1), dict(a9=(1 << 24) + 1),
                dict(a15=(1 << 24) + 1), dict(a16=65536)):
        assert call(**scan, **bad) == UNSUPPORTED, bad
    assert call(**scan, a0=None, a4=0) == NULL and call(**scan, a4=0, a5=513) == SHAPE and call(**scan, a6=math.nan, a5=513) == SHAPE
    assert call(**scan, a3=0, a0=None, a1=0, a13=0) == 0                                         # k_max = 0: nothing launched
