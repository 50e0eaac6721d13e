"""CPU side of the front end's stage tests (tests/test_frontend_stages_gpu.py): the case lists and input generators both files
share, and the checks that need no GPU -- the float64 references agree with each other, a float32 restatement of every case
stays inside the bound the device is held to, each plausible wrong answer lies more than 100 times outside it, and the product's
band drawing equals the oracle's.

Bounds (derived, never measured on the device):
  DFT   rel-L2 < 2e-5 over the whole result AND over every single row (the fp32 GEMM TOL of tests/test_property_gpu.py).
  mel   |log error| <= 2e-5.  Every term of sum_k fb[k,m] (Re_k^2 + Im_k^2) is non-negative, so the relative error of the sum
        in any order is at most (nk + 7) 2^-24 <= 1.3e-5 (nk products, the power's three roundings, the four-wave reduction);
        logf adds at most 2 ulp of a result of magnitude <= 12 (< 2e-6); the clamp does not widen it because
        |log max(a, f) - log max(b, f)| <= |log a - log b|.
  end to end   max <= 4 E_max and mean <= 4 E_mean, E = the error of oracle.log_mel_f32 against log_mel_numpy64 on 3 x 16000
        samples of the same noise: two float32 orders on the CPU (sequential and BLAS) differ by up to 2.8x on the smallest
        case and by less than 1.3x on larger ones.
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import frontend_oracle as FO

DFT_TOL = 2e-5
MEL_TOL = 2e-5
E2E_FACTOR = 4.0
FLOOR32 = np.float32(FO.LOG_FLOOR)          # the floor as the kernel receives it


def ceil8(n):
    return (n + 7) // 8 * 8


# ==== reflect padding ========================================================================================================
PAD_CASES = [(1, 201, 200, 601), (3, 201, 200, 640), (2, 1000, 200, 1400), (2, 1000, 200, 1563), (1, 5, 4, 13), (1, 5, 0, 8)]


def pad_case(B, L, pad, ld_out):
    """(x (B, L) float32, expected (B, ld_out) float32: np.pad reflect, zeros from column L + 2 pad)."""
    x = np.random.default_rng(B * 100003 + L * 17 + pad).standard_normal((B, L)).astype(np.float32)
    want = np.zeros((B, ld_out), np.float32)
    want[:, :L + 2 * pad] = np.pad(x, ((0, 0), (pad, pad)), mode="reflect")
    return x, want


# ==== the DFT as a GEMM over overlapping rows ================================================================================
# (rows, n_cols, n_fft, hop)
DFT_SMALL = [(1, 4, 4, 4), (33, 36, 64, 4), (129, 416, 400, 160), (200, 416, 400, 400), (65, 416, 400, 404), (127, 100, 400, 100)]
# rows -> (BM, BN) by csrc/gemm_f32.hip choose_tile at 416 columns: 4 column tiles of 128, so ceil(rows / 128) * 4 tiles of
# 128x128: 174 * 4 = 696 lies in (690, 768] -> 128x128; 193 * 4 = 772 >= 768 (and < 3072) -> 128x64.  Both last row tiles are
# ragged (22200 = 173 * 128 + 56, 24600 = 192 * 128 + 24).
DFT_TILES = [(22200, 416, 400, 160, (128, 128)), (24600, 416, 400, 160, (128, 64))]


def dft_case(rows, n_cols, n_fft, hop):
    """(wave of exactly (rows - 1) hop + n_fft floats, Gaussian basis (n_cols, n_fft)): float32 torch tensors."""
    g = torch.Generator().manual_seed(rows * 7919 + n_cols * 31 + hop)
    wave = torch.randn((rows - 1) * hop + n_fft, generator=g)
    basis = torch.randn(n_cols, n_fft, generator=g)
    return wave, basis


def dft_frames(wave, rows, n_fft, hop):
    return wave.as_strided((rows, n_fft), (hop, 1))


def dft_reference(wave, basis, rows, n_fft, hop):
    return dft_frames(wave.double(), rows, n_fft, hop) @ basis.double().t()


def dft_errors(got, ref):
    """(rel-L2 of the whole, the largest rel-L2 of a single row) against the float64 product."""
    got, ref = got.double(), ref.double()
    d = got - ref
    whole = float(d.norm() / ref.norm())
    per_row = d.norm(dim=1) / ref.norm(dim=1)
    return whole, float(per_row.max())


# ==== power + mel + log ======================================================================================================
# (T, n_mels, n_bins, B, rows_per_utt - T, ld_spec - 2 nk, bank): every value of each axis of
#   T {1, 31, 32, 33, 65} x n_mels {1, 31, 32, 33, 64, 80, 95, 96} x n_bins {1, 7, 8, 9, 24, 201} x B {1, 3} x rows_per_utt {T, T + 3}
#   x ld_spec {2 nk, 2 nk + 4}
# the corners (33, 96, 201) and (1, 1, 1), and the production slaney bank once.  T = 1 goes with B = 3: every case holds an all-zero
# frame, a frame whose mels straddle the floor and at least one ordinary frame.
MEL_MFMA = [
    (1, 1, 1, 3, 0, 0, "random"),
    (33, 96, 201, 3, 3, 4, "random"),
    (33, 96, 201, 1, 0, 0, "random"),
    (31, 31, 7, 1, 3, 0, "random"),
    (32, 32, 8, 3, 0, 4, "random"),
    (65, 33, 9, 1, 3, 4, "random"),
    (65, 64, 24, 3, 0, 0, "random"),
    (1, 80, 201, 3, 3, 4, "random"),
    (31, 95, 201, 1, 0, 4, "random"),
    (32, 1, 201, 1, 3, 0, "random"),
    (65, 96, 24, 1, 3, 0, "random"),
    (33, 64, 1, 3, 0, 4, "random"),
    (65, 80, 201, 3, 3, 0, "slaney"),
]
# the VALU form: n_bins = 201, B = 2, [Re | Im] rows of 402 floats with ld_spec in {402, 404}: (T, n_mels, ld_spec - 402)
MEL_VALU = [(1, 1, 0), (31, 31, 2), (32, 32, 0), (33, 33, 2), (65, 64, 0), (33, 80, 2), (31, 95, 0), (65, 96, 2), (1, 96, 2)]


@functools.lru_cache(maxsize=None)
def mel_case(T, n_mels, n_bins, B, bank):
    """Float32 inputs of one case: re, im (B, T, n_bins) = N(0, 1) exp(U(-6, 3)) per element, fb (n_bins, n_mels).
    The last frame is all zeros (where there are three or more), frame 0 is scaled so that the median of its (positive) mels is
    the floor; the random bank is non-negative and about 30 % dense with a weight in [0.5, 1] at bin 0 and at bin n_bins - 1, where
    the production bank has 0."""
    g = torch.Generator().manual_seed(((T * 131 + n_mels) * 257 + n_bins) * 5 + B)
    shape = (B, T, n_bins)
    re = torch.randn(shape, generator=g) * torch.exp(torch.rand(shape, generator=g) * 9 - 6)
    im = torch.randn(shape, generator=g) * torch.exp(torch.rand(shape, generator=g) * 9 - 6)
    if bank == "slaney":
        assert n_bins == 201
        fb = FO.mel_filterbank(n_freqs=201, n_mels=n_mels, dtype=torch.float64).float()
    else:
        fb = torch.rand(n_bins, n_mels, generator=g) * (torch.rand(n_bins, n_mels, generator=g) < 0.3)
        edge = 0.5 + 0.5 * torch.rand(2, n_mels, generator=g)
        fb[0] = edge[0]
        fb[n_bins - 1] = edge[1]
    re, im = re.reshape(B * T, n_bins), im.reshape(B * T, n_bins)
    mel0 = (re[0].double() ** 2 + im[0].double() ** 2) @ fb.double()
    s = float(torch.sqrt(float(FLOOR32) / mel0[mel0 > 0].median()))
    re[0] *= s
    im[0] *= s
    # frame 1 is ordinary but for Re of its two edge bins, which sits at the top of the range (|N| = 1, U = 3): where it is the only
    # ordinary frame the draw alone can leave an edge bin too weak for any mel to tell whether the kernel lost it
    for k in (0, n_bins - 1):
        re[1, k] = math.copysign(math.exp(3.0), float(re[1, k]))
    if B * T >= 3:                           # (two frames: the straddling one and an ordinary one)
        re[-1] = 0.0
        im[-1] = 0.0
    return re.reshape(shape).contiguous(), im.reshape(shape).contiguous(), fb.contiguous()


def mel_reference(re, im, fb, drop_bin=None):
    """float64 log(max(sum_k fb[k, m] (Re_k^2 + Im_k^2), floor)) of the float32 values: (B, n_mels, T)."""
    power = re.double() ** 2 + im.double() ** 2
    fb = fb.double().clone()
    if drop_bin is not None:
        fb[drop_bin] = 0.0
    return torch.log(torch.clamp(power @ fb, min=float(FLOOR32))).transpose(1, 2).contiguous()


def mel_f32_sequential(re, im, fb):
    """The same sum in float32, one bin after the other (no pairwise tree): the plainest order a kernel could use."""
    re, im, fb = re.numpy(), im.numpy(), fb.numpy()
    power = re * re + im * im
    acc = np.zeros(power.shape[:2] + (fb.shape[1],), np.float32)
    for k in range(fb.shape[0]):
        acc += power[..., k, None] * fb[k]
    return torch.from_numpy(np.log(np.maximum(acc, FLOOR32))).transpose(1, 2)


# ==== SpecAugment ============================================================================================================
SPECAUG_SHAPES = [(1, 1, 1), (2, 80, 101), (3, 7, 37)]


def specaug_band_sets(F, T):
    """name -> bands (axis, start, end); axis 1 = frequency, 2 = time."""
    return {
        "none": [],
        "empty": [(2, T // 2, T // 2), (1, F // 2, F // 2)],
        "to_the_edge": [(2, T - min(T, 5), T), (1, F - min(F, 3), F)],
        "past_the_edge": [(2, T - 1, T + 9), (1, F - 1, F + 40)],
        "overlapping": [(2, 0, min(T, 6)), (2, min(T - 1, 3), min(T, 11)), (1, 0, min(F, 4)), (1, min(F - 1, 2), min(F, 5)), (2, 0, 1)],
        "negative_start": [(2, -7, min(T, 2)), (1, -1, 1)],
    }


# ==== end to end =============================================================================================================
E2E_LENGTHS = [201, 400, 4959, 4960, 5120, 10400]           # T = 2, 3, 31, 32, 33, 66 at hop 160
# (name, B, L, constructor arguments of ConformerAudioFrontend)
E2E_CASES = [(f"L{L}", 3, L, {}) for L in E2E_LENGTHS] + [
    ("mels40", 3, 5120, dict(n_mels=40)),
    ("mels96", 3, 5120, dict(n_mels=96)),
    ("hop100", 3, 5120, dict(hop_length=100)),
    ("hop128", 3, 5120, dict(hop_length=128)),
    ("hop200", 3, 5120, dict(hop_length=200)),
    ("hop150", 3, 5120, dict(hop_length=150)),
    ("hop161", 3, 5120, dict(hop_length=161)),
    ("band20_7600", 3, 5120, dict(fmin=20.0, fmax=7600.0)),
]
CALL_LENGTHS = (4000, 201, 2500)


def noise(B, L, seed):
    """White noise at amplitude 0.3, different in every utterance: a flat spectrum, nothing near the floor."""
    return 0.3 * torch.randn(B, L, generator=torch.Generator().manual_seed(seed))


def oracle_kwargs(cfg):
    names = {"n_mels": "n_mels", "hop_length": "hop", "fmin": "f_min", "fmax": "f_max", "sample_rate": "sample_rate"}
    return {names[k]: v for k, v in cfg.items()}


# noise seed = 1 + the case's index, but where that draw leaves a reference element at the floor (the narrow low filters take one
# or two spectrum bins, and a bin's power is exponentially distributed): asserted for every case below
E2E_SEED = {"mels96": 28, "hop161": 21}


def e2e_wave(name, B, L):
    return noise(B, L, E2E_SEED.get(name, 1 + [c[0] for c in E2E_CASES].index(name)))


@functools.lru_cache(maxsize=None)
def e2e_yardstick():
    """(E_max, E_mean): float32 numpy against float64 numpy on 3 x 16000 samples of the noise, default configuration."""
    w = noise(3, 16000, 0).numpy()
    err = np.abs(FO.log_mel_f32(w).astype(np.float64) - FO.log_mel_numpy64(w))
    return float(err.max()), float(err.mean())


def floor_share(ref):
    return float(np.mean(ref <= np.log(FO.LOG_FLOOR)))


# =============================================================================================================================
# the CPU checks
# =============================================================================================================================
def test_parametrised_oracles_agree():
    """torch.stft oracle, float64 numpy DFT and the float32 restatement at a non-default configuration; defaults unchanged."""
    w = noise(2, 3000, 7)
    kw = dict(n_mels=40, hop=100, f_min=20.0, f_max=7600.0)
    a, b, c = FO.log_mel(w.double(), **kw).numpy(), FO.log_mel_numpy64(w.numpy(), **kw), FO.log_mel_f32(w.numpy(), **kw)
    assert a.shape == b.shape == c.shape == (2, 40, 31) and c.dtype == np.float32
    assert np.abs(a - b).max() < 1e-9                    # float64 FFT against the float64 DFT matrix
    assert np.abs(c - b).max() < 2e-5
    assert FO.batch_lengths([16000, 159, 160]) == [101, 1, 2] and FO.batch_lengths([16000, 99, 100], hop=100) == [161, 1, 2]
    assert torch.equal(FO.mel_filterbank(), FO.mel_filterbank(201, 80, 16000, 0.0, 8000.0))
    assert FO.log_mel(w).shape == (2, 80, 3000 // 160 + 1)
    # at other sample rates the bank spans 0 .. sample_rate / 2
    fb8 = FO.mel_filterbank(n_mels=40, sample_rate=8000, f_max=4000.0, dtype=torch.float64)
    assert fb8.shape == (201, 40) and (fb8.sum(0) > 0).all()


def test_production_bank_is_blind_at_the_edge_bins():
    """Why the mel stage gets a random bank: the slaney bank 0-8000 Hz weighs spectrum bins 0 and 200 with exactly 0."""
    fb = FO.mel_filterbank(dtype=torch.float64)
    assert float(fb[0].abs().max()) == 0.0 and float(fb[200].abs().max()) == 0.0
    _, _, rnd = mel_case(33, 96, 201, 3, "random")
    assert float(rnd[0].min()) > 0 and float(rnd[200].min()) > 0 and float(rnd.min()) >= 0
    assert 0.25 < float((rnd[1:-1] > 0).float().mean()) < 0.35


def test_product_constants_match_the_oracle():
    """The filterbank the product builds (float64, rounded once) equals the oracle's at every tested configuration."""
    from conformer_amd.frontend import _slaney_filterbank
    for cfg in [c[3] for c in E2E_CASES]:
        kw = oracle_kwargs(cfg)
        got = _slaney_filterbank(201, cfg.get("n_mels", 80), 16000, cfg.get("fmin", 0.0), cfg.get("fmax", 8000.0))
        want = FO.mel_filterbank(n_mels=kw.get("n_mels", 80), f_min=kw.get("f_min", 0.0), f_max=kw.get("f_max", 8000.0), dtype=torch.float64)
        assert float((got - want).abs().max()) < 1e-12


@pytest.mark.parametrize("B,L,pad,ld_out", PAD_CASES)
def test_pad_case_reference(B, L, pad, ld_out):
    x, want = pad_case(B, L, pad, ld_out)
    assert ld_out >= L + 2 * pad and L > pad
    assert np.array_equal(want[:, pad:pad + L], x) and not want[:, L + 2 * pad:].any()
    if pad:
        assert np.array_equal(want[:, 0], x[:, pad]) and np.array_equal(want[:, L + 2 * pad - 1], x[:, L - 1 - pad])


@pytest.mark.parametrize("rows,n_cols,n_fft,hop", DFT_SMALL + [c[:4] for c in DFT_TILES])
def test_dft_float32_inside_the_bound_and_wrong_answers_far_outside(rows, n_cols, n_fft, hop):
    wave, basis = dft_case(rows, n_cols, n_fft, hop)
    assert wave.numel() == (rows - 1) * hop + n_fft
    ref = dft_reference(wave, basis, rows, n_fft, hop)
    f32 = torch.from_numpy(dft_frames(wave, rows, n_fft, hop).numpy() @ basis.numpy().T)
    whole, worst = dft_errors(f32, ref)
    assert whole < DFT_TOL and worst < DFT_TOL, (whole, worst)
    # Re and Im blocks swapped (the two halves of the columns)
    swapped = torch.cat([ref[:, n_cols // 2:], ref[:, :n_cols // 2]], dim=1)
    assert dft_errors(swapped, ref)[0] > 100 * DFT_TOL
    # one row one hop late: only the per-row ratio is sure to see it (1 row of 24600 moves the whole by 2 / sqrt(rows))
    if rows > 1:
        for r in (0, rows - 2):
            shifted = ref.clone()
            shifted[r] = ref[r + 1]
            assert dft_errors(shifted, ref)[1] > 100 * DFT_TOL


def test_dft_tile_rule():
    """The row counts of the two large cases against the launch rule restated: csrc/gemm_f32.hip choose_tile, no GLU, K < 2048."""
    def rule(M, ncols):
        n128 = -(-M // 128) * -(-ncols // 128)
        if n128 >= 12 * 256:
            return (128, 128)
        if 690 < n128 <= 768:
            return (128, 128)
        if n128 >= 3 * 256:
            return (128, 64)
        return (64, 64)
    for rows, n_cols, _, _, tile in DFT_TILES:
        assert rule(rows, n_cols) == tile and rows % 128 != 0
    assert all(rule(c[0], c[1]) == (64, 64) for c in DFT_SMALL)
    assert rule(32 * (1000 + 4), 416) == (128, 64)             # the benchmark's batch: 32 x 10 s, 1004 rows per utterance


def _mel_inputs():
    return [(T, m, nb, B, bank) for T, m, nb, B, _, _, bank in MEL_MFMA] + [(T, m, 201, 2, "random") for T, m, _ in MEL_VALU]


def test_mel_grid_covers_every_axis_value():
    col = lambda i: {c[i] for c in MEL_MFMA}  # noqa: E731
    assert col(0) == {1, 31, 32, 33, 65} and col(1) == {1, 31, 32, 33, 64, 80, 95, 96} and col(2) == {1, 7, 8, 9, 24, 201}
    assert col(3) == {1, 3} and col(4) == {0, 3} and col(5) == {0, 4} and col(6) == {"random", "slaney"}
    assert {(33, 96, 201), (1, 1, 1)} <= {c[:3] for c in MEL_MFMA}
    assert {c[0] for c in MEL_VALU} == col(0) and {c[1] for c in MEL_VALU} == col(1) and {c[2] for c in MEL_VALU} == {0, 2}


@pytest.mark.parametrize("T,n_mels,n_bins,B,bank", sorted(set(_mel_inputs())))
def test_mel_float32_inside_the_bound_and_dropped_bin_far_outside(T, n_mels, n_bins, B, bank):
    re, im, fb = mel_case(T, n_mels, n_bins, B, bank)
    ref = mel_reference(re, im, fb)
    assert ref.shape == (B, n_mels, T) and bool(torch.isfinite(ref).all())
    at_floor = ref <= float(np.log(float(FLOOR32)))
    flat = at_floor.transpose(1, 2).reshape(B * T, n_mels)
    assert B * T < 3 or bool(flat[-1].all())                            # the all-zero frame
    if n_mels > 1:
        assert bool(flat[0].any()) and not bool(flat[0].all())          # the straddling frame: mels on both sides of the floor
    err = float((mel_f32_sequential(re, im, fb).double() - ref).abs().max())
    assert err <= MEL_TOL / 10, err                                     # (measured under 9e-7)
    if bank == "random":
        # a kernel that loses the last bin (or the first): the 8-bin groups and the wave split have their edges there
        for k in (n_bins - 1, 0):
            assert float((mel_reference(re, im, fb, drop_bin=k) - ref).abs().max()) > 100 * MEL_TOL


@pytest.mark.parametrize("name,B,L,cfg", E2E_CASES, ids=[c[0] for c in E2E_CASES])
def test_e2e_inputs_avoid_the_floor_and_float32_meets_the_bound(name, B, L, cfg):
    """No reference element of the noise input sits at the floor (nothing is hidden by the clamp), and the float32 restatement of
    every configuration stays inside the bound the device is held to."""
    w = e2e_wave(name, B, L).numpy()
    kw = oracle_kwargs(cfg)
    ref = FO.log_mel_numpy64(w, **kw)
    assert ref.shape == (B, cfg.get("n_mels", 80), L // cfg.get("hop_length", 160) + 1)
    assert floor_share(ref) == 0.0
    e_max, e_mean = e2e_yardstick()
    err = np.abs(FO.log_mel_f32(w, **kw).astype(np.float64) - ref)
    assert err.max() <= E2E_FACTOR * e_max and err.mean() <= E2E_FACTOR * e_mean, (err.max(), err.mean(), e_max, e_mean)


def test_e2e_yardstick_and_its_discrimination():
    """E is float32 rounding (a few 1e-6), ~80 times under the old 5e-3 bound; a filter weight wrong by 0.4 % -- which that bound
    passed -- lies far outside 4 E."""
    e_max, e_mean = e2e_yardstick()
    assert 5e-7 < e_max < 2e-5 and 5e-8 < e_mean < 2e-6, (e_max, e_mean)
    w = noise(3, 16000, 0).numpy()
    ref = FO.log_mel_numpy64(w)
    assert floor_share(ref) == 0.0
    wrong = ref + np.log(1.004)                                         # every weight of the bank 0.4 % too large
    err = np.abs(wrong - ref)
    assert err.max() < 5e-3 and err.max() > 100 * E2E_FACTOR * e_max and err.mean() > 100 * E2E_FACTOR * e_mean


def test_call_batch_reference_has_floor_tails():
    lens = CALL_LENGTHS
    w = torch.zeros(3, max(lens))
    for i, n in enumerate(lens):
        w[i, :n] = noise(1, n, 50 + i)[0]
    ref = FO.log_mel_numpy64(w.numpy())
    floor = np.log(FO.LOG_FLOOR)
    frames = FO.batch_lengths(lens)
    assert frames == [26, 2, 16]
    # frames whose 400-sample window lies wholly in the zero tail: centre t * 160 >= n + 200
    for i, n in enumerate(lens):
        first = -(-(n + 200) // 160)
        assert first >= frames[i]
        if first < ref.shape[2]:
            assert (ref[i, :, first:] == floor).all()
        assert (ref[i, :, :frames[i] - 1] > floor).all()
    e_max, e_mean = e2e_yardstick()
    err = np.abs(FO.log_mel_f32(w.numpy()).astype(np.float64) - ref)
    assert err.max() <= E2E_FACTOR * e_max and err.mean() <= E2E_FACTOR * e_mean, (err.max(), err.mean())


@pytest.mark.parametrize("F,T", [(80, 101), (7, 37), (1, 1)])
def test_augment_draws_the_oracles_bands(F, T):
    """ConformerAugment.draw_bands against oracle.specaugment_bands: ratio < 1, and ratio == 1 with a time_mask_param above T
    (band starts can then be negative and ends lie past T: a mask by comparison covers [max(s, 0), min(e, T)))."""
    from conformer_amd.frontend import ConformerAugment
    for ratio, tparam in ((0.05, 35), (0.5, 35), (1, 500), (1, 27)):
        aug = ConformerAugment(n_time_masks=4, time_mask_param=tparam, n_freq_masks=3, freq_mask_param=27, ratio=ratio)
        aug.generator = torch.Generator().manual_seed(11)
        got = aug.draw_bands(F, T)
        want = FO.specaugment_bands(T, F, 4, tparam, 3, 27, float(ratio), torch.Generator().manual_seed(11))
        assert got == want
        if ratio == 1:
            assert len(got) == 7
    # the oracle's apply is a mask by comparison
    x = torch.arange(2 * 7 * 37, dtype=torch.float32).reshape(2, 7, 37)
    out = FO.specaugment_apply(x, [(2, -5, 3), (1, 6, 90), (2, 30, 30)], -3.25)
    want = x.clone()
    want[..., :3] = -3.25
    want[:, 6:, :] = -3.25
    assert torch.equal(out, want)
