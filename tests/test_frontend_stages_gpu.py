"""The audio front end stage by stage on the device: reflect padding, the DFT as one GEMM over overlapping wave rows, power + mel + log
in both forms, SpecAugment, then the whole pipeline at several configurations -- each against a float64 restatement of the same
arithmetic at the tightness float32 allows.  The cases, their inputs, the references and the derivation of every bound live in
tests/test_frontend_cpu.py, which also checks on the CPU that a float32 restatement of each case meets its bound and that the
plausible wrong answers miss it by more than 100 times.

Raw entries are called through the checked binding (`_lib.call`) or, where a status is the expected answer, through `_lib.load()`.
Every output is carved from a larger NaN-filled buffer: each element must be written, and nothing behind the end.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import frontend_oracle as FO
from tests import test_frontend_cpu as C

pytestmark = pytest.mark.gpu
BAND = 4096                                  # floats of sentinel behind every carved buffer
OK, BAD_SHAPE, UNSUPPORTED, NULL, ALIGN = 0, -1, -2, -3, -6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conformer_amd import _lib
    assert _lib.load().cfm_device_check() == 0, "not a gfx950 device"
    return torch.device("cuda:0")


def call(name, *args):
    from conformer_amd import _lib, ops
    _lib.call(name, *args, ops._stream())


def status(name, *args):
    """The raw status of an entry (a refusal is an answer, not an error)."""
    from conformer_amd import _lib, ops
    return int(getattr(_lib.load(), name)(*args, ops._stream()))


def carved(n, dev, fill=float("nan")):
    """(the first n floats, the sentinel band behind them) of one allocation filled with `fill`."""
    buf = torch.full((n + BAND,), fill, device=dev, dtype=torch.float32)
    return buf[:n], buf[n:]


def last_tile():
    from conformer_amd import _lib
    out = (ctypes.c_int * 6)()
    _lib.check(_lib.load().cfm_debug_gemm_last_tile(0, ctypes.addressof(out)), "cfm_debug_gemm_last_tile")
    return tuple(out)


# ==== cfm_reflect_pad_f32: bit-exact =========================================================================================
@pytest.mark.parametrize("B,L,pad,ld_out", C.PAD_CASES)
def test_reflect_pad_bit_exact(dev, B, L, pad, ld_out):
    x, want = C.pad_case(B, L, pad, ld_out)
    xd = torch.from_numpy(x).to(dev)
    out, band = carved(B * ld_out, dev)
    call("cfm_reflect_pad_f32", xd.data_ptr(), out.data_ptr(), B, L, pad, ld_out)
    got = out.view(B, ld_out).cpu().numpy()
    assert np.array_equal(got, want)                                   # (no NaN left: every element written, zeros from L + 2 pad)
    assert bool(torch.isnan(band).all())


def test_reflect_pad_refusals(dev):
    x = torch.zeros(2 * 400, device=dev)
    out, band = carved(2 * 1200, dev)
    p, q = x.data_ptr(), out.data_ptr()
    assert status("cfm_reflect_pad_f32", p, q, 2, 200, 200, 600) == BAD_SHAPE          # L == pad: no reflection exists
    assert status("cfm_reflect_pad_f32", p, q, 2, 400, 200, 799) == BAD_SHAPE          # ld_out < L + 2 pad
    assert status("cfm_reflect_pad_f32", None, q, 2, 400, 200, 800) == NULL
    assert status("cfm_reflect_pad_f32", p, None, 2, 400, 200, 800) == NULL
    assert status("cfm_reflect_pad_f32", p, q, 2, 400, 200, 800) == OK
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[2 * 800:]).all()) and bool(torch.isnan(band).all())     # the refused calls wrote nothing


# ==== cfm_dft_frames_f32: the forward fp32 GEMM with lda = hop < K ===========================================================
def run_dft(dev, rows, n_cols, n_fft, hop):
    """Device result (rows, n_cols) on the CPU and the float64 reference.  The wave is followed by a band of NaN in the same
    allocation and holds not one float more than the last frame needs: a read past its end that reaches the output shows."""
    wave, basis = C.dft_case(rows, n_cols, n_fft, hop)
    wd, wband = carved(wave.numel(), dev)
    wd.copy_(wave)
    bd = basis.to(dev)
    out, band = carved(rows * n_cols, dev)
    last_tile()
    call("cfm_dft_frames_f32", wd.data_ptr(), bd.data_ptr(), out.data_ptr(), rows, n_cols, n_fft, hop)
    tile = last_tile()
    got = out.view(rows, n_cols).cpu()
    assert bool(torch.isnan(band).all()) and bool(torch.isnan(wband).all())
    assert bool(torch.isfinite(got).all()), "a non-finite output: a read past the end of the wave, or an element never written"
    return got, C.dft_reference(wave, basis, rows, n_fft, hop), tile


@pytest.mark.parametrize("rows,n_cols,n_fft,hop", C.DFT_SMALL)
def test_dft_frames_small(dev, rows, n_cols, n_fft, hop):
    got, ref, tile = run_dft(dev, rows, n_cols, n_fft, hop)
    whole, worst = C.dft_errors(got, ref)
    print(f"DFT rows={rows} n_cols={n_cols} n_fft={n_fft} hop={hop} tile={tile[:2]} rel_l2={whole:.3e} worst_row={worst:.3e}")
    assert tile[:2] == (64, 64) and tile[3] == 1
    assert whole < C.DFT_TOL and worst < C.DFT_TOL


@pytest.mark.parametrize("rows,n_cols,n_fft,hop,tile", C.DFT_TILES)
def test_dft_frames_large_tiles(dev, rows, n_cols, n_fft, hop, tile):
    """The two tiles the benchmark-sized batches run on (128x128 and 128x64), each with a ragged last row tile, every row checked."""
    got, ref, rec = run_dft(dev, rows, n_cols, n_fft, hop)
    whole, worst = C.dft_errors(got, ref)
    print(f"DFT rows={rows} tile={rec[:2]} rel_l2={whole:.3e} worst_row={worst:.3e}")
    assert rec[:2] == tile and rec[3] == 1
    assert whole < C.DFT_TOL and worst < C.DFT_TOL


def test_dft_frames_refusals(dev):
    w = torch.zeros(8192, device=dev)
    b = torch.zeros(416 * 400, device=dev)
    out, band = carved(16 * 416, dev)
    a, p, q = w.data_ptr(), b.data_ptr(), out.data_ptr()
    assert status("cfm_dft_frames_f32", a, p, q, 16, 416, 400, 150) == BAD_SHAPE        # hop % 4
    assert status("cfm_dft_frames_f32", a, p, q, 16, 416, 398, 160) == BAD_SHAPE        # n_fft % 4
    assert status("cfm_dft_frames_f32", a, p, q, 16, 414, 400, 160) == BAD_SHAPE        # n_cols % 4
    assert status("cfm_dft_frames_f32", a + 4, p, q, 16, 416, 400, 160) == ALIGN
    assert status("cfm_dft_frames_f32", a, p + 8, q, 16, 416, 400, 160) == ALIGN
    assert status("cfm_dft_frames_f32", a, p, q + 4, 16, 416, 400, 160) == ALIGN
    assert status("cfm_dft_frames_f32", None, p, q, 16, 416, 400, 160) == NULL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(band).all())


# ==== power + mel + log ======================================================================================================
def check_mel(got, band, re, im, fb, what):
    ref = C.mel_reference(re, im, fb)
    got = got.view(ref.shape).cpu()
    assert bool(torch.isnan(band).all()), "a write behind the end of out"
    assert bool(torch.isfinite(got).all()), "an element of out was never written, or a poisoned row / column was read"
    err = float((got.double() - ref).abs().max())
    print(f"MEL {what} max_abs_err={err:.3e}")
    assert err <= C.MEL_TOL, err


@pytest.mark.parametrize("T,n_mels,n_bins,B,extra_rows,extra_ld,bank", C.MEL_MFMA)
def test_power_mel_log_mfma(dev, T, n_mels, n_bins, B, extra_rows, extra_ld, bank):
    re, im, fb = C.mel_case(T, n_mels, n_bins, B, bank)
    nk, rpu = C.ceil8(n_bins), T + extra_rows
    ld = 2 * nk + extra_ld
    spec = torch.full((B, rpu, ld), float("nan"))               # NaN: the rows between T and rows_per_utt, the columns from 2 nk
    spec[:, :T, :2 * nk] = 0.0                                  # the zero padding columns of the contract
    spec[:, :T, :n_bins] = re
    spec[:, :T, nk:nk + n_bins] = im
    fbT = torch.zeros(96, nk)
    fbT[:n_mels, :n_bins] = fb.t()
    sd, fd = spec.to(dev), fbT.to(dev)
    out, band = carved(B * n_mels * T, dev)
    call("cfm_power_mel_log_mfma_f32", sd.data_ptr(), ld, fd.data_ptr(), out.data_ptr(), B, T, rpu, n_bins, n_mels, float(C.FLOOR32))
    check_mel(out, band, re, im, fb, f"mfma T={T} n_mels={n_mels} n_bins={n_bins} B={B} rpu={rpu} ld={ld} {bank}")


@pytest.mark.parametrize("T,n_mels,extra_ld", C.MEL_VALU)
def test_power_mel_log_valu(dev, T, n_mels, extra_ld):
    """The VALU form of the C ABI (no caller in the package): rows [Re 0..200 | Im 0..200], utterance b at row b * T."""
    B, n_bins = 2, 201
    re, im, fb = C.mel_case(T, n_mels, n_bins, B, "random")
    ld = 2 * n_bins + extra_ld
    spec = torch.full((B, T, ld), float("nan"))
    spec[:, :, :n_bins] = re
    spec[:, :, n_bins:2 * n_bins] = im
    sd, fd = spec.to(dev), fb.to(dev)
    out, band = carved(B * n_mels * T, dev)
    call("cfm_power_mel_log_f32", sd.data_ptr(), ld, fd.data_ptr(), out.data_ptr(), B, T, n_bins, n_mels, float(C.FLOOR32))
    check_mel(out, band, re, im, fb, f"valu T={T} n_mels={n_mels} ld={ld}")


def test_power_mel_log_refusals(dev):
    spec = torch.zeros(2 * 40 * 420, device=dev)
    fbT = torch.zeros(97 * 208, device=dev)
    out, band = carved(2 * 97 * 33, dev)
    s, f, o = spec.data_ptr(), fbT.data_ptr(), out.data_ptr()
    name = "cfm_power_mel_log_mfma_f32"
    assert status(name, s, 416, f, o, 2, 33, 36, 201, 97, 1e-5) == UNSUPPORTED          # three 32-row accumulators: 96 at most
    assert status(name, s, 418, f, o, 2, 33, 36, 201, 80, 1e-5) == BAD_SHAPE            # ld_spec % 4
    assert status(name, s, 412, f, o, 2, 33, 36, 201, 80, 1e-5) == BAD_SHAPE            # ld_spec < 2 nk
    assert status(name, s, 416, f, o, 2, 33, 32, 201, 80, 1e-5) == BAD_SHAPE            # rows_per_utt < T
    assert status(name, s + 4, 416, f, o, 2, 33, 36, 201, 80, 1e-5) == ALIGN
    assert status(name, s, 416, f + 8, o, 2, 33, 36, 201, 80, 1e-5) == ALIGN
    assert status(name, None, 416, f, o, 2, 33, 36, 201, 80, 1e-5) == NULL
    name = "cfm_power_mel_log_f32"
    assert status(name, s, 402, f, o, 2, 33, 200, 80, 1e-5) == UNSUPPORTED              # the VALU form is built for 201 bins
    assert status(name, s, 400, f, o, 2, 33, 201, 80, 1e-5) == BAD_SHAPE                # ld_spec < 2 n_bins
    assert status(name, s, 402, None, o, 2, 33, 201, 80, 1e-5) == NULL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(band).all())


# ==== SpecAugment: bit-exact =================================================================================================
@pytest.mark.parametrize("value", [0.0, -3.25])
@pytest.mark.parametrize("B,F,T", C.SPECAUG_SHAPES)
def test_specaugment_kernel_bit_exact(dev, B, F, T, value):
    x = torch.randn(B, F, T, generator=torch.Generator().manual_seed(B * 1000 + F * 10 + T))
    for name, bands in C.specaug_band_sets(F, T).items():
        buf, band = carved(B * F * T, dev, fill=7.0)
        buf.copy_(x.flatten())
        bt = torch.tensor(bands, dtype=torch.int32, device=dev).reshape(-1, 3) if bands else None
        call("cfm_specaugment_apply_f32", buf.data_ptr(), B, F, T, None if bt is None else bt.data_ptr(), len(bands), value)
        got = buf.view(B, F, T).cpu()
        want = FO.specaugment_apply(x, [(a, s, min(e, F if a == 1 else T)) for a, s, e in bands], value)
        assert torch.equal(got, want), name
        assert bool((band == 7.0).all()), name
        if name in ("none", "empty"):
            assert torch.equal(got, x), name
        else:
            assert int((got == value).sum()) > 0, name


def test_augment_mean_fill_and_full_ratio(dev):
    """zero_masking=False fills with the mean taken BEFORE masking; ratio == 1 with a time_mask_param above T (no cap: band starts
    below 0 and ends past T) equals the oracle's bands applied."""
    from conformer_amd.frontend import ConformerAugment
    x = torch.randn(2, 80, 101, generator=torch.Generator().manual_seed(5)) - 2.0
    aug = ConformerAugment(n_time_masks=2, time_mask_param=20, n_freq_masks=2, freq_mask_param=10, ratio=0.5, zero_masking=False)
    aug.generator = torch.Generator().manual_seed(9)
    xd = x.to(dev)
    mean = float(xd.mean())
    assert abs(mean - float(x.double().mean())) < 1e-5
    out = aug(xd).cpu()
    bands = FO.specaugment_bands(101, 80, 2, 20, 2, 10, 0.5, torch.Generator().manual_seed(9))
    assert len(bands) == 4 and any(e > s for _, s, e in bands)
    want = FO.specaugment_apply(x, bands, mean)
    assert torch.equal(out, want) and int((out == np.float32(mean)).sum()) > 0

    y = torch.randn(3, 7, 37, generator=torch.Generator().manual_seed(6))
    full = ConformerAugment(n_time_masks=3, time_mask_param=500, n_freq_masks=2, freq_mask_param=27, ratio=1)
    full.generator = torch.Generator().manual_seed(12)
    out = full(y.to(dev)).cpu()
    bands = FO.specaugment_bands(37, 7, 3, 500, 2, 27, 1.0, torch.Generator().manual_seed(12))
    assert len(bands) == 5
    assert torch.equal(out, FO.specaugment_apply(y, bands, 0.0))


# ==== end to end =============================================================================================================
def e2e_check(got, ref, what):
    e_max, e_mean = C.e2e_yardstick()
    err = np.abs(got.astype(np.float64) - ref)
    print(f"E2E {what} max={err.max():.3e} mean={err.mean():.3e}  (E_max={e_max:.3e} E_mean={e_mean:.3e}: "
          f"{err.max() / e_max:.2f} x, {err.mean() / e_mean:.2f} x)")
    assert err.max() <= C.E2E_FACTOR * e_max and err.mean() <= C.E2E_FACTOR * e_mean, (err.max(), err.mean(), e_max, e_mean)


@pytest.mark.parametrize("name,B,L,cfg", C.E2E_CASES, ids=[c[0] for c in C.E2E_CASES])
def test_logmel_end_to_end_tight(dev, name, B, L, cfg):
    """White noise (nothing at the floor) through mel_spectrogram against the float64 oracle within 4 x the float32 yardstick.
    hop 150 and 161 run the copied-frames branch (a hop that is no multiple of 4 floats)."""
    from conformer_amd.frontend import ConformerAudioFrontend
    fe = ConformerAudioFrontend(device=dev, **cfg)
    w = C.e2e_wave(name, B, L)
    got = fe.mel_spectrogram(w.to(dev)).cpu().numpy()
    ref = FO.log_mel_numpy64(w.numpy(), **C.oracle_kwargs(cfg))
    assert got.shape == ref.shape == (B, fe.n_mels, L // fe.hop_length + 1)
    e2e_check(got, ref, name)


def call_batch():
    return [C.noise(1, n, 50 + i)[0] for i, n in enumerate(C.CALL_LENGTHS)]


def test_call_batch_tails_sit_at_the_floor(dev):
    """Lengths (4000, 201, 2500) through __call__: the frames that lie wholly in a zero-padded tail (41 % of the elements) are
    the oracle's floor, as ONE device value.  That value is logf(1e-5f), measured 1.6e-6 from log(1e-5) (inside the 2 ulp of 11.5
    the mel bound allows), which alone puts this batch's mean error at 2.6 E_mean where the noise cases sit at 1.0-1.3."""
    from conformer_amd.frontend import ConformerAudioFrontend
    fe = ConformerAudioFrontend(device=dev)
    audios = call_batch()
    mels, lengths = fe(audios)
    assert lengths.tolist() == FO.batch_lengths(C.CALL_LENGTHS) == [26, 2, 16]
    padded = torch.stack([torch.nn.functional.pad(a, (0, max(C.CALL_LENGTHS) - a.numel())) for a in audios])
    ref = FO.log_mel_numpy64(padded.numpy())
    got = mels.cpu().numpy()
    assert got.shape == ref.shape == (3, 80, 26)
    at_floor = ref == np.log(FO.LOG_FLOOR)
    assert at_floor[1, :, 4:].all() and at_floor[2, :, 17:].all() and not at_floor[0].any()
    floor = np.unique(got[at_floor])
    assert floor.size == 1 and abs(float(floor[0]) - math.log(float(C.FLOOR32))) <= 2e-6      # one value: logf(floor), 2 ulp of 11.5
    e2e_check(got, ref, "call(4000, 201, 2500)")


def test_front_end_writes_stay_inside_their_buffers(dev):
    """mel_spectrogram (both hop branches), __call__ with an augment and one FrontendPipeline batch with every buffer the front end
    allocates carved out of sentinel bytes; the results equal the unguarded ones."""
    from conformer_amd.frontend import ConformerAudioFrontend, ConformerAugment
    from conformer_amd.pipeline import FrontendPipeline
    from tests.test_write_guard_gpu import guarded_allocations
    fe, fe150 = ConformerAudioFrontend(device=dev), ConformerAudioFrontend(device=dev, hop_length=150)
    audios = call_batch()
    w = C.noise(3, 5120, 3).to(dev)
    want, want150 = fe.mel_spectrogram(w), fe150.mel_spectrogram(w)
    want_call, _ = fe(audios)

    def augment():
        a = ConformerAugment(n_time_masks=2, time_mask_param=10, n_freq_masks=2, freq_mask_param=10, ratio=0.5, zero_masking=False)
        a.generator = torch.Generator().manual_seed(4)
        return a
    want_aug = augment()(want_call.clone())
    with guarded_allocations() as gt:
        got, got150 = fe.mel_spectrogram(w), fe150.mel_spectrogram(w)
        got_aug, lengths = fe(audios, augment=augment())
        batches = list(FrontendPipeline([audios], fe))
        bad = gt.check()
        n = len(gt.allocs)
    assert n >= 12, f"the hook saw only {n} allocations: the proxy is not in the path"
    assert not bad, f"{len(bad)} of {n} buffers were written outside their bounds: {bad[:5]}"
    assert torch.equal(got, want) and torch.equal(got150, want150) and torch.equal(got_aug, want_aug)
    assert lengths.tolist() == [26, 2, 16]
    (mels, frames, order), = batches
    assert frames.tolist() == [26, 16, 2] and torch.equal(mels, want_call[order])
