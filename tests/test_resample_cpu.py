"""The resampler's definition and host arithmetic without a GPU (conformer_amd/resample.py, INTEGRATION.md "Input sample rates").

Pinned here: the bank's geometry and row sums at the seven input rates of the contract; the restatement
(tests/resample_restatement.py) against scipy.signal.upfirdn, an independent statement of the same filter; the filter's
orientation and phase order on a sine, its stop band on a tone above the new Nyquist rate; the streaming rule's output counts,
tail lengths and caps over drawn chunkings, and the restated stream against the whole utterance; the new header and its
binding.
"""
import functools
import os
import re

import numpy as np
import pytest
from hypothesis import given, settings
from hypothesis import strategies as st

from tests import resample_restatement as R

TARGET = 16000
# R_in: (o, n, width, K)
TABLE = {8000: (1, 2, 7, 15), 11025: (441, 640, 7, 455), 22050: (441, 320, 9, 459), 32000: (2, 1, 13, 28),
         44100: (441, 160, 17, 475), 48000: (3, 1, 19, 41), 96000: (6, 1, 37, 80)}


@functools.lru_cache(maxsize=None)
def bank(r_in):
    k, o, n, width = R.bank(r_in, TARGET)
    k.setflags(write=False)
    return k, o, n, width


@pytest.mark.parametrize("r_in", sorted(TABLE))
def test_bank_table(r_in):
    from conformer_amd.resample import resample_bank
    k, o, n, width = bank(r_in)
    assert (o, n, width, k.shape[1]) == TABLE[r_in] and k.shape[0] == n
    sums, mass = k.sum(axis=1), np.abs(k).sum(axis=1)
    assert 1.00003 <= sums.min() and sums.max() <= 1.0009, (sums.min(), sums.max())
    assert mass.max() <= 1.87, mass.max()
    got, geo = resample_bank(r_in, TARGET)
    assert geo == (width, o, n) and got.dtype == np.float64 and got.shape == k.shape
    assert np.abs(got - k).max() <= 1e-15                                # (np.sinc against sin(pi t) / (pi t))


def test_bank_of_equal_rates_is_one_tap():
    from conformer_amd.resample import resample_bank
    got, geo = resample_bank(16000, 16000)
    assert geo == (0, 1, 1) and got.tolist() == [[1.0]]
    with pytest.raises(ValueError):
        resample_bank(0, 16000)


@pytest.mark.parametrize("r_in", sorted(TABLE))
def test_restatement_against_upfirdn(r_in):
    """The single prototype h[p] = f(p / (o n)), |p| <= P, P a multiple of o past the filter's support: upfirdn(h, x, up=n,
    down=o) read from index P / o is the definition."""
    from scipy.signal import upfirdn
    k, o, n, width = bank(r_in)
    base = R.geometry(r_in, TARGET)[4]
    x = np.random.default_rng(r_in).standard_normal(3001)
    y, _ = R.resample64(x, k, o, width)
    P = (width + 1) * n * o                                              # f(u) = 0 from |u| = lpw o / base <= width on
    h = R.kernel_f(np.arange(-P, P + 1) / n, o, base)
    full = upfirdn(h, x, up=n, down=o)
    ref = full[P // o:P // o + len(y)]
    assert len(y) == R.out_len(3001, o, n) == len(ref)
    err = np.abs(y - ref).max()
    print(f"upfirdn {r_in}: {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("r_in", [8000, 11025, 44100, 48000, 32000])
def test_a_sine_comes_out_where_it_went_in(r_in):
    """Orientation and phase order: 1 kHz, 0.5 s, equals sin(2 pi 1000 q / 16000) within 2e-3 away from the ends."""
    k, o, n, width = bank(r_in)
    L = r_in // 2
    x = np.sin(2 * np.pi * 1000 * np.arange(L) / r_in)
    y, _ = R.resample64(x, k, o, width)
    q = np.arange(len(y))
    err = np.abs(y - np.sin(2 * np.pi * 1000 * q / TARGET))[100:-100].max()
    print(f"sine {r_in}: {err:.3e}")
    assert len(y) == 8000 and err <= 2e-3


def test_stop_band_from_48k():
    k, o, n, width = bank(48000)
    t = np.arange(24000) / 48000
    rms = [np.sqrt(np.mean(R.resample64(np.sin(2 * np.pi * f * t), k, o, width)[0][100:-100] ** 2)) for f in (1000, 12000)]
    db = 20 * np.log10(rms[1] / rms[0])
    print(f"12 kHz against 1 kHz: {db:.1f} dB")
    assert db < -50


CHUNK = st.sampled_from([0, 1, 2, 3, 6, 7, 19, 37, 440, 441, 442, 900, 3000])


@settings(max_examples=60, deadline=None)
@given(r_in=st.sampled_from(sorted(TABLE)), chunks=st.lists(CHUNK, min_size=0, max_size=12), flush_with_last=st.booleans())
def test_output_counts(r_in, chunks, flush_with_last):
    """resample_plan over drawn chunkings: emitted totals follow Eb, the flush brings ceil(n L / o), tails stay under K, no step
    passes step_output_cap, and every row equals the restated stream's."""
    from conformer_amd.resample import blocks_so_far, resample_plan, step_output_cap
    o, n, width, K = TABLE[r_in]
    cap = step_output_cap(3000, width, o, n)
    steps = [(c, flush_with_last and i == len(chunks) - 1) for i, c in enumerate(chunks)]
    if not flush_with_last or not chunks:
        steps.append((0, True))
    ref = R.Stream(np.zeros((n, K)), o, width, np.float32)
    received = total = 0
    for c, flush in steps:
        p = resample_plan(received, c, flush, width, o, n)
        assert total == n * blocks_so_far(received, width, o)
        received += c
        total += p.outputs
        assert 0 <= p.outputs <= cap and 0 <= p.tail_len < K and 0 <= p.new_tail_len < K and p.new_tail_len <= R.TAIL_LD
        assert p.row(c, flush) == ref.step(np.zeros(c, np.float32), flush)["row"]
        if not flush:
            assert total == n * R.blocks_emitted(received, width, o)
    assert total == -(-n * received // o) == R.out_len(received, o, n) and p.new_tail_len == 0


def test_the_cap_is_reached_within_n():
    """step_output_cap is a bound, and not a loose one: some step of max_chunk samples comes within n outputs of it."""
    from conformer_amd.resample import resample_plan, step_output_cap
    for r_in, (o, n, width, K) in TABLE.items():
        cap = step_output_cap(640, width, o, n)
        most = max(resample_plan(before, 640, True, width, o, n).outputs for before in range(0, 3 * (o + width)))
        assert cap - n <= most <= cap, (r_in, most, cap)


@pytest.mark.parametrize("r_in", [8000, 44100, 48000])
def test_restated_stream_equals_the_whole(r_in):
    k, o, n, width = bank(r_in)
    x = np.random.default_rng(5).standard_normal(2 * o + 2500)
    whole, _ = R.resample64(x, k, o, width)
    for seed, flush_with_last in ((0, True), (1, False)):
        rng, chunks, left = np.random.default_rng(seed), [], len(x)
        while left:
            chunks.append(min(int(rng.choice([0, 1, o - 1 or 1, o, o + 1, width, 700])), left))
            left -= chunks[-1]
        got, steps = R.run_stream(x, chunks, flush_with_last, k, o, width)
        assert got.shape == whole.shape and np.abs(got - whole).max() <= 1e-13
        assert max(len(s["tail_out"]) for s in steps) < k.shape[1]


def test_conversion_and_downmix_restated():
    v = np.array([-32768, -1, 0, 1, 32767], np.int16)
    assert R.from_int16(v).tolist() == [-1.0, -2.0 ** -15, 0.0, 2.0 ** -15, 32767 / 32768]
    x = np.array([[1.0, 2.0 ** -24, 2.0 ** -24], [0.1, 0.2, 0.3]], np.float32)
    # left to right: (1 + 2^-24) rounds back to 1 twice, where any other order gives 1 + 2^-23
    assert R.downmix(x)[0] == np.float32(1.0) * (np.float32(1.0) / np.float32(3.0))
    assert R.downmix(x)[1] == (np.float32(0.1) + np.float32(0.2) + np.float32(0.3)) * (np.float32(1) / np.float32(3))
    assert R.downmix(x[:, :1]).tolist() == x[:, 0].tolist()


def test_header_and_binding():
    """The two entries take the same list and the library exports them; what every header shares (its record, its names, the
    binding, the rebuild message, the build) is in test_abi_binding_cpu."""
    from conformer_amd import _lib
    header = _lib.HEADERS["conformer_hip_resample.h"]
    sigs, params = header.signatures, header.params
    assert sorted(sigs) == ["cfm_resample_f32", "cfm_resample_i16"]
    assert params["cfm_resample_f32"] == params["cfm_resample_i16"] == [
        "samples", "ld_samples", "n_max", "C", "tail_in", "tail_out", "table", "bank_t", "o", "n", "width", "y", "ld_y", "S",
        "stream"]
    assert sigs["cfm_resample_f32"] == sigs["cfm_resample_i16"]
    with open(_lib.HEADER_PATH) as f:
        assert "cfm_resample" not in f.read()                            # the main header stays as it was
    assert os.path.exists(_lib.LIB_PATH), "build the library first (python -m conformer_amd.build)"
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    for name in sigs:
        assert re.search(name.encode() + b"\0", blob), f"{name} is not in the library's symbol strings"
