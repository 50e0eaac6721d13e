"""The restated dropout mask (tests/dropout_restatement.py) on its own: published test vectors, the statistics of a Bernoulli
mask down to the four lanes of one hash and to neighbouring elements and seeds, and the proof that the device equality tests
(tests/test_dropout_sites_gpu.py) can tell the plausible wrong masks apart at the sizes, seeds and p they run.

Every statistical bound is 5 standard errors of the binomial expectation with q = 1 - threshold / 65536: derived, not measured.
The inputs are pinned, so the test is deterministic; the worst value over all of them is printed."""
import numpy as np
import pytest

from tests import dropout_restatement as R


def test_hash_is_splitmix64():
    """The published splitmix64 outputs for seed 0: output g is the finaliser of g * GOLDEN."""
    want = (0x0, 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F)
    assert [int(R.hash64(0, g)) for g in range(4)] == list(want)
    assert [int(v) for v in R.hash64(0, np.arange(4))] == list(want)
    # the seed is the counter's origin: hash64(s, g) is output g of the stream seeded with s, all mod 2^64
    assert int(R.hash64(R.GOLDEN, 0)) == want[1] and int(R.hash64(2 ** 64 - R.GOLDEN, 1)) == 0
    assert int(R.hash64(2 ** 64 - 1, 5)) == int(R.hash64(-1, 5))


def test_lanes_take_16_bits_from_the_low_end():
    z = int(R.hash64(12345, 7))
    assert [int(R.bits(12345, 28 + e)) for e in range(4)] == [(z >> (16 * e)) & 0xFFFF for e in range(4)]
    assert [int(b) for b in R.bits(0, np.arange(4, 8))] == [0xCDAF, 0x7B1D, 0xA839, 0xE220]
    assert not R.keep(0, np.arange(4), 2.0 ** -16).any()                  # hash64(0, 0) == 0: seed 0 drops elements 0..3
    for seed in R.SEEDS:                                                   # the grouped evaluation is the same function
        for start, n in ((0, 1), (0, 4), (1, 9), (3, 1030), (4093, 2050)):
            assert np.array_equal(R.bits_range(seed, n, start), R.bits(seed, start + np.arange(n)))


def test_thresholds():
    for p, th in ((0.1, 6554), (0.2, 13108), (0.25, 16384), (0.5, 32768), (2.0 ** -16, 1), (1e-6, 1), (0.99998, 65535), (0.0, 0)):
        assert R.threshold(p) == th, p
    assert R.threshold(0.1, np.floor) == 6553


def test_mask_values_and_index_maps():
    m = R.mask((7, 12), 0.25, 12345)
    assert m.dtype == np.float32 and set(np.unique(m)) == {np.float32(0), np.float32(4) / np.float32(3)}
    assert np.array_equal(m != 0, R.keep(12345, R.gemm_index(7, 12), 0.25))
    assert np.array_equal(R.gemm_index(7, 12).reshape(-1), np.arange(84))
    assert np.array_equal(R.attention_index(2, 3, 5).reshape(-1), np.arange(150))
    assert R.inv_keep(0.1) == np.float32(1) / np.float32(0.9)
    a = R.mask((2, 2, 61, 61), 0.1, 5)
    assert np.array_equal(a != 0, R.keep(5, R.attention_index(2, 2, 61), 0.1))


@pytest.mark.parametrize("p", [0.05, 0.1, 0.25, 0.5, 0.9])
def test_statistics(p):
    n = 2 ** 20
    q = 1.0 - R.threshold(p) / 65536.0
    worst = 0.0

    def sigma(what, z):
        nonlocal worst
        worst = max(worst, abs(z))
        assert abs(z) <= 5.0, f"p {p}: {what} is {z:.2f} standard errors off"

    for seed in R.SEEDS:
        k = R.keep_range(n, p, seed).astype(np.float64)
        sigma(f"seed {seed} keep rate", (k.mean() - q) / np.sqrt(q * (1 - q) / n))
        for lane in range(4):
            sigma(f"seed {seed} lane {lane}", (k[lane::4].mean() - q) / np.sqrt(q * (1 - q) / (n / 4)))
        c = (k - q) / np.sqrt(q * (1 - q))                                 # centred on the expectation, unit variance
        for lag in (1, 2, 3, 4, 5, 512, 2048):
            sigma(f"seed {seed} lag {lag}", float(np.mean(c[:-lag] * c[lag:])) * np.sqrt(n - lag))
        k1 = R.keep_range(n, p, (seed + 1) & R.MASK64).astype(np.float64)
        sigma(f"seeds {seed}, {seed} + 1", float(np.mean(c * (k1 - q) / np.sqrt(q * (1 - q)))) * np.sqrt(n))
    print(f"p {p}: worst {worst:.2f} sigma")


# ---- the device equality tests discriminate ---------------------------------------------------------------------------------
def test_reversed_lane_order_differs():
    """Lane 3 - (idx & 3) instead of idx & 3: another mask in every stand-alone case of at least 1024 elements at p = 0.1, 0.25
    and 0.5 (p = 2^-16 and 0.99998 drop or keep one element in 65536: there the 2^20 case shows it), and in every GEMM and
    attention case."""
    rev = (3, 2, 1, 0)
    for seed in R.SEEDS:
        for p in R.STANDALONE_P:
            th = R.threshold(p)
            for n in R.STANDALONE_SIZES:
                differs = bool(((R.bits_range(seed, n) >= th) != (R.bits_range(seed, n, lane_order=rev) >= th)).any())
                if (n >= 1024 and p in (0.1, 0.25, 0.5)) or n == 2 ** 20:
                    assert differs, (seed, p, n)
    th = R.threshold(R.SITE_P)
    for seed in R.SITE_SEEDS:
        for M, N in R.gemm_shapes():
            if M * N >= 64:
                assert ((R.bits_range(seed, M * N) >= th) != (R.bits_range(seed, M * N, lane_order=rev) >= th)).any(), (seed, M, N)
        for B, H, T in R.ATTENTION:
            n = B * H * T * T
            assert ((R.bits_range(seed, n) >= th) != (R.bits_range(seed, n, lane_order=rev) >= th)).any(), (seed, B, H, T)


def test_floor_threshold_differs_only_from_2_to_the_20_on():
    """floor(65536 p) = 6553 against ceil = 6554 at p = 0.1: the masks differ where the 16 bits equal 6553, one element in 65536.
    The stand-alone case of 2^20 elements shows it for every seed (16 expected); the four-element case cannot.  The large GEMM
    cells (10^7 elements) show it at the sites' seeds as well."""
    lo, hi = R.threshold(0.1, np.floor), R.threshold(0.1)
    assert (lo, hi) == (6553, 6554)
    for seed in R.SEEDS:
        b = R.bits_range(seed, 2 ** 20)
        assert ((b >= lo) != (b >= hi)).any(), seed
        assert not ((b[:4] >= lo) != (b[:4] >= hi)).any()
    for seed in R.SITE_SEEDS:
        for cell in ("n128>=3072", "690<n128<=768", "n128>=769", "K>=2048", "K>=4096"):
            M, N = R.GEMM_F32[cell][:2]
            b = R.bits_range(seed, M * N)
            assert ((b >= lo) != (b >= hi)).any(), (seed, cell)
        M, N = R.GEMM_16["128x128"][:2]
        b = R.bits_range(seed, M * N)
        assert ((b >= lo) != (b >= hi)).any(), seed


def test_leading_dimension_index_differs():
    """row * ldc + col with ldc = N rounded up past N (the next multiple of 4 above it): another mask for every GEMM case of
    more than one row."""
    th = R.threshold(R.SITE_P)
    for seed in R.SITE_SEEDS:
        for M, N in R.gemm_shapes():
            if M == 1:
                continue
            rows = np.unique(np.concatenate([np.arange(min(M, 300)), np.arange(max(M - 300, 0), M)])).astype(np.uint64)
            cols = np.arange(N, dtype=np.uint64)[None, :]
            right = R.bits(seed, rows[:, None] * np.uint64(N) + cols) >= th
            wrong = R.bits(seed, rows[:, None] * np.uint64(N // 4 * 4 + 4) + cols) >= th
            assert (right != wrong).any(), (seed, M, N)
            assert np.array_equal(right, R.keep_range(M * N, R.SITE_P, seed).reshape(M, N)[rows.astype(np.int64)])
