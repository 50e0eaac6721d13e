"""The dropout mask restated in exact integers (numpy, no torch kernels): the contract that the comment above `dropout_hash`
in csrc/cfm_common.h states, written a second time outside the code under test.

The mask is a pure function of (seed, flat index, p):
  * one splitmix64 finaliser per ALIGNED group of four elements, `hash64(seed, idx >> 2)`;
  * element idx takes 16 of its 64 bits, lane `idx & 3` counted from the least significant end;
  * the element is dropped iff those bits are below `threshold(p) = ceil(float32(p) * 65536)`;
  * a kept element is scaled by `float32(1) / (float32(1) - float32(p))`.

The flat index of every site is the C-order index of the tensor the mask multiplies:
  * GEMM results (the fused epilogues, the stand-alone kernel, the replay in the backward): `row * N + col` with the
    LOGICAL width N, never the leading dimension (`gemm_index`);
  * attention probabilities: `((b * H + h) * T + i) * T + k` (`attention_index`).

`hash64(0, 0) == 0`: the finaliser maps 0 to 0, so seed 0 drops elements 0..3 for any p > 0.  The sites pass seed 0 only
together with p == 0 (ops.new_seeds never returns it in practice: a 62-bit mix of the generator state).

The lists at the end are the cases tests/test_dropout_sites_gpu.py compares with the device bit for bit;
tests/test_dropout_restatement_cpu.py shows on the same cases that a swapped lane order, a floor in the threshold and a
leading-dimension index each give another mask.
"""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1
_U = np.uint64


def hash64(seed, group):
    """splitmix64's finaliser of `seed + group * GOLDEN`, everything mod 2^64.  group: an int or an integer array."""
    g = np.asarray(group).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = _U(int(seed) & MASK64) + g * _U(GOLDEN)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))


def bits(seed, idx):
    """The 16 bits of element `idx` (an int or an integer array of flat indices)."""
    i = np.asarray(idx).astype(np.uint64)
    return ((hash64(seed, i >> _U(2)) >> (_U(16) * (i & _U(3)))) & _U(0xFFFF)).astype(np.uint32)


def bits_range(seed, n, start=0, lane_order=(0, 1, 2, 3)):
    """bits(seed, start + arange(n)) with one hash per group (the same shift and mask, evaluated group by group in chunks so
    that a 5e7-element mask stays within a few hundred megabytes).  lane_order: which 16-bit lane element idx & 3 takes --
    (0, 1, 2, 3) is the contract; the CPU tests pass (3, 2, 1, 0) as a wrong variant."""
    g0, g1 = start >> 2, (start + n + 3) >> 2
    out = np.empty(4 * (g1 - g0), dtype=np.uint16)
    sh = (_U(16) * np.asarray(lane_order, dtype=np.uint64))[None, :]
    step = 1 << 20
    for a in range(g0, g1, step):
        b = min(a + step, g1)
        z = hash64(seed, np.arange(a, b, dtype=np.uint64))
        out[4 * (a - g0):4 * (b - g0)] = ((z[:, None] >> sh) & _U(0xFFFF)).astype(np.uint16).reshape(-1)
    off = start - 4 * g0
    return out[off:off + n]


def threshold(p, rounding=np.ceil):
    """ceil(float32(p) * 65536): the product is exact in fp32 (a power-of-two scale)."""
    return int(rounding(np.float32(p) * np.float32(65536.0)))


def inv_keep(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep(seed, idx, p):
    """Boolean: element idx is kept."""
    return bits(seed, idx) >= threshold(p)


def keep_range(n, p, seed, start=0):
    """keep(seed, start + arange(n), p)."""
    return bits_range(seed, n, start) >= threshold(p)


def mask(shape, p, seed):
    """fp32 array of `shape`: 0 or float32(1) / (float32(1) - float32(p)), over the C-order flat index."""
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    n = int(np.prod(shape, dtype=np.int64))
    return np.where(keep_range(n, p, seed), inv_keep(p), np.float32(0.0)).astype(np.float32).reshape(shape)


def gemm_index(M, N, ld=None):
    """(M, N) array of flat indices row * N + col; ld: a WRONG variant that counts rows in leading dimensions."""
    r = np.arange(M, dtype=np.uint64)[:, None]
    return r * _U(N if ld is None else ld) + np.arange(N, dtype=np.uint64)[None, :]


def attention_index(B, H, T):
    """(B, H, T, T) array of flat indices ((b * H + h) * T + i) * T + k."""
    b = np.arange(B, dtype=np.uint64)[:, None, None, None]
    h = np.arange(H, dtype=np.uint64)[None, :, None, None]
    i = np.arange(T, dtype=np.uint64)[None, None, :, None]
    k = np.arange(T, dtype=np.uint64)[None, None, None, :]
    return ((b * _U(H) + h) * _U(T) + i) * _U(T) + k


# ---- the cases of the device equality tests (tests/test_dropout_sites_gpu.py) ----------------------------------------------
SEEDS = (0, 1, 12345, 2 ** 63 + 5, 2 ** 64 - 1)
STANDALONE_SIZES = (4, 8, 1024, 1032, 2 ** 20)
STANDALONE_P = (2.0 ** -16, 0.1, 0.25, 0.5, 0.99998)
SITE_P = 0.1
SITE_SEEDS = (12345, 2 ** 63 + 5)

# fp32 training GEMM, one shape per cell of F32_CELLS (tests/test_property_gemm_gpu.py) that serves bias / Swish / residual:
# the smallest M and N of the cell, the first K listed there (a power of two): cell -> (M, N, K, epilogues, (BM, BN))
GEMM_F32 = {
    "n128>=3072": (11905, 4097, 16, ("bias",), (128, 128)),
    "690<n128<=768": (7297, 1409, 16, ("bias", "swish", "residual"), (128, 128)),
    "n128>=769": (7297, 1665, 16, ("bias", "swish", "residual"), (128, 64)),
    "K>=2048": (7105, 385, 2048, ("bias", "swish", "residual"), (64, 128)),
    "K>=4096": (7041, 449, 4096, ("bias", "residual"), (128, 64)),
    "default": (1, 1, 4, ("bias", "swish", "residual"), (64, 64)),
}
# Every smallest N above is 1 mod 4: the per-element epilogue.  The vectorised epilogue (N % 4 == 0, one hash per four columns:
# what a training step runs) in the same big tiles, three columns further into the cell: cell -> N
GEMM_F32_VEC = {"690<n128<=768": 1412, "n128>=769": 1668, "K>=2048": 388, "K>=4096": 452}
# 16-bit training GEMM: cell of TILE16 -> (M, N, K).  Forced tiles: ragged in M, more than one tile either way at 64 / 128 rows,
# N % 8 == 0 (16-bit C and Z), K % 8 == 0 (16-bit W: the 8-wave tiles take nothing else); the 128x128 tile by shape (t128 = 527).
GEMM_16 = {
    "64x64": (333, 264, 64),
    "128x64": (333, 264, 64),
    "128x128": (3841, 2056, 64),
    "256x128": (333, 264, 64),
    "256x256": (333, 264, 64),
}
# the per-element epilogue (N % 4 != 0): fp32 default tile and the 16-bit 64x64 tile
GEMM_ODD_N = ((300, 129, 16), (300, 130, 16), (300, 131, 16))
# attention probabilities: (B, H, T)
ATTENTION = ((2, 2, 61), (2, 2, 63), (2, 2, 64))


def gemm_shapes():
    """Every (M, N) whose mask the device tests compare."""
    shapes = [(c[0], c[1]) for c in GEMM_F32.values()] + [(c[0], c[1]) for c in GEMM_16.values()] + [(c[0], c[1]) for c in GEMM_ODD_N]
    shapes += [(GEMM_F32[cell][0], n) for cell, n in GEMM_F32_VEC.items()]
    return sorted(set(shapes))
