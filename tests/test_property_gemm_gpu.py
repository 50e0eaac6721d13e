"""Property-based sweep of the forward GEMMs along the block-tile dimension (the forward counterpart of
tests/test_property_train_gpu.py).

Three kernel families pick a block tile on the host from M, N and K, so the batch size and utterance length a caller picks decide
which kernel runs: the fp32 family (csrc/gemm_f32.hip choose_tile, split-K, the LayerNorm-fold producers and consumer), the 16-bit
family (csrc/gemm_mfma16.hip launch_t / launch_big) and the split-plane family (csrc/gemm_split.hip launch).  One test per
(family, tile) cell; hypothesis draws the raggedness inside the cell (derandomised: the same examples every run, one process)
and @example pins the threshold shapes.  Every call asserts the tile it recorded (cfm_debug_gemm_last_tile).

Reference: a float64 product (of the operands rounded to the 16-bit type for the 16-bit family).  Where M x N chooses the tile
K stays small, and for large M the reference covers a subset of rows that holds the first and the last row tile and every row
residue mod 256.  Besides rel-L2 over the checked rows, the last row tile and the last column tile are checked on their own (a
wrong last row of 24577 is invisible in the whole).  Exact properties (same MFMA, same k order, same epilogue in every tile)
are asserted bitwise.  The CPU tests at the end check that each plausible wrong answer misses its bound by 10x or more.
"""
import contextlib
import ctypes
import math

import pytest
import torch

hypothesis = pytest.importorskip("hypothesis")
from hypothesis import example, given, settings, strategies as st, HealthCheck  # noqa: E402

from tests.util import Calls, merged, ref_partials, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 2e-5                                  # fp32 and 16-bit families (16-bit: against the product of the rounded operands)
TOL_SPLIT = {3: 2e-6, 2: 1e-4}              # split-plane: bf16x6 / bf16x3 (tests/test_split_gpu.py)
DT16 = {1: torch.bfloat16, 2: torch.float16}
F32, F16, FSPLIT = 0, 1, 2                  # cfm_debug_gemm_last_tile families
EPI = {"bias": 0, "swish": 1, "relu": 2, "glu": 3, "resid": 4}
SET = dict(deadline=None, derandomize=True, suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conformer_amd import _lib, ops as _ops
    assert _lib.load().cfm_device_check() == 0, "not a gfx950 device"
    return _ops


def lib():
    from conformer_amd import _lib
    return _lib.load()


def last_tile(family):
    """(BM, BN, waves, K slices, operand form, 16-bit C) of the family's last launch; clears the record."""
    from conformer_amd import _lib
    out = (ctypes.c_int * 6)()
    _lib.check(lib().cfm_debug_gemm_last_tile(family, ctypes.addressof(out)), "cfm_debug_gemm_last_tile")
    return tuple(out)


def grnd(*shape, seed=0, scale=1.0, shift=0.0):
    """Device-side normal operand (big operands: no host generation, no copy)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, generator=g, device="cuda") * scale + shift


def check_rows(M):
    """Rows the float64 reference covers: all of them up to 1024; else the first 256 (every residue mod 256: the first row
    tile of every tile height), 64 in the middle and the last 256 (the last row tile of every tile height)."""
    if M <= 1024:
        return torch.arange(M)
    return torch.tensor(sorted(set(range(256)) | set(range(M // 2, M // 2 + 64)) | set(range(M - 256, M))))


def pick(lo, hi, q):
    """The value at q / 64 of [lo, hi] (q in 0..64): draws inside a cell that @example can pin."""
    return lo + (hi - lo) * q // 64


def epi_ref(epi, z, r=None, alpha=1.0):
    if epi == "bias":
        return z
    if epi == "swish":
        return z * torch.sigmoid(z)
    if epi == "relu":
        return torch.relu(z)
    if epi == "resid":
        return alpha * z + r
    n = z.shape[1] // 2
    return z[:, :n] * torch.sigmoid(z[:, n:])


def assert_close(c, ref, rows, M, bm, bn, tol, what=""):
    """rel-L2 of the checked rows, of the last row tile and of the last column tile (bm x bn: the tile's OUTPUT extent)."""
    got = c[rows.to(c.device)].double().cpu() if rows.numel() != M else c.double().cpu()
    n = ref.shape[1]
    e_all = rel_l2(got, ref)
    last_r = rows >= (M - 1) // bm * bm
    last_c = slice((n - 1) // bn * bn, n)
    e_row = rel_l2(got[last_r], ref[last_r])
    e_col = rel_l2(got[:, last_c], ref[:, last_c])
    assert e_all < tol and e_row < tol and e_col < tol, f"{what}: all {e_all:.2e} last row tile {e_row:.2e} last col tile {e_col:.2e}"


# ==== 16-bit family ==========================================================================================================
@contextlib.contextmanager
def force16(tile):
    lib().cfm_debug_gemm_mfma16_force_tile(tile)
    try:
        yield
    finally:
        lib().cfm_debug_gemm_mfma16_force_tile(0)


def gemm16(ops, prec, epi, a, w, b, form, res=None, alpha=1.0, c16=False):
    """cfm_gemm_mfma16_f32 with an explicit operand form: 0 = fp32 A and W, 1 = 16-bit W, 2 = 16-bit A (pre-rounded) and W."""
    from conformer_amd import _lib
    dt = DT16[prec]
    M, K = a.shape
    n = w.shape[0] // 2 if epi == "glu" else w.shape[0]
    A = a.to(dt) if form == 2 else a
    W = w.to(dt) if form >= 1 else w
    c = torch.empty(M, n, device="cuda", dtype=dt if c16 else torch.float32)
    st = lib().cfm_gemm_mfma16_f32(prec, EPI[epi], A.data_ptr(), int(form == 2), W.data_ptr(), int(form >= 1), b.data_ptr(),
                                   None if res is None else res.data_ptr(), alpha, c.data_ptr(), int(c16), None, 0, M, n, K, K, n, n,
                                   0.0, 0, ops._stream())
    _lib.check(st, "cfm_gemm_mfma16_f32")
    return c


def ref16(prec, a, w, b, rows):
    dt = DT16[prec]
    ar = a[rows.to(a.device)].to(dt).double().cpu()
    return ar @ w.to(dt).double().cpu().t() + b.double().cpu()


# cell -> (force_tile, expected (BM, BN, waves), epilogues, K % 8 == 0 required).  The 128x64 tile serves the bias and residual
# epilogues only (launch_t: force_tile 4 sends Swish / ReLU to 64x64); GLU takes its tiles by shape (test_mfma16_glu_tiles).
TILE16 = {
    "64x64": (5, (64, 64, 4), ("bias", "swish", "relu", "resid"), False),
    "128x64": (4, (128, 64, 4), ("bias", "resid"), False),
    "128x128": (1, (128, 128, 4), ("bias", "swish", "relu", "resid"), False),
    "256x128": (2, (256, 128, 8), ("bias", "swish", "relu", "resid"), True),
    "256x256": (3, (256, 256, 8), ("bias", "swish", "relu", "resid"), True),
}


def _run16_cell(ops, prec, cell, M, N, K, seed):
    force, tile, epis, need8 = TILE16[cell]
    forms = (0,) if K % 8 else ((0, 1, 2) if not need8 else (1, 2))
    a, w = grnd(M, K, seed=seed), grnd(N, K, seed=seed + 1, scale=1 / math.sqrt(K))
    b, r = grnd(N, seed=seed + 2), grnd(M, N, seed=seed + 3)
    rows = check_rows(M)
    z = ref16(prec, a, w, b, rows)
    rr = r[rows.to(r.device)].double().cpu()
    for epi in epis:
        res, alpha = (r, 0.75) if epi == "resid" else (None, 1.0)
        with force16(5):
            base = gemm16(ops, prec, epi, a, w, b, 0, res, alpha)              # the 64x64 tile on fp32 operands
        assert last_tile(F16)[:3] == (64, 64, 4)
        ref = epi_ref(epi, z, rr, alpha)
        for form in forms:
            with force16(force):
                c = gemm16(ops, prec, epi, a, w, b, form, res, alpha)
            rec = last_tile(F16)
            assert rec[:3] == tile and rec[4] == form, (cell, epi, form, rec)
            assert_close(c, ref, rows, M, tile[0], tile[1], TOL, f"{cell} {epi} form {form}")
            # same MFMA, same k order, same epilogue in every tile; staging rounds to nearest-even as torch does
            assert torch.equal(c, base), f"{cell} {epi} form {form}: bits differ from the 64x64 tile on fp32 operands"
            if epi != "resid" and N % 8 == 0:
                with force16(force):
                    c16 = gemm16(ops, prec, epi, a, w, b, form, c16=True)
                rec = last_tile(F16)
                assert rec[:3] == tile and rec[5] == 1
                assert torch.equal(c16, c.to(DT16[prec])), f"{cell} {epi} form {form}: 16-bit C != fp32 C rounded"


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("cell", ["64x64", "128x64", "256x128", "256x256"])
@settings(max_examples=3, **SET)
@given(M=st.integers(1, 700), N4=st.integers(1, 100), K=st.integers(1, 40).map(lambda k: 4 * k), odd_n=st.booleans(),
       seed=st.integers(0, 10 ** 6))
@example(M=257, N4=72, K=132, odd_n=False, seed=1).via("ragged in M, K % 8 == 4 (fp32 W)")
@example(M=511, N4=65, K=136, odd_n=False, seed=2).via("one row short of two 256-row tiles; N % 8 == 4")
@example(M=300, N4=33, K=200, odd_n=True, seed=3).via("N = 131: the per-element epilogue, 16-bit operands")
def test_mfma16_forced_tiles(ops, prec, cell, M, N4, K, odd_n, seed):
    """Each forced tile with every epilogue it serves and every operand form its inputs allow: float64 of the rounded operands,
    the same bits as the 64x64 tile, 16-bit C == fp32 C rounded.  odd_n: N % 4 == 3, the per-element epilogue (4-wave tiles
    only: the 8-wave tiles need the vectorised one and fall back, test_mfma16_big_tile_fallbacks)."""
    N = 4 * N4 - (1 if odd_n and not TILE16[cell][3] else 0)
    if TILE16[cell][3] and K % 8:
        K += 4                                                    # the 8-wave tiles take 16-bit weights only
    _run16_cell(ops, prec, cell, M, N, K, seed)


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@settings(max_examples=2, **SET)
@given(M=st.integers(3841, 4200), N4=st.integers(513, 530), K=st.integers(1, 12).map(lambda k: 8 * k), odd_n=st.booleans(),
       seed=st.integers(0, 10 ** 6))
@example(M=3841, N4=513, K=68, odd_n=False, seed=3).via("t128 = 31 x 17 = 527 >= 512 (last row tile of one row); fp32 W")
@example(M=4095, N4=515, K=72, odd_n=False, seed=4).via("16-bit W and A, N % 8 == 4")
@example(M=3900, N4=520, K=96, odd_n=True, seed=5).via("16-bit W with N % 4 != 0: where autocast reaches this tile")
def test_mfma16_128x128_tile(ops, prec, M, N4, K, odd_n, seed):
    """The 128x128 tile is reached by shape (t128 >= 512) with force_tile 1 keeping the 8-wave tiles out; every operand form
    (K % 8 == 0) and the per-element epilogue (N % 4 != 0)."""
    _run16_cell(ops, prec, "128x128", M, 4 * N4 - (1 if odd_n else 0), K, seed)


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@settings(max_examples=3, **SET)
@given(M=st.integers(1, 3000), n32=st.integers(1, 40), K=st.integers(1, 40).map(lambda k: 8 * k), seed=st.integers(0, 10 ** 6))
@example(M=4000, n32=32, K=64, seed=4).via("GLU 128x128: t128 = 32 x 16 = 512")
@example(M=3968, n32=32, K=64, seed=5).via("GLU 64x128: t128 = 31 x 16 = 496")
def test_mfma16_glu_tiles(ops, prec, M, n32, K, seed):
    """GLU takes its tile by shape only (64x128 below t128 = 512, 128x128 from it): float64 of the rounded operands, and the
    rows of the large product bitwise equal to the same rows computed alone (the small product's 64x128 tile)."""
    n = 32 * n32 - (7 if seed % 2 else 0)                     # odd widths: the per-element epilogue (GLU stores n % 4 != 0)
    t128 = (M + 127) // 128 * ((n + 63) // 64)
    tile = (128, 128, 4) if t128 >= 512 else (64, 128, 4)
    a, w, b = grnd(M, K, seed=seed), grnd(2 * n, K, seed=seed + 1, scale=1 / math.sqrt(K)), grnd(2 * n, seed=seed + 2)
    rows = check_rows(M)
    ref = epi_ref("glu", ref16(prec, a, w, b, rows))
    sub = a[rows.to(a.device)].contiguous()
    c_sub = gemm16(ops, prec, "glu", sub, w, b, 0)
    assert last_tile(F16)[:3] == ((64, 128, 4) if (rows.numel() + 127) // 128 * ((n + 63) // 64) < 512 else (128, 128, 4))
    for form in (0, 1, 2):
        c = gemm16(ops, prec, "glu", a, w, b, form)
        rec = last_tile(F16)
        assert rec[:3] == tile and rec[4] == form, rec
        assert_close(c, ref, rows, M, tile[0], tile[1] // 2, TOL, f"GLU form {form}")
        assert torch.equal(c[rows.to(c.device)], c_sub), f"GLU form {form}: the tile changed the bits"


# force_tile 0 on both sides of every threshold of launch_t: (M, N, K, form, epi) -> (BM, BN, waves)
THRESH16 = [
    ((7936, 1536, 64, 1, "swish"), (256, 128, 8)),   # t256 = 31 x 6 = 186 < 190; t2128 = 372 >= 224
    ((7937, 1536, 64, 1, "swish"), (256, 256, 8)),   # t256 = 32 x 6 = 192 (the B = 32 fused QKV product)
    ((14080, 512, 1024, 1, "resid"), (128, 64, 4)),  # t2128 = 55 x 4 = 220 < 224; t12864 = 880, K >= 1024
    ((14081, 512, 1024, 1, "resid"), (256, 128, 8)), # t2128 = 56 x 4 = 224
    ((3840, 2052, 68, 0, "relu"), (64, 64, 4)),      # fp32 W: t128 = 30 x 17 = 510 < 512
    ((3841, 2052, 68, 0, "relu"), (128, 128, 4)),    # t128 = 31 x 17 = 527
    ((7040, 512, 1028, 0, "bias"), (64, 64, 4)),     # t12864 = 55 x 8 = 440 < 448
    ((7041, 512, 1028, 0, "bias"), (128, 64, 4)),    # t12864 = 56 x 8 = 448 (FFN out at B = 32: M = 7968)
    ((7968, 512, 1020, 0, "resid"), (64, 64, 4)),    # K = 1020 < 1024
    ((7968, 512, 2048, 1, "resid"), (128, 64, 4)),   # the FFN out product of the benchmark
]


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case,tile", THRESH16, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c, _ in THRESH16])
def test_mfma16_auto_thresholds(ops, prec, case, tile):
    M, N, K, form, epi = case
    a, w = grnd(M, K, seed=M), grnd(N, K, seed=N, scale=1 / math.sqrt(K))
    b, r = grnd(N, seed=K), grnd(M, N, seed=M + 1)
    res, alpha = (r, 0.5) if epi == "resid" else (None, 1.0)
    c = gemm16(ops, prec, epi, a, w, b, form, res, alpha)
    rec = last_tile(F16)
    assert rec[:3] == tile, rec
    rows = check_rows(M)
    ref = epi_ref(epi, ref16(prec, a, w, b, rows), r[rows.to(r.device)].double().cpu(), alpha)
    assert_close(c, ref, rows, M, tile[0], tile[1], TOL, str(case))
    with force16(5):
        base = gemm16(ops, prec, epi, a, w, b, form, res, alpha)
    assert torch.equal(c, base)


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("force", [2, 3])
@pytest.mark.parametrize("why", ["n_mod4", "fp32_w"])
def test_mfma16_big_tile_fallbacks(ops, prec, force, why):
    """force_tile 2 / 3 with N % 4 != 0 (no vectorised epilogue) or an fp32 W falls back to a 4-wave tile, with the right result."""
    M, N, K = (333, 130, 72) if why == "n_mod4" else (333, 132, 68)
    N = N + 1 if why == "n_mod4" else N
    a, w, b = grnd(M, K, seed=7), grnd(N, K, seed=8, scale=1 / math.sqrt(K)), grnd(N, seed=9)
    with force16(force):
        c = gemm16(ops, prec, "bias", a, w, b, 1 if K % 8 == 0 else 0)
    rec = last_tile(F16)
    assert rec[:3] == (64, 64, 4), rec
    rows = torch.arange(M)
    assert_close(c, ref16(prec, a, w, b, rows), rows, M, 64, 64, TOL, f"fallback {why}")


# ==== fp32 family ============================================================================================================
CFG = {0: (128, 128), 1: (128, 64), 2: (64, 128), 3: (64, 64)}


def cfg_gemm(ops, cfg, epi, a, w, b, r, alpha):
    from conformer_amd import _lib
    M, K = a.shape
    N = w.shape[0]
    c = torch.empty(M, N, device="cuda")
    code = cfg + {"resid": 0, "bias": 16, "swish": 32}[epi]
    _lib.check(lib().cfm_debug_gemm_cfg_f32(code, a.data_ptr(), w.data_ptr(), b.data_ptr(), r.data_ptr(), alpha, c.data_ptr(), M, N, K,
                                            None, ops._stream()), "cfm_debug_gemm_cfg_f32")
    return c


@settings(max_examples=6, **SET)
@given(M=st.integers(1, 400), N=st.integers(1, 300), K4=st.integers(1, 200), seed=st.integers(0, 10 ** 6))
@example(M=129, N=65, K4=1, seed=1).via("one row and one column past a 128 / 64 tile; K = 4")
@example(M=64, N=64, K4=3, seed=2).via("K = 12: one partial K-tile")
def test_f32_forced_cfgs_bitwise(ops, M, N, K4, seed):
    """The four tiles forced through cfm_debug_gemm_cfg_f32 (residual, bias, Swish): float64, and the same bits for every cfg
    and for the production entry ("same results for every cfg")."""
    K = 4 * K4
    a, w = grnd(M, K, seed=seed), grnd(N, K, seed=seed + 1, scale=1 / math.sqrt(K))
    b, r = grnd(N, seed=seed + 2), grnd(M, N, seed=seed + 3)
    rows = torch.arange(M)
    z = a.double().cpu() @ w.double().cpu().t() + b.double().cpu()
    for epi in ("resid", "bias", "swish"):
        prod = ops.linear_residual(a, w, b, r, 0.25) if epi == "resid" else ops.linear(a, w, b, act="swish" if epi == "swish" else "none")
        last_tile(F32)
        ref = epi_ref(epi, z, r.double().cpu(), 0.25)
        for cfg, (bm, bn) in CFG.items():
            c = cfg_gemm(ops, cfg, epi, a, w, b, r, 0.25)
            rec = last_tile(F32)
            assert rec[:4] == (bm, bn, 4, 1), rec
            assert_close(c, ref, rows, M, bm, bn, TOL, f"cfg {cfg} {epi}")
            assert torch.equal(c, prod), f"cfg {cfg} {epi}: bits differ from the production entry"


def f32_call(ops, epi, a, w, b, r=None, alpha=1.0):
    if epi == "glu":
        return ops.linear_glu(a, w, b)
    if epi == "resid":
        return ops.linear_residual(a, w, b, r, alpha)
    return ops.linear(a, w, b, act={"bias": "none"}.get(epi, epi))


# choose_tile by shape, through ops: cell -> (M range, N range (output columns), K choices, epilogues, (BM, BN) of the product).
# K stays below 1024 where the product is small enough for split-K (test_splitk_every_slice_count).
F32_CELLS = {
    "n128>=3072": ((11905, 11968), (4097, 4200), (16,), ("bias", "relu"), (128, 128)),
    "690<n128<=768": ((7297, 8192), (1409, 1536), (16, 132), ("bias", "swish", "relu", "resid"), (128, 128)),
    "n128>=769": ((7297, 8192), (1665, 2100), (16, 132), ("bias", "swish", "relu", "resid"), (128, 64)),
    "K>=2048": ((7105, 8000), (385, 512), (2048,), ("bias", "swish", "relu", "resid"), (64, 128)),
    "K>=4096": ((7041, 7104), (449, 512), (4096,), ("bias", "resid"), (128, 64)),
    "default": ((1, 2500), (1, 520), (4, 132, 1020), ("bias", "swish", "relu", "resid"), (64, 64)),
    "glu_default": ((1, 3000), (1, 520), (8, 132), ("glu",), (64, 128)),
    "glu_n128>=3072": ((12161, 12200), (2017, 2100), (16,), ("glu",), (128, 128)),
}


@pytest.mark.parametrize("cell", list(F32_CELLS))
@settings(max_examples=2, **SET)
@given(mq=st.integers(0, 64), nq=st.integers(0, 64), kq=st.integers(0, 2), seed=st.integers(0, 10 ** 6))
@example(mq=64, nq=64, kq=2, seed=1).via("the largest M and N of the cell")
@example(mq=0, nq=37, kq=0, seed=2).via("the smallest M, a ragged N")
@example(mq=23, nq=0, kq=1, seed=3).via("a ragged M, the smallest N")
def test_f32_tiles_by_shape(ops, cell, mq, nq, kq, seed):
    """Every branch of choose_tile through the ops entry points (relu and GLU are reachable only this way)."""
    (mlo, mhi), (nlo, nhi), Ks, epis, tile = F32_CELLS[cell]
    M, N, K = pick(mlo, mhi, mq), pick(nlo, nhi, nq), Ks[kq % len(Ks)]
    glu = epis == ("glu",)
    a = grnd(M, K, seed=seed)
    w = grnd(2 * N if glu else N, K, seed=seed + 1, scale=1 / math.sqrt(K))
    b = grnd(w.shape[0], seed=seed + 2)
    r = grnd(M, N, seed=seed + 3)
    rows = check_rows(M)
    z = a[rows].double().cpu() @ w.double().cpu().t() + b.double().cpu()
    rr = r[rows.to(r.device)].double().cpu()
    for epi in epis:
        c = f32_call(ops, epi, a, w, b, r, 0.5)
        rec = last_tile(F32)
        assert rec[:4] == (*tile, 4, 1), (cell, epi, M, N, K, rec)
        assert_close(c, epi_ref(epi, z, rr, 0.5), rows, M, tile[0], tile[1] // (2 if glu else 1), TOL, f"{cell} {epi} {M}x{N}x{K}")


# ---- LayerNorm-fold producers (emit_stats=True): tile bands per N (the producer serves N in {32, ..., 512}, any K) ------------
def producer_band(tile, N):
    """M range of the cell at width N (K is 2048 for the 64x128 cell, small otherwise)."""
    nt = (N + 127) // 128
    if tile == "64x64":
        return 1, 2000
    if tile == "64x128":                                   # ceil(M/64) * nt >= 448, n128 <= 690
        return 64 * (-(-448 // nt) - 1) + 1, min(128 * (690 // nt), 64 * (-(-448 // nt) - 1) + 4000)
    if tile == "128x128":                                  # 690 < n128 <= 768
        return 128 * ((690 // nt + 1) - 1) + 1, 128 * (768 // nt)
    return 128 * (768 // nt) + 1, 128 * (768 // nt) + 4000   # 128x64: n128 >= 769


@pytest.mark.parametrize("N", [32, 64, 128, 256, 512])
@pytest.mark.parametrize("tile", ["64x64", "64x128", "128x128", "128x64"])
@settings(max_examples=1, **SET)
@given(off=st.integers(0, 300), seed=st.integers(0, 10 ** 6))
@example(off=0, seed=1).via("the first M of the band")
@example(off=300, seed=2).via("the last M of the band")
def test_lnfold_producers_every_tile(ops, tile, N, off, seed):
    """linear / linear_residual with emit_stats=True in each tile at N = 32 .. 512: C bitwise equal to the plain call, partials
    within the bounds of test_lnfold_gpu.py, C against float64."""
    lo, hi = producer_band(tile, N)
    M = min(lo + off, hi) if off < 290 else hi
    K = 2048 if tile == "64x128" else 36
    bm, bn = {"64x64": (64, 64), "64x128": (64, 128), "128x128": (128, 128), "128x64": (128, 64)}[tile]
    a, w = grnd(M, K, seed=seed), grnd(N, K, seed=seed + 1, scale=1 / math.sqrt(K))
    b, r = grnd(N, seed=seed + 2), grnd(M, N, seed=seed + 3, scale=2.0, shift=0.7)
    rows = check_rows(M)
    z = a[rows].double().cpu() @ w.double().cpu().t() + b.double().cpu()
    for resid in (False, True):
        c0 = ops.linear_residual(a, w, b, r, 0.5) if resid else ops.linear(a, w, b)
        rec0 = last_tile(F32)
        c1, st_ = ops.linear_residual(a, w, b, r, 0.5, emit_stats=True) if resid else ops.linear(a, w, b, emit_stats=True)
        rec = last_tile(F32)
        assert rec[:4] == (bm, bn, 4, 1) and rec0 == rec, (tile, M, N, rec0, rec)
        assert torch.equal(c0, c1)
        ref = 0.5 * z + r[rows.to(r.device)].double().cpu() if resid else z
        assert_close(c1, ref, rows, M, bm, bn, TOL, f"producer {tile} {M}x{N}")
        got = c1[rows.to(c1.device)].cpu()
        sp = st_[rows.to(st_.device)].cpu()
        rp = ref_partials(got, 32)
        assert rel_l2(sp[..., 0], rp[..., 0]) < 1e-6 and rel_l2(sp[..., 1], rp[..., 1]) < 1e-5
        last = rows >= (M - 1) // bm * bm                                    # the ragged last row tile on its own
        assert rel_l2(sp[last][..., 1], rp[last][..., 1]) < 1e-5
        mean, var = merged(sp, N)
        assert rel_l2(var, got.double().var(-1, unbiased=False)) < 1e-5
        assert float((mean - got.double().mean(-1)).abs().max()) < 1e-5


# ---- LayerNorm-fold consumer (linear_lnfold: bias, Swish, GLU; K = d <= 512, so never the non-GLU 64x128 tile) ---------------
LNC_CELLS = {  # cell -> (M range, N range (output columns), epilogues, (BM, BN) of the output)
    "64x64": ((1, 1500), (4, 400), ("bias", "swish"), (64, 64)),
    "128x128": ((7937, 8064), (1284, 1536), ("bias", "swish"), (128, 128)),
    "128x64": ((7937, 8064), (1540, 2100), ("bias", "swish"), (128, 64)),
    "glu_64x128": ((1, 1500), (4, 400), ("glu",), (64, 64)),
    "glu_128x128": ((7937, 8064), (3076, 3100), ("glu",), (128, 64)),
}


@pytest.mark.parametrize("d", [32, 64, 128, 256, 512])
@pytest.mark.parametrize("cell", list(LNC_CELLS))
@settings(max_examples=1, **SET)
@given(mq=st.integers(0, 64), nq=st.integers(0, 64), shift=st.floats(-1.5, 1.5), seed=st.integers(0, 10 ** 6))
@example(mq=64, nq=29, shift=1.5, seed=1).via("row means 1.5 x their spread")
@example(mq=17, nq=64, shift=-1.5, seed=2).via("row means -1.5 x their spread")
def test_lnfold_consumer_every_tile(ops, cell, d, mq, nq, shift, seed):
    """act(LN(x).W^T + b) from x's statistics: d/32 partials from a producer GEMM and one partial from the LayerNorm kernel, rows
    whose mean is of the order of their spread; float64 LayerNorm + Linear."""
    import torch.nn.functional as F
    (mlo, mhi), (nlo, nhi), epis, (bm, bn) = LNC_CELLS[cell]
    M, N = pick(mlo, mhi, mq), 4 * pick(nlo // 4, nhi // 4, nq)
    glu = epis == ("glu",)
    x0 = grnd(M, d, seed=seed, scale=1.7, shift=1.7 * shift)
    gam, bet = grnd(d, seed=seed + 1, scale=0.3, shift=1.0), grnd(d, seed=seed + 2, scale=0.2)
    w, b = grnd(2 * N if glu else N, d, seed=seed + 3, scale=1 / math.sqrt(d)), grnd(2 * N if glu else N, seed=seed + 4)
    wf, bf, cs = ops.fold_layernorm(w, b, gam, bet)
    x, st_prod = ops.linear_residual(torch.zeros(M, 16, device="cuda"), torch.zeros(d, 16, device="cuda"), torch.zeros(d, device="cuda"),
                                     x0, 1.0, emit_stats=True)               # identity through the residual epilogue
    g1, b1 = grnd(d, seed=seed + 5, scale=0.5, shift=1.0), grnd(d, seed=seed + 6, scale=0.1, shift=shift)
    xl, st_ln = ops.layernorm(x0, g1, b1, emit_stats=True)                 # one partial per row; mean ~ shift
    rows = check_rows(M)
    for xin, stats in ((x, st_prod), (xl, st_ln)):
        xr = xin[rows.to(xin.device)].double().cpu()
        z = F.layer_norm(xr, (d,), gam.double().cpu(), bet.double().cpu(), 1e-5) @ w.double().cpu().t() + b.double().cpu()
        for epi in epis:
            c = ops.linear_lnfold(xin, stats, wf, bf, cs, 1e-5, act="swish" if epi == "swish" else "none", glu=glu)
            rec = last_tile(F32)
            assert rec[:4] == (bm, bn * (2 if glu else 1), 4, 1), (cell, M, N, d, rec)
            assert_close(c, epi_ref(epi, z), rows, M, bm, bn, TOL, f"consumer {cell} {epi} parts {stats.shape[1]}")


# ---- split-K ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp", [2, 3, 4, 5, 6, 7, 8])
@settings(max_examples=2, **SET)
@given(r4=st.integers(0, 127), M=st.integers(1, 700), N4=st.integers(1, 40), seed=st.integers(0, 10 ** 6))
@example(r4=1, M=300, N4=128, seed=1).via("K = 512 sp + 4: the last slice is short (sp = 2: 528 and 500)")
@example(r4=3, M=1536, N4=128, seed=3).via("the most tiles split-K takes at this slice count (192 for sp <= 4)")
@example(r4=2, M=129, N4=3, seed=4).via("K % 16 == 8")
def test_splitk_every_slice_count(ops, sp, r4, M, N4, seed):
    """Every slice count _splitk can return (2..8), a short last slice, bias / Swish / residual: float64, the route and the
    slice count the launch recorded, and the same bits run to run."""
    K = 512 * sp + 4 * r4                                      # K // 512 == sp
    N = 4 * N4
    cap = min(192, 768 // sp)                                  # tiles <= cap: the product is small enough to take sp slices
    if ((M + 63) // 64) * ((N + 63) // 64) > cap:
        M = 64 * (cap // ((N + 63) // 64)) - 5                 # (ragged last row tile)
    rows = check_rows(M)
    assert ops._splitk(M, N, K) == sp
    a, w = grnd(M, K, seed=seed), grnd(N, K, seed=seed + 1, scale=1 / math.sqrt(K))
    b, r = grnd(N, seed=seed + 2), grnd(M, N, seed=seed + 3)
    z = a[rows].double().cpu() @ w.double().cpu().t() + b.double().cpu()
    rr = r[rows.to(r.device)].double().cpu()
    for epi in ("bias", "swish", "resid"):
        with Calls("cfm_gemm_splitk_f32") as seen:
            c = f32_call(ops, epi, a, w, b, r, 0.5)
        assert seen == {"cfm_gemm_splitk_f32"}
        rec = last_tile(F32)
        assert rec[:4] == (64, 64, 4, sp), (M, N, K, rec)
        assert_close(c, epi_ref(epi, z, rr, 0.5), rows, M, 64, 64, TOL, f"split-K {epi} {M}x{N}x{K}")
        assert torch.equal(c, f32_call(ops, epi, a, w, b, r, 0.5)), "split-K: the summing order is not fixed"


# ==== split-plane family =====================================================================================================
@contextlib.contextmanager
def fp32_matmul(ops, mode):
    prev = ops.set_fp32_matmul(mode)
    try:
        yield
    finally:
        ops.set_fp32_matmul(prev)


SPLIT_CELLS = {  # cell -> (M range, N range (output columns), epilogues, (BM, BN) of the output)
    "64x64": ((1, 1500), (1, 400), ("bias", "swish", "relu", "resid"), (64, 64)),
    "128x64": ((2945, 3072), (1025, 2048), ("bias", "resid"), (128, 64)),
    "128x128": ((2945, 3072), (2177, 2400), ("bias", "swish"), (128, 128)),
    "glu_64x128": ((1, 1500), (32, 320), ("glu",), (64, 64)),
    "glu_128x128": ((2945, 3072), (1088, 1120), ("glu",), (128, 64)),
}


@pytest.mark.parametrize("planes", [3, 2], ids=["bf16x6", "bf16x3"])
@pytest.mark.parametrize("cell", list(SPLIT_CELLS))
@settings(max_examples=2, **SET)
@given(mq=st.integers(0, 64), nq=st.integers(0, 64), K=st.integers(1, 12).map(lambda k: 16 * k), seed=st.integers(0, 10 ** 6))
@example(mq=64, nq=41, K=48, seed=1).via("the largest M, a ragged N")
@example(mq=13, nq=64, K=176, seed=2).via("a ragged M, the largest N")
def test_split_plane_every_tile(ops, planes, cell, mq, nq, K, seed):
    """64x64, 128x64, 128x128 and GLU 64x128 / 128x128 on split operands: ragged M and N, K % 16 == 0, GLU widths % 32 == 0."""
    (mlo, mhi), (nlo, nhi), epis, (bm, bn) = SPLIT_CELLS[cell]
    glu = epis == ("glu",)
    M = pick(mlo, mhi, mq)
    N = 32 * pick(nlo // 32, nhi // 32, nq) if glu else pick(nlo, nhi, nq)
    a = grnd(M, K, seed=seed)
    w = grnd(2 * N if glu else N, K, seed=seed + 1, scale=1 / math.sqrt(K))
    b, r = grnd(w.shape[0], seed=seed + 2), grnd(M, N, seed=seed + 3)
    rows = check_rows(M)
    z = a[rows].double().cpu() @ w.double().cpu().t() + b.double().cpu()
    rr = r[rows.to(r.device)].double().cpu()
    with fp32_matmul(ops, {3: "bf16x6", 2: "bf16x3"}[planes]):
        for epi in epis:
            c = f32_call(ops, epi, a, w, b, r, 0.5)
            rec = last_tile(FSPLIT)
            assert rec[:3] == (bm, bn * (2 if glu else 1), 4) and rec[4] == planes, (cell, M, N, rec)
            assert_close(c, epi_ref(epi, z, rr, 0.5), rows, M, bm, bn, TOL_SPLIT[planes], f"split {cell} {epi} {M}x{N}x{K}")


# ==== writes stay inside C: one example per tile, every allocation of the call guarded ======================================
GUARD = [  # (family, what, M, N, K, epi, setting, (BM, BN, waves))
    (F16, "16-bit 64x64", 333, 132, 72, "bias", 5, (64, 64, 4)),
    (F16, "16-bit 128x64", 333, 132, 72, "resid", 4, (128, 64, 4)),
    (F16, "16-bit 128x128", 3841, 2052, 64, "swish", 1, (128, 128, 4)),
    (F16, "16-bit 256x128", 333, 132, 72, "relu", 2, (256, 128, 8)),
    (F16, "16-bit 256x256", 333, 132, 72, "bias", 3, (256, 256, 8)),
    (F16, "16-bit GLU 64x128", 333, 132, 72, "glu", 0, (64, 128, 4)),
    (F16, "16-bit GLU 128x128", 4000, 1028, 64, "glu", 0, (128, 128, 4)),
    (F32, "fp32 64x64", 333, 130, 68, "resid", None, (64, 64, 4)),
    (F32, "fp32 128x64", 7297, 2050, 16, "bias", None, (128, 64, 4)),
    (F32, "fp32 128x128", 7297, 1534, 16, "swish", None, (128, 128, 4)),
    (F32, "fp32 64x128", 7105, 510, 2048, "relu", None, (64, 128, 4)),
    (F32, "fp32 GLU 64x128", 333, 130, 68, "glu", None, (64, 128, 4)),
    (F32, "fp32 GLU 128x128", 12161, 2046, 16, "glu", None, (128, 128, 4)),
    (F32, "fp32 split-K", 300, 132, 1028, "bias", None, (64, 64, 4)),
    (FSPLIT, "split 64x64", 333, 130, 64, "resid", "bf16x6", (64, 64, 4)),
    (FSPLIT, "split 128x64", 2945, 1030, 64, "bias", "bf16x6", (128, 64, 4)),
    (FSPLIT, "split 128x128", 2945, 2180, 64, "swish", "bf16x3", (128, 128, 4)),
    (FSPLIT, "split GLU 128x128", 2945, 1088, 64, "glu", "bf16x3", (128, 128, 4)),
]


@pytest.mark.parametrize("case", GUARD, ids=[g[1] for g in GUARD])
def test_writes_stay_inside_c(ops, case):
    from tests.test_write_guard_gpu import guarded_allocations
    family, what, M, N, K, epi, setting, tile = case
    glu = epi == "glu"
    a = grnd(M, K, seed=M)
    w = grnd(2 * N if glu else N, K, seed=N, scale=1 / math.sqrt(K))
    b, r = grnd(w.shape[0], seed=K), grnd(M, N, seed=M + 1)
    ctx = (torch.autocast("cuda", dtype=torch.bfloat16) if family == F16 else
           fp32_matmul(ops, setting) if family == FSPLIT else contextlib.nullcontext())
    with guarded_allocations() as gt, ctx, (force16(setting) if family == F16 else contextlib.nullcontext()):
        c = f32_call(ops, epi, a, w, b, r, 0.5)
        rec = last_tile(family)
        bad = gt.check()
    assert rec[:3] == tile, (what, rec)
    assert len(gt.allocs) >= 1 and not bad, f"{what}: {bad}"
    assert c.shape == (M, N) and bool(torch.isfinite(c).all())


# ==== the bounds are tight enough (CPU, float64) ============================================================================
def _rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_bounds_discriminate_dropped_k_tile_and_edges():
    """The last K-tile (16 deep: fp32; 64 deep: 16-bit) left out, and a last row / last column left out of the edge tiles."""
    M, N, K = 300, 130, 1028
    a, w = _rnd(M, K, seed=1), _rnd(N, K, seed=2) / math.sqrt(K)
    ref = a @ w.t()
    for tail in (4, 16, 64):                                  # K % 16 == 4: the short last tile of 4; whole 16 / 64-deep tiles
        wrong = a[:, :K - tail] @ w[:, :K - tail].t()
        assert rel_l2(wrong, ref) > 10 * TOL, tail
    rows = torch.arange(M)
    for bm, bn in ((64, 64), (128, 128), (256, 256)):
        wrong = ref.clone()
        wrong[-1] = 0
        last_r = rows >= (M - 1) // bm * bm
        assert rel_l2(wrong[last_r], ref[last_r]) > 10 * TOL
        wrong = ref.clone()
        wrong[:, -1] = 0
        last_c = slice((N - 1) // bn * bn, N)
        assert rel_l2(wrong[:, last_c], ref[:, last_c]) > 10 * TOL
    # a small error confined to the last of 24577 rows is diluted below the bound over the whole C, but not over the last row tile
    big = _rnd(24577, 512, seed=3)
    wrong = big.clone()
    wrong[-1] *= 1 + 1e-3
    assert rel_l2(wrong, big) < TOL and rel_l2(wrong[-1:], big[-1:]) > 10 * TOL


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
def test_bounds_discriminate_skipped_operand_rounding(prec):
    """A 16-bit kernel that multiplied the fp32 operands (no rounding on the way into LDS) misses the 2e-5 bound by 10x."""
    dt = DT16[prec]
    for M, N, K in ((64, 64, 8), (300, 130, 1028), (100, 512, 4096)):
        a, w = _rnd(M, K, seed=M).float(), (_rnd(N, K, seed=N) / math.sqrt(K)).float()
        ref = a.to(dt).double() @ w.to(dt).double().t()
        assert rel_l2(a.double() @ w.double().t(), ref) > 10 * TOL, (prec, M, N, K)


def test_bounds_discriminate_missing_split_k_slice():
    for sp in range(2, 9):
        K = 512 * sp + 4
        ln = ((K + sp - 1) // sp + 15) // 16 * 16
        a, w = _rnd(64, K, seed=sp), _rnd(32, K, seed=sp + 10) / math.sqrt(K)
        ref = a @ w.t()
        for s in range((K + ln - 1) // ln):
            keep = torch.ones(K, dtype=torch.bool)
            keep[s * ln:(s + 1) * ln] = False
            assert rel_l2(a[:, keep] @ w[:, keep].t(), ref) > 10 * TOL, (sp, s)
