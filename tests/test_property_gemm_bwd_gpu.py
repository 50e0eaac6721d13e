"""Property-based sweep of the BACKWARD GEMMs along the block tile, the operand layout and the split count (the backward
counterpart of tests/test_property_gemm_gpu.py).

Three launchers carry every weight and input gradient of training: csrc/gemm_bwd_f32.hip (fp32 MFMA), csrc/gemm_bwd_mfma16_impl.h
(16-bit MFMA on operands rounded while staged) and csrc/gemm_dw16_impl.h (the fused weight + bias gradient).  The first two choose
among 128x128, 128x64 and 64x64 by tile count and split the contraction up to 32 ways; the third has one tile and splits up to
64 ways.  Every call below asserts the launch it recorded (cfm_debug_gemm_last_tile, families 3, 4 and 5: tile, K slices
launched, layout / epilogue / aligned-instantiation / 16-bit-B bits) against the launch rule restated here, so a test that silently
fell back to another tile fails.

Reference: a float64 product on the CPU.  Under bf16 / fp16 it takes the operands rounded (RNE) to that type where the kernel
documents the rounding (A and B of the products) and the STORED values where the kernel does not round (the dY summed into db, Z
of swish', the dropout mask).  Checks are per window: rel-L2 of every BM x BN block of C and of the last row band and the last
column band on their own.  Every output is carved from a sentinel-filled buffer (a guard row either side, the columns J..ldc)
and the sentinels are asserted afterwards; operand padding is NaN unless the call declares it zero (pad4).

Bounds: the project's TOL where no slices meet, TOL_ATOMIC where K slices (or, for db, waves) meet through fp32 atomics, both
for contractions up to 2048; beyond that TOL * sqrt(Kc / 2048) -- random-walk growth of the fp32 accumulation error, derived and
not measured.  The CPU tests at the end check that each plausible wrong answer misses the bound of the case it corrupts.
"""
import ctypes
import math

import pytest
import torch

hypothesis = pytest.importorskip("hypothesis")
from hypothesis import example, given, settings, strategies as st, HealthCheck  # noqa: E402

pytestmark = pytest.mark.gpu
# Worst window observed on an MI355X over the whole file, next to each bound (the `ops` fixture prints them: pytest -s).  Every
# family sits 35x or more below its bound: the bounds are the project's, they were not fitted to these figures.
TOL = 2e-5                   # no split.  fp32 5.7e-7 (Kc = 1023), 16-bit 2.0e-7 (Kc = 1023), swish' epilogue 2.3e-7,
                             # weight-gradient kernel dw, one slice 1.2e-7
TOL_ATOMIC = 5e-5            # slices meet through atomics.  fp32 5.6e-7, 16-bit 2.0e-7 (both Kc = 2047, two calls onto one C),
                             # weight-gradient kernel db 2.8e-7 (M = 1000); figures through atomics move in the second digit run to run
LONG_K = 2048                # beyond: TOL * sqrt(Kc / LONG_K).  fp32 5.8e-7 of 2.8e-5 (Kc = 4095, 4 slices), 16-bit 1.6e-7 of
                             # 2.0e-5 (Kc = 2049), weight-gradient kernel dw 1.6e-7 of 2.1e-5 (M = 2240), db 4.2e-7 of 3.2e-5 (M = 5119)
DT16 = {1: torch.bfloat16, 2: torch.float16}
PREC_IDS = {0: "fp32", 1: "bf16", 2: "fp16"}
F_BWD32, F_BWD16, F_DW16 = 3, 4, 5            # cfm_debug_gemm_last_tile families
TILES = {0: (128, 128), 1: (128, 64), 3: (64, 64)}   # cfm_debug_set_bwd_tile
SENT = 7.0
NAN = float("nan")
SET = dict(deadline=None, derandomize=True, suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])
WORST = {}                   # label -> (error / bound, error, bound, what): printed when the module is done (pytest -s)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conformer_amd import _lib, ops as _ops
    assert _lib.load().cfm_device_check() == 0, "not a gfx950 device"
    yield _ops
    for k in sorted(WORST):
        r, e, b, what = WORST[k]
        print(f"\n[worst] {k}: {e:.3e} of {b:.3e} ({r:.3f}) at {what}", end="")
    print()


@pytest.fixture
def bwd_tile(ops):
    """Forces the block tile of the backward GEMMs; the heuristic is restored whatever happens."""
    def force(tile):
        from conformer_amd import _lib
        _lib.check(lib().cfm_debug_set_bwd_tile(tile), "cfm_debug_set_bwd_tile")
    try:
        yield force
    finally:
        lib().cfm_debug_set_bwd_tile(-1)


def lib():
    from conformer_amd import _lib
    return _lib.load()


def last_tile(family):
    """(BM, BN, waves, K slices, form, 16-bit C) of the family's last launch; clears the record."""
    from conformer_amd import _lib
    out = (ctypes.c_int * 6)()
    _lib.check(lib().cfm_debug_gemm_last_tile(family, ctypes.addressof(out)), "cfm_debug_gemm_last_tile")
    return tuple(out)


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def r16(t, prec):
    """t rounded to the 16-bit type of `prec` (identity for fp32), as float64."""
    return (t.to(DT16[prec]) if prec else t).double()


def up(n, q):
    return (n + q - 1) // q * q


def dswish(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def bound(Kc, atomic=False):
    if Kc <= LONG_K:
        return TOL_ATOMIC if atomic else TOL
    return TOL * math.sqrt(Kc / LONG_K)


# ---- the launch rules, restated ---------------------------------------------------------------------------------------------
def form_bits(a_col, b_col, epi_dswish=False, aligned=0, b16=False):
    return int(not a_col) | int(not b_col) << 1 | int(epi_dswish) << 2 | int(aligned) << 3 | int(b16) << 4


def aligned16(a_col, b_col, b16, I, J, Kc, pad4):
    """The 16-bit launcher's ALIGNED instantiation: every 16-byte chunk of both operands is all in or all out."""
    al_a = ((I % 4 == 0) if a_col else (Kc % 4 == 0)) or pad4
    al_b = ((J % (8 if b16 else 4) == 0) if b_col else (Kc % 4 == 0)) or (pad4 and not b16)
    return int(al_a and al_b)


def t128_of(I, J, nbatch=1):
    return -(-I // 128) * -(-J // 128) * nbatch


def auto_tile_f32(I, J, nbatch=1):
    t = t128_of(I, J, nbatch)
    if t >= 3072 and I >= 96 and J >= 96:
        return 0
    if t >= 768 and I >= 96 and J >= 48:
        return 1
    return 3


def auto_tile_16(a_col, b_col, I, J, nbatch=1):
    t = t128_of(I, J, nbatch)
    if a_col and b_col and nbatch == 1 and 96 <= I <= 512 and J >= 512:
        return 1
    if I < 96 or J < 96:
        return 3
    if t >= 400:
        return 0
    if t >= 200 and J >= 64 and not (a_col and b_col):
        return 1
    return 3


def general_splits(prec, bm, bn, I, J, Kc, nbatch=1):
    """(K slices launched, slice length) of the general kernels with allow_split: doubled while the grid is short of the target
    and a half slice still holds 512 contraction steps, up to 32; the slice is rounded up to the K-tile."""
    target, gran = (1024, 64) if prec else (768, 16)
    tiles = -(-I // bm) * -(-J // bn)
    s = 1
    while tiles * nbatch * s < target and Kc // (2 * s) >= 512 and s < 32:
        s *= 2
    return s, up(-(-Kc // s), gran)


def dw16_splits(N, K, M):
    """(K slices launched, slice length) of the weight-gradient kernel: ~2 workgroups per CU, slices of >= 256 rows, at most 64;
    slices that would start past M are not launched."""
    tiles = -(-N // 128) * -(-K // 128)
    s = 1
    while tiles * s < 448 and M // (2 * s) >= 256 and s < 64:
        s *= 2
    kps = up(-(-M // s), 64)
    return -(-M // kps), kps


# ---- operands, outputs, checks ---------------------------------------------------------------------------------------------
def lay(x, col, prec=0, as16=False, zero_pad=False, extra=0):
    """Device image of the logical (index, contraction) matrix x: index-major (rows padded to 4) or contraction-major (rows
    padded to 4, or 8 for a 16-bit tensor), + `extra` columns.  Padding is NaN unless the call promises zeros (pad4)."""
    idx, kc = x.shape
    fill = 0.0 if zero_pad else NAN
    if col:
        buf = torch.full((kc, up(idx, 8 if as16 else 4) + extra), fill)
        buf[:, :idx] = x.t()
    else:
        buf = torch.full((idx, up(kc, 4) + extra), fill)
        buf[:, :kc] = x
    return (buf.to(DT16[prec]) if as16 else buf).cuda()


def carve(I, J, dtype=torch.float32, init=None, extra=None):
    """(buffer, C): C is rows 1..I of a sentinel-filled (I + 2, ldc) buffer, ldc > J."""
    q = 4 if dtype == torch.float32 else 8
    buf = torch.full((I + 2, up(J, q) + (q if extra is None else extra)), SENT, dtype=dtype, device="cuda")
    c = buf[1:I + 1]
    if init is not None:
        c[:, :J] = init if isinstance(init, float) else init.to(dtype).cuda()
    return buf, c


def sentinels_ok(buf, J):
    return bool((buf[0] == SENT).all()) and bool((buf[-1] == SENT).all()) and bool((buf[1:-1, J:] == SENT).all())


def _rel(a, b):
    den = float(b.norm())
    return float((a - b).norm()) / (den if den > 0 else 1.0)


def check_windows(got, ref, bm, bn, tol, what, label):
    """rel-L2 of every bm x bn block and of the last row band and the last column band on their own."""
    got = got.double().cpu()
    I, J = ref.shape
    assert got.shape == ref.shape
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values in C"
    worst, where = 0.0, None
    for i0 in range(0, I, bm):
        for j0 in range(0, J, bn):
            e = _rel(got[i0:i0 + bm, j0:j0 + bn], ref[i0:i0 + bm, j0:j0 + bn])
            if e > worst:
                worst, where = e, (i0, j0)
    for name, r, c in (("last row band", slice((I - 1) // bm * bm, I), slice(0, J)),
                       ("last column band", slice(0, I), slice((J - 1) // bn * bn, J))):
        e = _rel(got[r, c], ref[r, c])
        if e > worst:
            worst, where = e, name
    if label not in WORST or worst / tol > WORST[label][0]:
        WORST[label] = (worst / tol, worst, tol, what)
    assert worst < tol, f"{what}: window {where}: {worst:.3e} >= {tol:.3e}"
    return worst


def fam_of(prec):
    return F_BWD16 if prec else F_BWD32


def lbl(prec, kind):
    return f"{'16-bit' if prec else 'fp32'} {kind}"


# ==== a. every forced tile x every layout x {fp32, bf16, fp16} ===============================================================
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]
OFFS = (0, 1, -1, 4, -4, -6, 3)                # exactly full, +1, -1, +4, -4 and two residues mod 4 (2 and 3)
KCS = (1, 4, 60, 64, 68, 127, 130)


def extent(n, b, off):
    return max(1, n * b + off)


def run_layouts(ops, force, prec, tile, I, J, Kc, alpha, acc, pad4, seed):
    bm, bn = TILES[tile]
    pad4 = bool(pad4 and prec)
    A, B = rnd(I, Kc, seed=seed) / math.sqrt(Kc), rnd(J, Kc, seed=seed + 1)
    C0 = rnd(I, J, seed=seed + 2) if acc else None
    ref = alpha * (r16(A, prec) @ r16(B, prec).t()) + (C0.double() if acc else 0.0)
    forms = [(a, b, False) for a, b in LAYOUTS] + ([(False, True, True), (True, True, True)] if prec else [])
    force(tile)
    for a_col, b_col, b16 in forms:
        Ad = lay(A, a_col, zero_pad=pad4)
        Bd = lay(B, b_col, prec, as16=b16, zero_pad=pad4)
        buf, c = carve(I, J, init=C0)
        ops.gemm_bwd(Ad, a_col, Bd, b_col, I, J, Kc, alpha=alpha, out=c, accumulate=acc, prec=prec, b16=b16, pad4=pad4)
        rec = last_tile(fam_of(prec))
        al = aligned16(a_col, b_col, b16, I, J, Kc, pad4) if prec else 0
        what = f"{PREC_IDS[prec]} tile {bm}x{bn} a_col={a_col} b_col={b_col} b16={b16} {I}x{J}x{Kc} alpha={alpha} acc={acc} pad4={pad4}"
        assert rec == (bm, bn, 4, 1, form_bits(a_col, b_col, False, al, b16), 0), (what, rec)
        check_windows(c[:, :J], ref, bm, bn, bound(Kc), what, lbl(prec, "direct"))
        assert sentinels_ok(buf, J), f"{what}: wrote outside C"


@pytest.mark.parametrize("prec", [0, 1, 2], ids=PREC_IDS.values())
@pytest.mark.parametrize("tile", [0, 1, 3], ids=["128x128", "128x64", "64x64"])
@settings(max_examples=4, **SET)
@given(ni=st.integers(1, 3), nj=st.integers(1, 3), oi=st.sampled_from(OFFS), oj=st.sampled_from(OFFS), Kc=st.sampled_from(KCS),
       alpha=st.sampled_from([1.0, 0.5, -1.75]), acc=st.booleans(), pad4=st.booleans(), seed=st.integers(0, 10 ** 6))
@example(ni=1, nj=1, oi=0, oj=0, Kc=64, alpha=1.0, acc=False, pad4=False, seed=1).via("one full tile, one full K-tile")
@example(ni=2, nj=3, oi=1, oj=-1, Kc=130, alpha=-1.75, acc=True, pad4=True, seed=2).via("ragged everywhere, zero-padded operands: the aligned instantiation")
@example(ni=3, nj=2, oi=-6, oj=3, Kc=127, alpha=0.5, acc=False, pad4=False, seed=3).via("ragged everywhere: the unaligned instantiation")
@example(ni=2, nj=2, oi=4, oj=-4, Kc=1, alpha=1.0, acc=True, pad4=False, seed=4).via("a contraction of one")
def test_forced_tiles_every_layout(ops, bwd_tile, prec, tile, ni, nj, oi, oj, Kc, alpha, acc, pad4, seed):
    """Each forced tile with the four a_col / b_col layouts (16-bit: also a 16-bit contraction-major B), ragged I / J / Kc,
    alpha, accumulate onto a non-zero C: float64 of the (rounded) operands per window, the recorded tile, aligned bit, one
    slice."""
    bm, bn = TILES[tile]
    run_layouts(ops, bwd_tile, prec, tile, extent(ni, bm, oi), extent(nj, bn, oj), Kc, alpha, acc, pad4, seed)


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
def test_both_aligned_instantiations_run(ops, bwd_tile, prec):
    """The record's aligned bit, literally: ragged extents take the element-wise instantiation, the same extents with pad4 (and
    aligned extents without it) the select-only one."""
    I, J, Kc = 130, 67, 70
    A, B = rnd(I, Kc, seed=5) / math.sqrt(Kc), rnd(J, Kc, seed=6)
    ref = r16(A, prec) @ r16(B, prec).t()
    for tile, (bm, bn) in TILES.items():
        bwd_tile(tile)
        for a_col, b_col in LAYOUTS:
            for pad4, want in ((False, 0), (True, 1)):
                buf, c = carve(I, J)
                ops.gemm_bwd(lay(A, a_col, zero_pad=pad4), a_col, lay(B, b_col, zero_pad=pad4), b_col, I, J, Kc, out=c, prec=prec, pad4=pad4)
                rec = last_tile(F_BWD16)
                assert rec[:4] == (bm, bn, 4, 1) and (rec[4] >> 3) & 1 == want, (tile, a_col, b_col, pad4, rec)
                check_windows(c[:, :J], ref, bm, bn, TOL, f"aligned={want} tile {tile} {a_col} {b_col}", lbl(prec, "direct"))
                assert sentinels_ok(buf, J)
        buf, c = carve(128, 64)                                                # aligned extents, no pad4
        ops.gemm_bwd(lay(A[:128, :68], True), True, lay(B[:64, :68], True), True, 128, 64, 68, out=c, prec=prec)
        assert (last_tile(F_BWD16)[4] >> 3) & 1 == 1


# ==== b. the swish' epilogue on every forced tile ============================================================================
def z_image(Z, ld, dtype=torch.float32):
    buf = torch.full((Z.shape[0], ld), NAN)
    buf[:, :Z.shape[1]] = Z
    return buf.to(dtype).cuda()


def run_dswish(ops, force, prec, tile, I, J, Kc, alpha, drop_p, zslice, b16, acc, seed):
    bm, bn = TILES[tile]
    fam = fam_of(prec)
    b16 = bool(b16 and prec)
    dY, W, Z = rnd(I, Kc, seed=seed) / math.sqrt(Kc), rnd(J, Kc, seed=seed + 1), rnd(I, J, seed=seed + 2) * 1.5
    C0 = rnd(I, J, seed=seed + 3) if acc else None
    dseed = seed * 7 + 1
    # the mask is a function of the flat index row * J + col: drawn over I * J rounded up to the 4 elements dropout_apply needs
    mask = (ops.dropout_apply(torch.ones(up(I * J, 4), device="cuda"), drop_p, dseed)[:I * J].view(I, J).double().cpu()
            if drop_p > 0 else 1.0)
    prod = alpha * (r16(dY, prec) @ r16(W, prec).t()) * mask
    Ad, Bd = lay(dY, False), lay(W, True, prec, as16=b16)
    zforms = [(torch.float32, up(J, 8) + 4 if zslice else up(J, 4))]
    if prec and J % 8 == 0:
        zforms.append((DT16[prec], J + 8 if zslice else J))                 # z16: J % 8 == 0, ldz % 8 == 0
    force(tile)
    for zdt, ldz in zforms:
        zd = z_image(Z, ldz, zdt)
        ref = prod * dswish(zd[:, :J].double().cpu()) + (C0.double() if acc else 0.0)     # the STORED Z
        buf, c = carve(I, J, init=C0)
        kw = dict(alpha=alpha, Z=zd[:, :J], drop_p=drop_p, drop_seed=dseed, prec=prec, b16=b16)
        ops.gemm_bwd(Ad, False, Bd, True, I, J, Kc, out=c, accumulate=acc, **kw)
        rec = last_tile(fam)
        al = aligned16(False, True, b16, I, J, Kc, False) if prec else 0
        what = f"{PREC_IDS[prec]} swish' tile {bm}x{bn} {I}x{J}x{Kc} z={zdt} ldz={ldz} p={drop_p} b16={b16} acc={acc}"
        assert rec == (bm, bn, 4, 1, form_bits(False, True, True, al, b16), 0), (what, rec)
        check_windows(c[:, :J], ref, bm, bn, bound(Kc), what, "swish' epilogue")
        assert sentinels_ok(buf, J), f"{what}: wrote outside C"
        if prec and J % 8 == 0 and not acc:
            # c16: "identical results" -- the fp32 value of the same call, rounded once
            buf16, c16 = carve(I, J, dtype=DT16[prec])
            ops.gemm_bwd(Ad, False, Bd, True, I, J, Kc, out=c16, c16=True, **kw)
            rec16 = last_tile(fam)
            assert rec16[:5] == rec[:5] and rec16[5] == 1, (what, rec, rec16)
            assert torch.equal(c16[:, :J], c[:, :J].to(DT16[prec])), f"{what}: the 16-bit C is not the fp32 C rounded"
            assert sentinels_ok(buf16, J), f"{what}: c16 wrote outside C"


@pytest.mark.parametrize("prec", [0, 1, 2], ids=PREC_IDS.values())
@pytest.mark.parametrize("tile", [0, 1, 3], ids=["128x128", "128x64", "64x64"])
@settings(max_examples=4, **SET)
@given(ni=st.integers(1, 3), nj=st.integers(1, 3), oi=st.sampled_from(OFFS), oj=st.sampled_from((0, 8, -8, 0, 4, -4, 1, -6)),
       Kc=st.sampled_from(KCS), alpha=st.sampled_from([1.0, 0.5, -1.75]), drop_p=st.sampled_from([0.0, 0.2]), zslice=st.booleans(),
       b16=st.booleans(), acc=st.booleans(), seed=st.integers(0, 10 ** 6))
@example(ni=2, nj=2, oi=1, oj=-8, Kc=130, alpha=0.5, drop_p=0.2, zslice=True, b16=True, acc=False, seed=11).via("J % 8 == 0: z16 and c16, sliced Z, dropout, 16-bit W")
@example(ni=3, nj=1, oi=-1, oj=0, Kc=64, alpha=-1.75, drop_p=0.0, zslice=False, b16=False, acc=False, seed=12).via("J % 8 == 0: z16 and c16, contiguous Z, fp32 W")
@example(ni=1, nj=3, oi=3, oj=-6, Kc=127, alpha=1.0, drop_p=0.2, zslice=True, b16=False, acc=True, seed=13).via("J % 4 == 2: the element-wise epilogue, accumulate")
@example(ni=2, nj=2, oi=0, oj=4, Kc=68, alpha=1.0, drop_p=0.2, zslice=False, b16=True, acc=True, seed=14).via("J % 8 == 4: the row-major epilogue on an fp32 Z only")
def test_dswish_epilogue_every_tile(ops, bwd_tile, prec, tile, ni, nj, oi, oj, Kc, alpha, drop_p, zslice, b16, acc, seed):
    """dX = alpha * (dY.W) * swish'(Z) * mask on each forced tile: Z contiguous or a column slice with ldz % 8 == 4 (16-bit Z:
    ldz % 8 == 0), fp32 and 16-bit Z and W; wherever the entry accepts a 16-bit C it equals the fp32 C of the same call rounded
    once, on the same tile."""
    bm, bn = TILES[tile]
    run_dswish(ops, bwd_tile, prec, tile, extent(ni, bm, oi), extent(nj, bn, oj), Kc, alpha, drop_p, zslice, b16, acc, seed)


def c16_inputs(prec, seed=21):
    """The inputs of the pinned c16 comparison: test_bounds_discriminate_c16_double_rounding shows, on the CPU, that rounding
    the exact result once gives other bits than rounding its fp32 value at some of these elements."""
    I, J, Kc = 200, 192, 68
    return I, J, Kc, rnd(I, Kc, seed=seed) / math.sqrt(Kc), rnd(J, Kc, seed=seed + 1), rnd(I, J, seed=seed + 2) * 1.5


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("tile", [0, 1, 3], ids=["128x128", "128x64", "64x64"])
def test_c16_is_the_fp32_result_rounded_once(ops, bwd_tile, prec, tile):
    I, J, Kc, dY, W, Z = c16_inputs(prec)
    bwd_tile(tile)
    dt = DT16[prec]
    Ad, Bd, zd = lay(dY, False), lay(W, True), z_image(Z, J)
    buf, c = carve(I, J)
    buf16, c16 = carve(I, J, dtype=dt)
    ops.gemm_bwd(Ad, False, Bd, True, I, J, Kc, alpha=0.5, Z=zd, out=c, prec=prec)
    rec = last_tile(F_BWD16)
    ops.gemm_bwd(Ad, False, Bd, True, I, J, Kc, alpha=0.5, Z=zd, out=c16, prec=prec, c16=True)
    rec16 = last_tile(F_BWD16)
    assert rec[:2] == TILES[tile] and rec16[:5] == rec[:5] and (rec[5], rec16[5]) == (0, 1)
    assert torch.equal(c16[:, :J], c[:, :J].to(dt))
    assert sentinels_ok(buf, J) and sentinels_ok(buf16, J)
    ref = 0.5 * (r16(dY, prec) @ r16(W, prec).t()) * dswish(Z.double())
    check_windows(c[:, :J], ref, *TILES[tile], TOL, f"c16 inputs {PREC_IDS[prec]} tile {tile}", "swish' epilogue")


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
def test_16bit_entry_refusals(ops, prec):
    """cfm_gemm_bwd_batched_mfma16_f32 refuses a 16-bit C with accumulate (or without Z), a 16-bit Z at J % 8 != 0 and a 16-bit
    B that is not contraction-major."""
    Err = ops._lib.ConformerHipError
    last_tile(F_BWD16)
    dt = DT16[prec]
    I, J, Kc = 64, 72, 64
    A, B, Z = lay(rnd(I, Kc), False), lay(rnd(J, Kc), True), z_image(rnd(I, J), J)
    c16 = torch.zeros(I, J, device="cuda", dtype=dt)
    with pytest.raises(Err):
        ops.gemm_bwd(A, False, B, True, I, J, Kc, Z=Z, out=c16, prec=prec, c16=True, accumulate=True)
    with pytest.raises(Err):
        ops.gemm_bwd(A, False, B, True, I, J, Kc, out=c16, prec=prec, c16=True)
    J4 = 68                                                              # J % 8 == 4
    B4, Z16 = lay(rnd(J4, Kc), True), z_image(rnd(I, J4), 72, dt)
    with pytest.raises(Err):
        ops.gemm_bwd(A, False, B4, True, I, J4, Kc, Z=Z16[:, :J4], out=torch.zeros(I, J4, device="cuda"), prec=prec)
    Brow16 = lay(rnd(J, Kc), False).to(dt)
    with pytest.raises(Err):
        ops.gemm_bwd(A, False, Brow16, False, I, J, Kc, out=torch.zeros(I, J, device="cuda"), prec=prec, b16=True)
    assert last_tile(F_BWD16) == (0,) * 6, "a refused call launched a kernel"


# ==== c. every split count, decided by shape ================================================================================
def short_tail_kc(prec, S):
    """The smallest Kc that takes S slices with a last non-empty slice of 1..4 contraction steps, or None."""
    gran = 64 if prec else 16
    for Kc in range(512 * S, 1024 * S if S < 32 else 40 * 1024):
        kps = up(-(-Kc // S), gran)
        tail = Kc - (-(-Kc // kps) - 1) * kps
        if 1 <= tail <= 4:
            return Kc
    return None


@pytest.mark.parametrize("prec", [0, 1, 2], ids=PREC_IDS.values())
@pytest.mark.parametrize("S", [1, 2, 4, 8, 16, 32])
def test_general_split_counts(ops, prec, S):
    """allow_split on a 64 x 64 output (one tile: the grid is always short of the target, the contraction decides): Kc = 512 S is
    the first to take S slices and 512 S - 1 the last to take S / 2; + 1 makes the last slice short (16-bit, S >= 16: the last
    slices empty but launched).  Every layout; the recorded slice count; C must be zero beforehand -- a second call doubles it."""
    I = J = 64
    Kcs = [512 * S, 512 * S + 1] + ([512 * S - 1] if S > 1 else [511, 1023]) + ([short_tail_kc(prec, S)] if S > 1 else [])
    seen = set()
    for Kc in [k for k in Kcs if k]:
        want, kps = general_splits(prec, 64, 64, I, J, Kc)
        seen.add(want)
        empty = sum(1 for y in range(want) if y * kps >= Kc)
        if prec and S == 32 and Kc == 512 * S + 1:
            assert empty > 0, "this case is meant to launch empty slices"
        A, B = rnd(I, Kc, seed=Kc) / math.sqrt(Kc), rnd(J, Kc, seed=Kc + 1)
        ref = 0.5 * (r16(A, prec) @ r16(B, prec).t())
        forms = [(a, b, False) for a, b in LAYOUTS] + ([(True, True, True)] if prec else [])
        for a_col, b_col, b16 in forms:
            Ad, Bd = lay(A, a_col), lay(B, b_col, prec, as16=b16)
            buf, c = carve(I, J, init=0.0)
            kw = dict(alpha=0.5, out=c, allow_split=True, prec=prec, b16=b16)
            ops.gemm_bwd(Ad, a_col, Bd, b_col, I, J, Kc, **kw)
            rec = last_tile(fam_of(prec))
            al = aligned16(a_col, b_col, b16, I, J, Kc, False) if prec else 0
            what = f"{PREC_IDS[prec]} split {want} (slice {kps}, {empty} empty) Kc={Kc} a_col={a_col} b_col={b_col} b16={b16}"
            assert rec == (64, 64, 4, want, form_bits(a_col, b_col, False, al, b16), 0), (what, rec)
            kind = ("atomic" if want > 1 else "direct") + (" long" if Kc > LONG_K else "")
            check_windows(c[:, :J], ref, 64, 64, bound(Kc, want > 1), what, lbl(prec, kind))
            if want > 1:
                ops.gemm_bwd(Ad, a_col, Bd, b_col, I, J, Kc, **kw)                 # not re-zeroed: the slices add onto C
                last_tile(fam_of(prec))
                check_windows(c[:, :J], 2 * ref, 64, 64, bound(Kc, True), what + " twice", lbl(prec, kind))
            assert sentinels_ok(buf, J), f"{what}: wrote outside C"
    assert S in seen and (S == 1 or S // 2 in seen), (S, seen)


def dw16_call(ops, prec, dy, dy16, x, x16, alpha, with_db, extra=8):
    """cfm_linear_bwd_weight_mfma16_f32 on row-major dy (M, N) and x (M, K) with leading dimensions wider than the extents;
    returns (dw, db or None, the K slices recorded) after asserting the record's form and the sentinels."""
    from conformer_amd import _lib
    dt = DT16[prec]
    (M, N), K = dy.shape, x.shape[1]
    dyb, xb = torch.full((M, N + extra), NAN), torch.full((M, K + extra), NAN)
    dyb[:, :N], xb[:, :K] = dy, x
    dyd, xd = (dyb.to(dt) if dy16 else dyb).cuda(), (xb.to(dt) if x16 else xb).cuda()
    buf, dw = carve(N, K, init=0.0, extra=12)
    dbuf = torch.full((N + 16,), SENT, device="cuda")
    dbuf[8:8 + N] = 0.0
    st_ = lib().cfm_linear_bwd_weight_mfma16_f32(prec, dyd.data_ptr(), int(dy16), dyd.stride(0), xd.data_ptr(), int(x16), xd.stride(0),
                                                 dw.data_ptr(), dw.stride(0), dbuf[8:].data_ptr() if with_db else None, N, K, M, alpha,
                                                 ops._stream())
    _lib.check(st_, "cfm_linear_bwd_weight_mfma16_f32")
    rec = last_tile(F_DW16)
    assert rec[:3] == (128, 128, 4) and rec[4] == int(dy16) | int(x16) << 1 and rec[5] == 0, rec
    assert sentinels_ok(buf, K), "dw: wrote outside the matrix"
    assert bool((dbuf[:8] == SENT).all()) and bool((dbuf[8 + N:] == SENT).all()), "db: wrote outside the vector"
    if not with_db:
        assert bool((dbuf[8:8 + N] == 0).all()), "db was NULL and something was written"
    return dw[:, :K], (dbuf[8:8 + N] if with_db else None), rec[3]


# dY whose stored fp32 value differs from its 16-bit rounding by a known, one-sided amount: g has 8 significant bits (exact in
# bf16 and fp16), dY = g + |g| * DELTA is exact in fp32 (8 + 16 <= 24 bits) and less than half a 16-bit ulp from g, so it rounds
# back to g.  The column sums of the stored and of the rounded values then differ by DELTA * sum |g| -- far more than the bound
# (test_bounds_discriminate_db_stored_vs_rounded) -- which pins WHICH of the two db sums.
DELTA = {1: 2.0 ** -9 - 2.0 ** -13, 2: 2.0 ** -12 - 2.0 ** -16}


def dy_off_grid(M, N, prec, seed):
    g = rnd(M, N, seed=seed).to(torch.bfloat16).float()
    g = torch.where(g.abs() < 2.0 ** -6, torch.copysign(torch.tensor(2.0 ** -6), g), g)     # (inside fp16's normal range)
    dy = (g.double() + g.double().abs() * DELTA[prec]).float()
    assert torch.equal(dy.double(), g.double() + g.double().abs() * DELTA[prec]) and torch.equal(dy.to(DT16[prec]).float(), g)
    return dy


def check_dw16(ops, prec, M, N, K, dy16, x16, alpha, with_db, seed, want_slices=None):
    dy, x = dy_off_grid(M, N, prec, seed), rnd(M, K, seed=seed + 1)
    dw, db, slices = dw16_call(ops, prec, dy, dy16, x, x16, alpha, with_db)
    if want_slices is not None:
        assert slices == want_slices, (M, N, K, slices, want_slices)
    what = f"dw16 {PREC_IDS[prec]} dy16={dy16} x16={x16} M={M} N={N} K={K} slices={slices}"
    check_windows(dw, alpha * (r16(dy, prec).t() @ r16(x, prec)), 128, 128, bound(M, slices > 1), what,
                  "dw16 dw" + (" long" if M > LONG_K else ""))
    if with_db:
        stored = r16(dy, prec) if dy16 else dy.double()                       # the kernel sums what is stored
        check_windows(db[None, :], alpha * stored.sum(0)[None, :], 1, 128, bound(M, True), what + " db",
                      "dw16 db" + (" long" if M > LONG_K else ""))
    return slices


def dw16_reachable():
    """K slices the weight-gradient launcher can produce for M in 255 .. 20480 (one output tile) -> {count: [M, ...]} with up to
    three M each: the last slice full, one row long, one row short."""
    out = {}
    for M in range(255, 20481):
        y, kps = dw16_splits(8, 8, M)
        tail = M - (y - 1) * kps
        kind = 0 if tail == kps else 1 if tail == 1 else 2 if tail == kps - 1 else 3
        out.setdefault(y, {}).setdefault(kind, M)
    return {y: sorted(m for k, m in v.items() if k < 3 or len(v) == 1) for y, v in out.items()}


DW16_MS = dw16_reachable()


def test_dw16_split_rule_reaches_these_counts():
    """What "every split count" means for the weight-gradient kernel: the rule rounds a slice up to 64 rows and launches only
    the slices that start inside M, so between the powers of two it reaches the counts just below them only."""
    got = set(DW16_MS)
    assert {1, 2, 4, 8, 16, 32, 64} <= got and max(got) == 64
    assert got == {1, 2, 4, 7, 8} | set(range(13, 17)) | set(range(26, 33)) | set(range(52, 65)), sorted(got)


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("band", [(1, 8), (13, 16), (26, 32), (52, 58), (59, 64)], ids=lambda b: f"{b[0]}-{b[1]}")
def test_dw16_every_split_count(ops, prec, band):
    """Every K-slice count the launcher can produce, decided by M (255 .. 20480) and asserted through the record, with the last
    slice full, one row long and one row short; N and K in 8 .. 136 (one, two and four output tiles), the four operand forms in
    turn.  dw and db accumulate: both are zeroed beforehand."""
    shapes = [(136, 136), (8, 136), (136, 8), (72, 128), (128, 8), (8, 8)]
    n = 0
    for y in [y for y in range(band[0], band[1] + 1) if y in DW16_MS]:
        for M in DW16_MS[y]:
            N, K = shapes[n % len(shapes)] if M <= 4096 else shapes[1 + n % (len(shapes) - 1)]
            assert dw16_splits(N, K, M)[0] == y
            check_dw16(ops, prec, M, N, K, bool(n & 1), bool(n & 2), -0.75, True, seed=M, want_slices=y)
            n += 1


# ==== d. the heuristic's own thresholds =====================================================================================
def run_batched(ops, prec, I, J, Kc, nb0, nb1, a_col, b_col, want_tile):
    """nb0 x nb1 problems: A varies with b0 only (sa1 = 0), B with b1 only (sb0 = 0), C (b0, b1) has its own guard rows; every
    block of the first and of the last entry against float64, no sentinel left inside any entry, none disturbed outside."""
    bm, bn = TILES[want_tile]
    A, B = rnd(nb0, I, Kc, seed=I + nb0) / math.sqrt(Kc), rnd(nb1, J, Kc, seed=J + nb1)
    Ad = torch.stack([lay(A[i], a_col) for i in range(nb0)])
    Bd = torch.stack([lay(B[i], b_col) for i in range(nb1)])
    ldc = up(J, 4) + 4
    buf = torch.full((nb0 * nb1, I + 2, ldc), SENT, device="cuda")
    ops.gemm_bwd(Ad, a_col, Bd, b_col, I, J, Kc, alpha=0.5, out=buf, c_ptr=buf[0, 1].data_ptr(), prec=prec, nbatch=nb0 * nb1, nb1=nb1,
                 sa=(Ad.stride(0), 0), sb=(0, Bd.stride(0)), sc=(nb1 * buf.stride(0), buf.stride(0)))
    rec = last_tile(fam_of(prec))
    al = aligned16(a_col, b_col, False, I, J, Kc, False) if prec else 0
    what = f"{PREC_IDS[prec]} {nb0}x{nb1} problems of {I}x{J}x{Kc} a_col={a_col} b_col={b_col}"
    assert rec == (bm, bn, 4, 1, form_bits(a_col, b_col, False, al), 0), (what, rec, want_tile)
    for b0, b1 in ((0, 0), (nb0 - 1, nb1 - 1)):
        ref = 0.5 * (r16(A[b0], prec) @ r16(B[b1], prec).t())
        check_windows(buf[b0 * nb1 + b1, 1:I + 1, :J], ref, bm, bn, bound(Kc), f"{what} entry ({b0}, {b1})", lbl(prec, "direct"))
    assert bool((buf[:, 0] == SENT).all()) and bool((buf[:, -1] == SENT).all()) and bool((buf[:, 1:-1, J:] == SENT).all()), what
    assert not bool((buf[:, 1:-1, :J] == SENT).any()), f"{what}: an entry was not written"


# (I, J, nb0, nb1, a_col, b_col): t128 on both sides of 768 and of 3072, and the extent conditions of each rule
THRESH_F32 = [
    (128, 128, 13, 59, False, True), (128, 128, 12, 64, False, True),        # t128 = 767 | 768
    (96, 48, 12, 64, True, True), (96, 47, 12, 64, True, False), (95, 48, 12, 64, False, False),   # 768: I >= 96 and J >= 48
    (128, 128, 37, 83, True, True), (96, 96, 48, 64, False, True),           # t128 = 3071 | 3072
    (95, 96, 48, 64, False, False), (96, 95, 48, 64, True, False),           # 3072 with an extent below 96: the next rule
    (256, 256, 12, 16, False, True), (256, 256, 191, 1, True, True),         # 256 x 256 problems: t128 = 768 | 764
]


@pytest.mark.parametrize("case", THRESH_F32, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_f32_auto_thresholds(ops, case):
    I, J, nb0, nb1, a_col, b_col = case
    run_batched(ops, 0, I, J, 4 if nb0 * nb1 > 1000 else 20, nb0, nb1, a_col, b_col, auto_tile_f32(I, J, nb0 * nb1))


def test_f32_threshold_cases_cover_every_branch():
    got = {(auto_tile_f32(c[0], c[1], c[2] * c[3]), t128_of(c[0], c[1], c[2] * c[3])) for c in THRESH_F32}
    assert {(3, 767), (1, 768), (1, 3071), (0, 3072), (3, 3072), (1, 3072)} <= got, sorted(got)


THRESH_16 = [
    (128, 128, 199, 1, False, True), (128, 128, 10, 20, False, True),        # t128 = 199 | 200 -> 64x64 | 128x64
    (128, 128, 10, 20, True, True),                                          # 200, both contraction-major: stays 64x64
    (128, 63, 10, 20, False, False),                                         # 200 with J < 64 (< 96): 64x64
    (100, 100, 19, 21, True, False), (100, 100, 20, 20, True, True),         # t128 = 399 | 400 -> 128x64 | 128x128
    (95, 128, 20, 20, False, True), (128, 95, 20, 20, False, True),          # 400 with an extent below 96: 64x64
    (2432, 2688, 1, 1, False, True), (2560, 2560, 1, 1, False, True),        # one problem: 19 x 21 = 399 | 20 x 20 = 400
]


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", THRESH_16, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_16bit_auto_thresholds(ops, prec, case):
    I, J, nb0, nb1, a_col, b_col = case
    run_batched(ops, prec, I, J, 4, nb0, nb1, a_col, b_col, auto_tile_16(a_col, b_col, I, J, nb0 * nb1))


def test_16bit_threshold_cases_cover_every_branch():
    got = [(auto_tile_16(c[4], c[5], c[0], c[1], c[2] * c[3]), t128_of(c[0], c[1], c[2] * c[3])) for c in THRESH_16]
    assert got == [(3, 199), (1, 200), (3, 200), (3, 200), (1, 399), (0, 400), (3, 400), (3, 400), (1, 399), (0, 400)], got


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("I", [95, 96, 512, 516])
@pytest.mark.parametrize("J", [508, 512])
def test_16bit_weight_gradient_tile_rule(ops, prec, I, J):
    """Both operands contraction-major with a narrow dY (96 <= I <= 512) and J >= 512 take 128x64; one step outside, and any
    other layout at the same shape, 64x64 (t128 <= 20)."""
    Kc = 68
    A, B = rnd(I, Kc, seed=I) / math.sqrt(Kc), rnd(J, Kc, seed=J)
    ref = r16(A, prec) @ r16(B, prec).t()
    for a_col, b_col in ((True, True), (False, True)):
        want = auto_tile_16(a_col, b_col, I, J)
        assert want == (1 if a_col and 96 <= I <= 512 and J == 512 else 3)
        buf, c = carve(I, J)
        ops.gemm_bwd(lay(A, a_col), a_col, lay(B, b_col), b_col, I, J, Kc, out=c, prec=prec)
        rec = last_tile(F_BWD16)
        assert rec[:4] == (*TILES[want], 4, 1), (I, J, a_col, rec)
        check_windows(c[:, :J], ref, *TILES[want], TOL, f"dW rule {I}x{J} a_col={a_col}", lbl(prec, "direct"))
        assert sentinels_ok(buf, J)


# ==== e. sub-block addressing on the two large tiles ========================================================================
@pytest.mark.parametrize("prec", [0, 1, 2], ids=PREC_IDS.values())
@pytest.mark.parametrize("tile", [0, 1], ids=["128x128", "128x64"])
def test_sub_block_pointers(ops, bwd_tile, prec, tile):
    """a_ptr / b_ptr / c_ptr into wider tensors (head slices): the middle third of each, the rest NaN (operands) or sentinel
    (C); every layout, ragged extents."""
    bm, bn = TILES[tile]
    I, J, Kc = bm + 37, 2 * bn + 3, 70
    A, B = rnd(I, Kc, seed=31) / math.sqrt(Kc), rnd(J, Kc, seed=32)
    ref = -1.75 * (r16(A, prec) @ r16(B, prec).t())
    bwd_tile(tile)
    for a_col, b_col in LAYOUTS:
        wides = []
        for x, col in ((A, a_col), (B, b_col)):
            one = lay(x, col)
            w = one.shape[1]
            wide = torch.full((one.shape[0], 3 * w), NAN, device="cuda")
            wide[:, w:2 * w] = one
            wides.append((wide, wide.data_ptr() + 4 * w))
        (Aw, ap), (Bw, bp) = wides
        ldj = up(J, 4) + 4
        cw = torch.full((I + 2, 3 * ldj), SENT, device="cuda")
        ops.gemm_bwd(Aw, a_col, Bw, b_col, I, J, Kc, alpha=-1.75, out=cw, a_ptr=ap, b_ptr=bp, c_ptr=cw[1, ldj:].data_ptr(), prec=prec)
        rec = last_tile(fam_of(prec))
        assert rec[:4] == (bm, bn, 4, 1) and rec[4] & 3 == form_bits(a_col, b_col) & 3, rec
        check_windows(cw[1:I + 1, ldj:ldj + J], ref, bm, bn, TOL, f"sub-block {PREC_IDS[prec]} tile {tile} {a_col} {b_col}", lbl(prec, "direct"))
        keep = torch.ones_like(cw, dtype=torch.bool)
        keep[1:I + 1, ldj:ldj + J] = False
        assert bool((cw[keep] == SENT).all()), "wrote outside the sub-block"


@pytest.mark.parametrize("prec", [0, 1, 2], ids=PREC_IDS.values())
@pytest.mark.parametrize("tile", [0, 1], ids=["128x128", "128x64"])
@pytest.mark.parametrize("Kc", [44, 42])
def test_overlapping_rows(ops, bwd_tile, prec, tile, Kc):
    """lda < Kc for an index-major operand: row i starts lda = 8 elements after row i - 1 (frames of a signal)."""
    bm, bn = TILES[tile]
    I, J, lda = bm + 9, bn + 5, 8
    flat = rnd((I - 1) * lda + Kc, seed=41)
    A = flat.as_strided((I, Kc), (lda, 1))
    B = rnd(J, Kc, seed=42)
    fd = torch.full((up(flat.numel(), 4) + 4,), NAN)
    fd[:flat.numel()] = flat
    fd = fd.cuda()
    bwd_tile(tile)
    for b_col in (False, True):
        buf, c = carve(I, J)
        ops.gemm_bwd(fd, False, lay(B, b_col), b_col, I, J, Kc, out=c, lda=lda, prec=prec)
        rec = last_tile(fam_of(prec))
        assert rec[:4] == (bm, bn, 4, 1), rec
        check_windows(c[:, :J], r16(A, prec) @ r16(B, prec).t(), bm, bn, TOL, f"overlapping rows {PREC_IDS[prec]} Kc={Kc}", lbl(prec, "direct"))
        assert sentinels_ok(buf, J)


# ==== f. cfm_linear_bwd_weight_mfma16_f32 directly ==========================================================================
DW_NK = (8, 120, 128, 136, 264)
DW_M = (1, 63, 64, 65, 129, 1000)


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("dy16,x16", [(False, False), (True, False), (False, True), (True, True)], ids=["f32.f32", "dy16", "x16", "dy16.x16"])
def test_dw16_forms_and_shapes(ops, prec, dy16, x16):
    """Every (N, K) of {8, 120, 128, 136, 264}^2 at two M of {1, 63, 64, 65, 129, 1000} (all six over the pairs), leading
    dimensions wider than the extents, db present and NULL, alpha != 1.  dw: the rounded operands; db: the stored dY."""
    p = 0
    for N in DW_NK:
        for K in DW_NK:
            for M in (DW_M[p % 6], DW_M[(p + 3) % 6]):
                check_dw16(ops, prec, M, N, K, dy16, x16, -1.75 if p & 1 else 0.5, with_db=bool((p + M) & 1) or M == 1000, seed=100 * p + M,
                           want_slices=dw16_splits(N, K, M)[0])
            p += 1


# ==== g. the bounds are tight enough (CPU, float64) =========================================================================
def _rnd64(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_bounds_discriminate_dropped_k_chunk_and_split_slice():
    """A dropped last chunk of 4 contraction steps at the longest contractions used (the general kernels' 16705, the
    weight-gradient kernel's 20479) and at the forced-tile sweep's 130; the first, a middle and the last K slice of every split
    count dropped: each against the bound of the case it corrupts."""
    assert short_tail_kc(1, 32) == 16705 and max(m for ms in DW16_MS.values() for m in ms) == 20479
    for Kc in (16705, 20479, 16385, 130):
        a, b = _rnd64(64, Kc, seed=1) / math.sqrt(Kc), _rnd64(64, Kc, seed=2)
        ref = a @ b.t()
        assert _rel(a[:, :Kc - 4] @ b[:, :Kc - 4].t(), ref) > 10 * max(bound(Kc, True), bound(Kc)), Kc
    for prec in (0, 1):
        for S in (2, 4, 8, 16, 32):
            for Kc in (512 * S, 512 * S + 1, short_tail_kc(prec, S)):
                if not Kc:
                    continue
                s, kps = general_splits(prec, 64, 64, 64, 64, Kc)
                a, b = _rnd64(64, Kc, seed=S) / math.sqrt(Kc), _rnd64(64, Kc, seed=S + 1)
                ref = a @ b.t()
                live = [y for y in range(s) if y * kps < Kc]
                for y in {live[0], live[len(live) // 2], live[-1]}:             # the first, a middle and the last (shortest) slice
                    keep = torch.ones(Kc, dtype=torch.bool)
                    keep[y * kps:(y + 1) * kps] = False
                    assert _rel(a[:, keep] @ b[:, keep].t(), ref) > 10 * bound(Kc, True), (prec, S, Kc, y)
    for y, M in [(y, M) for y, Ms in DW16_MS.items() for M in Ms]:             # the weight-gradient kernel's slices (rows of dY, x)
        kps = dw16_splits(8, 8, M)[1]
        dy, x = _rnd64(M, 8, seed=y), _rnd64(M, 8, seed=y + 1)
        ref = dy.t() @ x
        keep = torch.ones(M, dtype=torch.bool)
        keep[(y - 1) * kps:] = False                                           # its last slice: the shortest
        if y > 1:
            assert _rel(dy[keep].t() @ x[keep], ref) > 10 * bound(M, True), (y, M)


def test_bounds_discriminate_duplicated_edge_row():
    """The last row (column) of C computed from the row before it -- a clamped index that is stored instead of dropped -- is
    far outside the bound of the last row (column) band, for each tile height."""
    for I, J in ((129, 131), (257, 67), (65, 385)):
        ref = _rnd64(I, 70, seed=I) @ _rnd64(J, 70, seed=J).t()
        for bm, bn in TILES.values():
            wrong = ref.clone()
            wrong[-1] = ref[-2]
            band = slice((I - 1) // bm * bm, I)
            assert _rel(wrong[band], ref[band]) > 10 * TOL
            wrong = ref.clone()
            wrong[:, -1] = ref[:, -2]
            band = slice((J - 1) // bn * bn, J)
            assert _rel(wrong[:, band], ref[:, band]) > 10 * TOL


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
def test_bounds_discriminate_skipped_operand_rounding(prec):
    """A 16-bit kernel that multiplied its operands as stored (no rounding on the way into LDS) misses TOL by 10x at the
    contractions of the forced-tile sweep; one operand rounded twice as coarsely, or one not at all, by 10x from Kc = 70.  (The
    effect does not grow with Kc while the bound does: beyond Kc = 2048 the margin shrinks, to 5x under fp16 at Kc = 16384.)"""
    for I, J, Kc in ((64, 64, 4), (130, 67, 70), (200, 192, 130)):
        a, b = (_rnd64(I, Kc, seed=I) / math.sqrt(Kc)).float(), _rnd64(J, Kc, seed=J).float()
        ref = r16(a, prec) @ r16(b, prec).t()
        assert _rel(a.double() @ b.double().t(), ref) > 10 * TOL
        if Kc >= 70:
            assert _rel(r16(a, prec) @ b.double().t(), ref) > 10 * TOL and _rel(a.double() @ r16(b, prec).t(), ref) > 10 * TOL


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
def test_bounds_discriminate_db_stored_vs_rounded(prec):
    """db from the rounded dY where the stored fp32 dY is documented, and the other way round: with the off-grid dY of
    check_dw16 either misses the db bound by 10x from M = 63 on.  (At M = 1 the two differ by DELTA itself: 19x the bound under
    bf16, 4.6x under fp16.)"""
    for M in DW_M[1:] + (4096, 20480):
        dy = dy_off_grid(M, 136, prec, seed=M)
        stored, rounded = dy.double().sum(0), r16(dy, prec).sum(0)
        for blk in range(0, 136, 128):
            s, r = stored[blk:blk + 128], rounded[blk:blk + 128]
            assert _rel(r, s) > 10 * bound(M, True) and _rel(s, r) > 10 * bound(M, True), (M, _rel(r, s))
    dy = dy_off_grid(1, 136, prec, seed=1)
    assert _rel(r16(dy, prec).sum(0), dy.double().sum(0)) > 4 * TOL_ATOMIC


def round_once(v64, prec):
    """float64 -> the 16-bit type's grid in ONE round-to-nearest-even, as float64 (fp16: fewer bits below 2^-14)."""
    m, e = torch.frexp(v64)
    scale = torch.full_like(v64, 2.0 ** 8) if prec == 1 else torch.exp2(torch.clamp(e + 24, max=11).double())
    return torch.ldexp(torch.round(m * scale) / scale, e)


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
def test_bounds_discriminate_c16_double_rounding(prec):
    """A 16-bit C rounded once from the exact result is not the fp32 result rounded: at the inputs of
    test_c16_is_the_fp32_result_rounded_once the two differ in at least one element, so torch.equal tells them apart."""
    I, J, Kc, dY, W, Z = c16_inputs(prec)
    exact = 0.5 * (r16(dY, prec) @ r16(W, prec).t()) * dswish(Z.double())
    assert torch.equal(round_once(exact.float().double(), prec), exact.float().to(DT16[prec]).double())     # round_once is the cast
    flips = int((round_once(exact, prec) != exact.float().to(DT16[prec]).double()).sum())
    assert flips >= 1, flips
