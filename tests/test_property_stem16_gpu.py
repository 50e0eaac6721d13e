"""Property-based sweep of the conv-subsampling stem's implicit-GEMM kernels along the block-tile dimension (the stem's
counterpart of tests/test_property_gemm_gpu.py, whose helpers and bounds it shares).

Under torch.autocast the stem's second convolution and its input gradient run on the 16-bit GEMM kernel (csrc/gemm_mfma16.hip):
CONV = 1 gathers the 3x3 / stride-2 windows of h1, CONV = 2 runs the transposed convolution as four parity classes with a per-tap
row validity and scattered output rows.  launch_t picks the block tile from M = B*T2*F2 (the class's row count for the gradient)
and C, so batch size and utterance length decide which instantiation runs; csrc/gemm_split.hip does the same for the split-plane
convolution.  One test per (entry, tile) cell, every operand form and both 16-bit types in each; the C entries are called directly
and every call asserts the tile it recorded (cfm_debug_gemm_last_tile) against the launch rule restated here.

Reference: a float64 conv2d with stride 2 (or its transpose) of the operands rounded to the 16-bit type wherever the kernel rounds
them (w2 always; h1 / dz2 whether supplied in 16 bits or as fp32 that the kernel rounds while staging); fp32 bias.  The bound is
the GEMM sweep's TOL = 2e-5 rel-L2 (TOL_SPLIT for the split-plane form), applied per checked window and never per tensor: the
whole output at small shapes; at large shapes the first 12, the middle 12 and the last 12 output frames of the first and of the
last utterance, the reference's input sliced to the frames each window needs.  The rows of the last row tile of the tile that ran
are checked on their own.  Exact properties are asserted bitwise: every tile and every operand form gives the same bits (same
MFMA, same K order, same epilogue; staging rounds to nearest-even as torch does), a 16-bit output equals the fp32 output of the
same call form converted with .to(dtype), and the 16-bit producers (conv1, LayerNorm, depthwise conv) equal their fp32 twins
rounded.  The CPU tests at the end check that each plausible wrong answer misses its bound by 10x or more.

Measured on an MI355X, worst rel-L2 against float64 over every check of the cell (bound 2e-5), bf16 / fp16:
    forward conv2       64x64 3.4e-7 / 4.3e-7    128x128 2.4e-7 / 3.1e-7    256x256 3.4e-7 / 4.3e-7
    input gradient dh1  64x64 1.5e-7 / 1.7e-7    256x256 and 128x128 (one call) 1.5e-7 / 1.7e-7
Split-plane conv2, planes 3 (bound 2e-6) / planes 2 (bound 1e-4) / the native fp32 kernel on the same input:
    64x64 (K = 1152) 5.0e-7 / 4.6e-6 / 4.3e-7    128x64 (K = 2304) 7.1e-7 / 4.7e-6 / 6.2e-7    128x128 (K = 2304) 7.1e-7 / 4.6e-6 / 6.1e-7
so planes = 3 holds 2e-6 at K = 2304 as it stands, within 1.2x of the native kernel's error.
The conv kernels passed every cell as they were.  One kernel bug was found, in cell (cfm_dwconv_bn_swish_fwd_out16_f32, fp16, every K,
C >= 72): the compiler folded the last fp32 multiply of Swish into the conversion (v_fma_mixlo_f16: one rounding, straight to
fp16), so wherever the fp32 product rounds onto an fp16 tie (one element in about 2^13) the result was one fp16 ulp away from the
fp32 kernel's, rounded.  csrc/dwconv.hip now converts the
fp32 value (f32_value in csrc/cfm_common.h); the bf16 and fp32 instantiations are unchanged.
"""
import math

import pytest
import torch
import torch.nn.functional as Fn

hypothesis = pytest.importorskip("hypothesis")
from hypothesis import example, given, settings, strategies as st  # noqa: E402

from tests.test_property_gemm_gpu import DT16, F16, FSPLIT, SET, TOL, TOL_SPLIT, force16, grnd, last_tile, lib  # noqa: E402
from tests.util import rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
PRECS = pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
WORST = {}                                   # (entry, tile, type) -> the worst rel-L2 against float64 seen in this run


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conformer_amd import _lib, ops as _ops
    assert _lib.load().cfm_device_check() == 0, "not a gfx950 device"
    yield _ops
    _lib.load().cfm_debug_gemm_mfma16_force_tile(0)
    for key in sorted(WORST):
        print(f"worst rel-L2 against float64 {key}: {WORST[key]:.2e}")


def check_status(st_, what):
    from conformer_amd import _lib
    _lib.check(st_, what)


# ---- the launch rules, restated ---------------------------------------------------------------------------------------------
def conv_tile16(M, C, form, force=0):
    """launch_t of csrc/gemm_mfma16.hip for CONV != 0: (BM, BN, waves).  form: 0 fp32 operands, 1 16-bit W, 2 16-bit A and W."""
    if form >= 1 and C % 256 == 0 and force != 1 and -(-M // 256) * (C // 256) >= 224:
        return (256, 256, 8)
    if -(-M // 128) * -(-C // 128) >= 512 and force < 4:
        return (128, 128, 4)
    return (64, 64, 4)


def conv_tile_split(M, C):
    """launch of csrc/gemm_split.hip (ReLU epilogue)."""
    rows128 = -(-M // 128)
    if rows128 * -(-C // 128) >= 400:
        return (128, 128, 4)
    if rows128 * -(-C // 64) >= 400:
        return (128, 64, 4)
    return (64, 64, 4)


def class_rows(B, T1, F1):
    """Row counts of the four parity classes (pt, pf) of the input gradient: t1 = 2a + pt, f1 = 2c + pf."""
    return [B * ((T1 - pt + 1) // 2) * ((F1 - pf + 1) // 2) for pt in (0, 1) for pf in (0, 1)]


# ---- checked windows ----------------------------------------------------------------------------------------------------------
def windows(B, T):
    """(utterance, first frame, end) of the checked windows along an axis of T frames: everything up to 36 frames, else the first,
    the middle and the last 12 frames of the first and of the last utterance."""
    if T <= 36:
        return [(u, 0, T) for u in range(B)]
    return [(u, a, a + 12) for u in sorted({0, B - 1}) for a in (0, T // 2 - 6, T - 12)]


def got_rows(out, segs, skip):
    """The rows (positions x C, float64) of `out` (B, T, F, C) in the frame segments [(utterance, first, end)], less `skip` rows."""
    return torch.cat([out[u, a:b].reshape(-1, out.shape[-1]) for u, a, b in segs])[skip:].double().cpu()


def assert_windows(out, checks, tol, key, what):
    """rel-L2 of every check (label, segments, rows skipped, float64 rows) on its own."""
    errs = []
    for label, segs, skip, ref in checks:
        got = got_rows(out, segs, skip)
        e = rel_l2(got, ref) if bool(torch.isfinite(got).all()) else float("inf")
        errs.append((label, e))
        WORST[key] = max(WORST.get(key, 0.0), e)
    print(f"{key} {what}: " + ", ".join(f"{la} {e:.2e}" for la, e in errs))
    bad = [(la, f"{e:.2e}") for la, e in errs if not e < tol]
    assert not bad, f"{key} {what}: past {tol:.0e}: {bad}"


# ==== 1. forward conv2 on the 16-bit kernel ====================================================================================
class Fwd:
    """Operands of one conv2 shape in every form the entry takes, and the float64 reference of its windows (computed once)."""

    def __init__(self, ops, prec, B, T1, F1, C, seed, rounded=True):
        self.ops, self.prec, self.dt = ops, prec, DT16[prec] if rounded else torch.float32
        self.B, self.T1, self.F1, self.C = B, T1, F1, C
        self.T2, self.F2 = (T1 - 1) // 2, (F1 - 1) // 2
        self.M = B * self.T2 * self.F2
        self.h1 = grnd(B, T1, F1, C, seed=seed).relu_()
        self.w2 = grnd(C, C, 3, 3, seed=seed + 1, scale=1 / math.sqrt(9 * C))
        self.b2 = grnd(C, seed=seed + 2, scale=0.1)
        self.w2p = ops.pack_conv2_weight(self.w2)                       # (co, kf, kt, ci)
        self.w16 = self.w2p.to(self.dt) if rounded else None
        self._h16 = None
        self._w64, self._b64 = self.w2.to(self.dt).double().cpu(), self.b2.double().cpu()
        self._refs = {}

    def h16(self):
        if self._h16 is None:
            self._h16 = self.h1.to(self.dt)
        return self._h16

    def out(self, h2_16=False):
        return torch.full((self.B, self.T2, self.F2, self.C), NAN, device="cuda", dtype=self.dt if h2_16 else torch.float32)

    def run(self, form, h2_16=False, out=None):
        h1 = self.h16() if form == 2 else self.h1
        w = self.w16 if form >= 1 else self.w2p
        h2 = self.out(h2_16) if out is None else out
        check_status(lib().cfm_subsample_conv2_relu_mfma16_f32(self.prec, h1.data_ptr(), int(form == 2), w.data_ptr(), int(form >= 1),
                                                               self.b2.data_ptr(), h2.data_ptr(), int(h2_16), self.B, self.F1,
                                                               self.T1, self.C, self.ops._stream()),
                     "cfm_subsample_conv2_relu_mfma16_f32")
        return h2

    def ref(self, u, a, b):
        """Output frames [a, b) of utterance u, (b - a, F2, C) float64, from the h1 frames [2a, 2b] they read."""
        if (u, a, b) not in self._refs:
            x = self.h1[u, 2 * a:2 * b + 1].to(self.dt).double().cpu()             # (frames, F1, C)
            y = Fn.conv2d(x.permute(2, 1, 0)[None], self._w64, self._b64, stride=2).relu()   # (1, C, F2, b - a)
            self._refs[(u, a, b)] = y[0].permute(2, 1, 0).contiguous()
        return self._refs[(u, a, b)]

    def checks(self, bm):
        """The windows, and the rows of the last row tile of a tile bm rows high on their own."""
        C, T2, F2 = self.C, self.T2, self.F2
        out = [(f"u{u}[{a},{b})", [(u, a, b)], 0, self.ref(u, a, b).reshape(-1, C)) for u, a, b in windows(self.B, T2)]
        r0 = (self.M - 1) // bm * bm                                    # first row of the last row tile; row = (u*T2 + t2)*F2 + f2
        g0 = r0 // F2
        segs = [(u, max(g0 - u * T2, 0), T2) for u in range(g0 // T2, self.B)]
        skip = r0 - g0 * F2
        ref = torch.cat([self.ref(u, a, b).reshape(-1, C) for u, a, b in segs])[skip:]
        assert ref.shape[0] == self.M - r0
        return out + [(f"last row tile of {bm}", segs, skip, ref)]


def _run_fwd(ops, prec, B, T1, F1, C, seed, forms, tile, every_tile=False):
    """Every form with an fp32 and a 16-bit h2 on the tile the shape picks; every_tile: the same bits on the 4-wave tiles by shape
    (force 1) and on the 64x64 tile with fp32 operands (force 5)."""
    c = Fwd(ops, prec, B, T1, F1, C, seed)
    name = "bf16" if prec == 1 else "fp16"
    base = None
    for form in forms:
        want = conv_tile16(c.M, C, form)
        assert want == tile, (c.M, C, form, want)
        h2 = c.run(form)
        rec = last_tile(F16)
        assert rec[:3] == tile and rec[4] == form and rec[5] == 0, (form, rec)
        assert_windows(h2, c.checks(tile[0]), TOL, ("conv2 fwd", f"{tile[0]}x{tile[1]}", name), f"{(B, T1, F1, C)} form {form}")
        base = h2 if base is None else base
        assert torch.equal(h2, base), f"form {form}: bits differ from form {forms[0]}"
        h2_16 = c.run(form, h2_16=True)
        rec = last_tile(F16)
        assert rec[:3] == tile and rec[4] == form and rec[5] == 1, (form, rec)
        assert torch.equal(h2_16, h2.to(c.dt)), f"form {form}: 16-bit h2 != fp32 h2 rounded"
        del h2_16
    if every_tile:
        with force16(5):
            b64 = c.run(0)
        assert last_tile(F16)[:3] == conv_tile16(c.M, C, 0, 5) == (64, 64, 4)
        assert_windows(b64, c.checks(64), TOL, ("conv2 fwd", "64x64", name), f"{(B, T1, F1, C)} force 5, fp32 operands")
        assert torch.equal(base, b64), f"{tile}: bits differ from the 64x64 tile on fp32 operands"
        del b64
        if tile != (128, 128, 4):
            for form in forms:
                with force16(1):
                    b128 = c.run(form)
                rec = last_tile(F16)
                assert rec[:3] == conv_tile16(c.M, C, form, 1) == (128, 128, 4) and rec[4] == form, rec
                assert torch.equal(base, b128), f"{tile} form {form}: bits differ from the 128x128 tile"
                del b128
    # the entry refuses a 16-bit h1 with fp32 weights, and writes nothing
    h2 = c.out()
    st_ = lib().cfm_subsample_conv2_relu_mfma16_f32(prec, c.h16().data_ptr(), 1, c.w2p.data_ptr(), 0, c.b2.data_ptr(), h2.data_ptr(), 0,
                                                    B, F1, T1, C, ops._stream())
    assert st_ != 0 and bool(torch.isnan(h2).all())


@PRECS
@settings(max_examples=4, **SET)
@given(B=st.integers(1, 3), T1=st.integers(3, 24), F1=st.integers(3, 24), C=st.sampled_from([64, 128, 192]), seed=st.integers(0, 10 ** 6))
@example(B=1, T1=3, F1=3, C=64, seed=1).via("M = 1")
@example(B=2, T1=4, F1=6, C=64, seed=2).via("even T1 and F1: the last input row and column are never read")
@example(B=3, T1=21, F1=13, C=128, seed=3).via("M = 180: ragged against 64")
@example(B=2, T1=9, F1=39, C=192, seed=4).via("N not a multiple of 128")
def test_conv2_fwd_64x64(ops, prec, B, T1, F1, C, seed):
    _run_fwd(ops, prec, B, T1, F1, C, seed, (0, 1, 2), (64, 64, 4))


@PRECS
def test_conv2_fwd_128x128_by_shape(ops, prec):
    """M = 32718 = 255 x 128 + 78: 256 x 2 = 512 tiles of 128x128, every operand form; the same bits on the 64x64 tile."""
    _run_fwd(ops, prec, 7, 493, 39, 256, 11, (0, 1, 2), (128, 128, 4), every_tile=True)


FWD_256 = [  # (B, T1, F1, C), tile: both sides of the 8-wave tile's threshold (16-bit weights on every line)
    ((16, 447, 33, 256), (128, 128, 4)),    # M = 57088: 223 row tiles of 256
    ((16, 449, 33, 256), (256, 256, 8)),    # M = 57344: 224
    ((12, 503, 39, 256), (256, 256, 8)),    # M = 57228 = 223 x 256 + 140: a ragged last tile
    ((6, 501, 39, 512), (256, 256, 8)),     # M = 28500 = 111 x 256 + 84, two column tiles: the benchmark's width
]


@PRECS
@pytest.mark.parametrize("shape,tile", FWD_256, ids=["x".join(map(str, s)) for s, _ in FWD_256])
def test_conv2_fwd_256x256_threshold(ops, prec, shape, tile):
    """The 8-wave tile and the 128x128 tile just below it: float64 windows, the same bits as the 128x128 tile (force 1) and as the
    64x64 tile on fp32 operands (force 5; fp32 weights never take the 8-wave tile)."""
    _run_fwd(ops, prec, *shape, 21, (1, 2), tile, every_tile=True)


# ==== 2. input gradient dh1 ======================================================================================================
class Bwd:
    def __init__(self, ops, prec, B, T1, F1, C, seed):
        self.ops, self.prec, self.dt = ops, prec, DT16[prec]
        self.B, self.T1, self.F1, self.C = B, T1, F1, C
        self.T2, self.F2 = (T1 - 1) // 2, (F1 - 1) // 2
        self.dz2 = grnd(B, self.T2, self.F2, C, seed=seed)
        self.w2 = grnd(C, C, 3, 3, seed=seed + 1, scale=1 / math.sqrt(9 * C))
        w2c = torch.empty(9 * C * C, device="cuda")
        check_status(lib().cfm_pack_conv2_weight_t_f32(self.w2.data_ptr(), w2c.data_ptr(), C, ops._stream()), "cfm_pack_conv2_weight_t_f32")
        self.w2c16 = w2c.to(self.dt)
        self.zb = torch.zeros(C, device="cuda")
        self._w64 = self.w2.to(self.dt).double().cpu()
        self._refs = {}

    def run(self, form, d16=False, dz2=None, out=None):
        """form 1: fp32 dz2 (rounded while staging), 2: dz2 stored in the 16-bit type; d16: the _out16_ entry."""
        dz2 = self.dz2 if dz2 is None else dz2
        B = dz2.shape[0]
        a = dz2.to(self.dt) if form == 2 else dz2
        dh1 = torch.full((B, self.T1, self.F1, self.C), NAN, device="cuda", dtype=self.dt if d16 else torch.float32) if out is None else out
        fn = lib().cfm_subsample_conv2_bwd_input_fwdkernel_out16_mfma16_f32 if d16 else lib().cfm_subsample_conv2_bwd_input_fwdkernel_mfma16_f32
        check_status(fn(self.prec, a.data_ptr(), int(form == 2), self.w2c16.data_ptr(), self.zb.data_ptr(), dh1.data_ptr(), B, self.F1,
                        self.T1, self.C, self.ops._stream()), "cfm_subsample_conv2_bwd_input_fwdkernel_mfma16_f32")
        return dh1

    def ref(self, dz2, tag, u, a, b):
        """dh1 frames [a, b) of utterance u of dz2, (b - a, F1, C) float64: the transposed convolution of the dz2 frames that reach them."""
        key = (tag, u, a, b)
        if key not in self._refs:
            lo, hi = max(0, (a - 1) // 2), min(self.T2, (b - 1) // 2 + 1)           # t2 with [2 t2, 2 t2 + 2] meeting [a, b)
            out = torch.zeros(b - a, self.F1, self.C, dtype=torch.float64)
            if hi > lo:
                d = dz2[u, lo:hi].to(self.dt).double().cpu().permute(2, 1, 0)[None]  # (1, C, F2, frames)
                y = Fn.conv_transpose2d(d, self._w64, stride=2, output_padding=(self.F1 - (2 * self.F2 + 1), 0))
                y = y[0].permute(2, 1, 0)                                           # frames [2 lo, 2 hi + 1) x F1 x C
                s0, s1 = max(a, 2 * lo), min(b, 2 * hi + 1)
                out[s0 - a:s1 - a] = y[s0 - 2 * lo:s1 - 2 * lo]
            self._refs[key] = out
        return self._refs[key]

    def checks(self, dz2, tag, bm):
        """The windows along T1, and on their own the last frames of the last utterance: they hold the last row tile (bm class rows)
        of every class."""
        B, T1, C = dz2.shape[0], self.T1, self.C
        out = [(f"u{u}[{a},{b})", [(u, a, b)], 0, self.ref(dz2, tag, u, a, b).reshape(-1, C)) for u, a, b in windows(B, T1)]
        n = min(T1, 2 * -(-bm // (self.F1 // 2)) + 2)
        return out + [(f"last {n} frames (last row tiles of {bm})", [(B - 1, T1 - n, T1)], 0, self.ref(dz2, tag, B - 1, T1 - n, T1).reshape(-1, C))]


def assert_unreached_zero(dh1, T1, F1):
    """Positions no tap reaches (the last frame of an even T1, the last column of an even F1) are written, as exact zeros."""
    assert not bool(torch.isnan(dh1.float()).any()), "dh1 elements left unwritten"
    if T1 % 2 == 0:
        assert bool((dh1[:, -1] == 0).all())
    if F1 % 2 == 0:
        assert bool((dh1[:, :, -1] == 0).all())


def _run_bwd(c, dz2, tag, name):
    """Both entries with dz2 as fp32 and as 16 bits; returns the fp32 dh1 of the fp32-dz2 call."""
    B, T1, F1, C = dz2.shape[0], c.T1, c.F1, c.C
    tile = conv_tile16(class_rows(B, T1, F1)[3], C, 1)                  # the record shows the last class (pt = pf = 1)
    base = None
    for form in (1, 2):
        dh1 = c.run(form, dz2=dz2)
        rec = last_tile(F16)
        assert rec[:3] == tile and rec[4] == form and rec[5] == 0, (form, rec)
        assert_unreached_zero(dh1, T1, F1)
        assert_windows(dh1, c.checks(dz2, tag, tile[0]), TOL, ("conv2 dh1", f"{tile[0]}x{tile[1]}", name), f"{(B, T1, F1, C)} form {form}")
        base = dh1 if base is None else base
        assert torch.equal(dh1, base), "16-bit dz2: bits differ from the fp32 dz2 the kernel rounds"
        d16 = c.run(form, d16=True, dz2=dz2)
        rec = last_tile(F16)
        assert rec[:3] == tile and rec[4] == form and rec[5] == 1, (form, rec)
        assert_unreached_zero(d16, T1, F1)
        assert torch.equal(d16, dh1.to(c.dt)), f"form {form}: 16-bit dh1 != fp32 dh1 rounded"
    return base


@PRECS
@settings(max_examples=4, **SET)
@given(B=st.integers(1, 3), T1=st.integers(3, 24), F1=st.integers(3, 24), C=st.sampled_from([64, 128]), seed=st.integers(0, 10 ** 6))
@example(B=1, T1=3, F1=3, C=64, seed=1).via("one output position per class")
@example(B=2, T1=4, F1=6, C=64, seed=2).via("even T1 and F1: the last row and column of dh1 are exact zeros")
@example(B=3, T1=22, F1=13, C=128, seed=3).via("even T1, odd F1, ragged against 64")
def test_conv2_bwd_input_64x64(ops, prec, B, T1, F1, C, seed):
    c = Bwd(ops, prec, B, T1, F1, C, seed)
    assert all(conv_tile16(m, C, 1) == (64, 64, 4) for m in class_rows(B, T1, F1))
    _run_bwd(c, c.dz2, "all", "bf16" if prec == 1 else "fp16")


@PRECS
def test_conv2_bwd_input_big_tiles(ops, prec):
    """(12, 499, 39, 256): the classes have 60000, 57000, 59760 and 56772 rows, so one call runs the 256x256 kernel (classes 0, 2)
    and the 128x128 kernel (1, 3).  dh1 of utterances 0, 5 and 11 bitwise equal to the three-utterance sub-batch computed alone (the
    64x64 tile), that one against float64; the big call's last frames (the last row tile of every class) against float64 too."""
    B, T1, F1, C = 12, 499, 39, 256
    name = "bf16" if prec == 1 else "fp16"
    rows = class_rows(B, T1, F1)
    assert rows == [60000, 57000, 59760, 56772]
    assert [conv_tile16(m, C, 1)[0] for m in rows] == [256, 128, 256, 128]
    assert all(conv_tile16(m, C, 1) == (64, 64, 4) for m in class_rows(3, T1, F1))
    c = Bwd(ops, prec, B, T1, F1, C, 31)
    pick = [0, 5, 11]
    sub = c.dz2[pick].contiguous()
    sub_dh1 = _run_bwd(c, sub, "sub", name)
    n = 2 * -(-256 // (F1 // 2)) + 2
    tail = [(f"last {n} frames of utterance 11", [(B - 1, T1 - n, T1)], 0, c.ref(sub, "sub", 2, T1 - n, T1).reshape(-1, C))]
    for form in (1, 2):
        for d16 in (False, True):
            dh1 = c.run(form, d16=d16)
            rec = last_tile(F16)
            assert rec[:3] == (128, 128, 4) and rec[4] == form and rec[5] == int(d16), rec
            assert_unreached_zero(dh1[pick], T1, F1)
            if not d16:
                assert_windows(dh1, tail, TOL, ("conv2 dh1", "256x256+128x128", name), f"form {form}")
            assert torch.equal(dh1[pick], sub_dh1.to(c.dt) if d16 else sub_dh1), f"form {form} 16-bit dh1 {d16}: bits differ from the sub-batch"
            del dh1


# ==== 3. split-plane conv2 =======================================================================================================
SPLIT = {  # cell -> (B, T1, F1, C)
    "64x64": (3, 21, 13, 128),              # M = 180
    "128x64": (4, 337, 39, 256),            # M = 12768: 100 row tiles x 4 column tiles of 64 = 400
    "128x128": (7, 385, 39, 256),           # M = 25536: 200 row tiles (ragged) x 2
}


def split_conv2(ops, c, planes, out=None):
    ws = ops.weight_split(c.w2p.view(c.C, 9 * c.C), planes)
    h2 = c.out() if out is None else out
    check_status(lib().cfm_subsample_conv2_relu_split_bf16_f32(planes, c.h1.data_ptr(), ws.data_ptr(), c.b2.data_ptr(), h2.data_ptr(), c.B,
                                                               c.F1, c.T1, c.C, ops._stream()), "cfm_subsample_conv2_relu_split_bf16_f32")
    return h2


@pytest.mark.parametrize("planes", [3, 2], ids=["bf16x6", "bf16x3"])
@pytest.mark.parametrize("cell", list(SPLIT))
def test_conv2_split_plane_every_tile(ops, planes, cell):
    """fp32 operands, float64 of the same operands; K = 9C = 2304 at the two large tiles."""
    B, T1, F1, C = SPLIT[cell]
    c = Fwd(ops, 0, B, T1, F1, C, 41, rounded=False)
    tile = conv_tile_split(c.M, C)
    assert f"{tile[0]}x{tile[1]}" == cell
    h2 = split_conv2(ops, c, planes)
    rec = last_tile(FSPLIT)
    assert rec[:3] == tile and rec[4] == planes, rec
    checks = c.checks(tile[0])
    native = c.out()
    check_status(lib().cfm_subsample_conv2_relu_f32(c.h1.data_ptr(), c.w2p.data_ptr(), c.b2.data_ptr(), native.data_ptr(), B, F1, T1, C,
                                                    ops._stream()), "cfm_subsample_conv2_relu_f32")
    e_native = {label: rel_l2(got_rows(native, segs, skip), ref) for label, segs, skip, ref in checks}
    print(f"native fp32 conv2 {cell} K = {9 * C}: " + ", ".join(f"{la} {e:.2e}" for la, e in e_native.items()))
    WORST[("conv2 native fp32", cell, "fp32")] = max(e_native.values())

    # K = 2304, measured: planes 3 7.1e-7 next to the native kernel's 6.2e-7, so the plain 2e-6 holds; planes 2 4.7e-6
    assert_windows(h2, checks, TOL_SPLIT[planes], ("conv2 split", cell, f"planes {planes}"), str(SPLIT[cell]))


# ==== 4a. writes stay inside the outputs: one example per tile, the output carved out of sentinel bytes ========================
GUARD = [  # (what, kind, (B, T1, F1, C), form / planes, 16-bit output, tile of the (last) launch)
    ("fwd 64x64", "fwd", (3, 21, 13, 128), 2, True, (64, 64, 4)),
    ("fwd 128x128", "fwd", (7, 493, 39, 256), 0, False, (128, 128, 4)),
    ("fwd 256x256", "fwd", (12, 503, 39, 256), 2, True, (256, 256, 8)),
    ("fwd 256x256 two column tiles", "fwd", (6, 501, 39, 512), 1, False, (256, 256, 8)),
    ("dh1 64x64", "bwd", (3, 22, 13, 128), 1, False, (64, 64, 4)),
    ("dh1 256x256 + 128x128", "bwd", (12, 499, 39, 256), 2, True, (128, 128, 4)),
    ("split 64x64", "split", SPLIT["64x64"], 3, False, (64, 64, 4)),
    ("split 128x64", "split", SPLIT["128x64"], 2, False, (128, 64, 4)),
    ("split 128x128", "split", SPLIT["128x128"], 3, False, (128, 128, 4)),
]


@pytest.mark.parametrize("case", GUARD, ids=[g[0] for g in GUARD])
def test_writes_stay_inside_the_outputs(ops, case):
    from tests.test_write_guard_gpu import guarded_allocations
    what, kind, (B, T1, F1, C), form, o16, tile = case
    with guarded_allocations() as gt:
        if kind == "bwd":
            c = Bwd(ops, 1, B, T1, F1, C, 51)
            out = gt.full((B, T1, F1, C), NAN, dtype=c.dt if o16 else torch.float32, device="cuda")
            c.run(form, d16=o16, out=out)
            fam = F16
        else:
            c = Fwd(ops, 1, B, T1, F1, C, 51, rounded=kind == "fwd")
            out = gt.full((B, c.T2, c.F2, C), NAN, dtype=c.dt if o16 else torch.float32, device="cuda")
            if kind == "fwd":
                c.run(form, h2_16=o16, out=out)
            else:
                split_conv2(ops, c, form, out=out)
            fam = F16 if kind == "fwd" else FSPLIT
        rec = last_tile(fam)
        bad = gt.check()
    assert rec[:3] == tile, (what, rec)
    assert len(gt.allocs) >= 1 and not bad, f"{what}: {bad}"
    assert bool(torch.isfinite(out.float()).all())


# ==== 4b. the 16-bit producers, bitwise against their fp32 twins ================================================================
@pytest.mark.parametrize("C", [8, 12, 36, 64, 144, 512, 1024])
def test_conv1_out16_equals_fp32_rounded(ops, C):
    """cfm_subsample_conv1_relu_out16_f32 (eight channels per thread where C % 8 == 0, else four; its own thread-to-channel map and
    positions per workgroup) against the fp32 kernel rounded, and the fp32 kernel against float64.  Bound of the latter: ten fp32
    roundings (nine fmaf and the bias) of at most 2^-24 each relative to the running sum, so 10 x 2^-24 = 6e-7 of sum |terms|, which
    for normal data is within 3x of the output's norm: 2e-6."""
    B = 2
    for F in (3, 7, 80, 81):
        for T in (3, 8, 57):
            F1, T1 = (F - 1) // 2, (T - 1) // 2
            x = grnd(B, F, T, seed=F * 100 + T)
            w1, b1 = grnd(C, 1, 3, 3, seed=C, scale=1 / 3), grnd(C, seed=C + 1, scale=0.1)
            h32 = torch.full((B, T1, F1, C), NAN, device="cuda")
            check_status(lib().cfm_subsample_conv1_relu_f32(x.data_ptr(), w1.data_ptr(), b1.data_ptr(), h32.data_ptr(), B, F, T, C,
                                                            ops._stream()), "cfm_subsample_conv1_relu_f32")
            ref = Fn.conv2d(x.double().cpu()[:, None], w1.double().cpu(), b1.double().cpu(), stride=2).relu().permute(0, 3, 2, 1)
            e = rel_l2(h32, ref) if bool(torch.isfinite(h32).all()) else float("inf")
            assert e < 2e-6, (C, F, T, e)
            for prec in (1, 2):
                h16 = torch.full((B, T1, F1, C), NAN, device="cuda", dtype=DT16[prec])
                check_status(lib().cfm_subsample_conv1_relu_out16_f32(prec, x.data_ptr(), w1.data_ptr(), b1.data_ptr(), h16.data_ptr(), B, F,
                                                                      T, C, ops._stream()), "cfm_subsample_conv1_relu_out16_f32")
                assert torch.equal(h16, h32.to(DT16[prec])), (C, F, T, prec)


@pytest.mark.parametrize("rows", [1, 5, 4097])
@pytest.mark.parametrize("d", [132, 388, 772, 1540, 2564])
def test_layernorm_out16_equals_fp32_rounded(ops, d, rows):
    """One ragged d in each width class of layernorm_launch (<= 256, 512, 1024, 2048, above), with and without mean / rstd."""
    x = grnd(rows, d, seed=d + rows, scale=1.7, shift=0.4)
    ga, be = grnd(d, seed=d, scale=0.3, shift=1.0), grnd(d, seed=d + 1, scale=0.2)
    y32, mean32, rstd32 = torch.full((rows, d), NAN, device="cuda"), torch.full((rows,), NAN, device="cuda"), torch.full((rows,), NAN, device="cuda")
    check_status(lib().cfm_layernorm_fwd_f32(x.data_ptr(), ga.data_ptr(), be.data_ptr(), y32.data_ptr(), mean32.data_ptr(), rstd32.data_ptr(),
                                             rows, d, 1e-5, ops._stream()), "cfm_layernorm_fwd_f32")
    assert bool(torch.isfinite(y32).all())
    for prec in (1, 2):
        for stats in (False, True):
            y16 = torch.full((rows, d), NAN, device="cuda", dtype=DT16[prec])
            mean, rstd = torch.full((rows,), NAN, device="cuda"), torch.full((rows,), NAN, device="cuda")
            check_status(lib().cfm_layernorm_fwd_out16_f32(prec, x.data_ptr(), ga.data_ptr(), be.data_ptr(), y16.data_ptr(),
                                                           mean.data_ptr() if stats else None, rstd.data_ptr() if stats else None, rows, d,
                                                           1e-5, ops._stream()), "cfm_layernorm_fwd_out16_f32")
            assert torch.equal(y16, y32.to(DT16[prec])), (d, rows, prec, stats)
            if stats:
                assert torch.equal(mean, mean32) and torch.equal(rstd, rstd32)


@pytest.mark.parametrize("C", [8, 72, 512])
@pytest.mark.parametrize("K", [3, 7, 15, 31])
def test_dwconv_out16_equals_fp32_rounded(ops, K, C):
    """T below K (every window clipped on both sides) and across the 64 frames of a workgroup; C off and on the 64-channel block.
    (fp16 differed by one ulp in a few elements until the kernel converted the fp32 value: the module docstring.)"""
    B = 2
    w, bias = grnd(C, K, seed=K, scale=1 / math.sqrt(K)), grnd(C, seed=K + 1, scale=0.1)
    bn_w, bn_b = grnd(C, seed=K + 2, scale=0.3, shift=1.0), grnd(C, seed=K + 3, scale=0.2)
    bn_m, bn_v = grnd(C, seed=K + 4, scale=0.2), grnd(C, seed=K + 5).abs() + 0.5
    for T in sorted({1, K - 1, 63, 64, 65, 130}):
        g = grnd(B, T, C, seed=T)
        y32 = torch.full((B, T, C), NAN, device="cuda")
        args = (g.data_ptr(), w.data_ptr(), bias.data_ptr(), bn_w.data_ptr(), bn_b.data_ptr(), bn_m.data_ptr(), bn_v.data_ptr(), 1e-5)
        check_status(lib().cfm_dwconv_bn_swish_fwd_f32(*args, y32.data_ptr(), B, T, C, K, ops._stream()), "cfm_dwconv_bn_swish_fwd_f32")
        assert bool(torch.isfinite(y32).all())
        for prec in (1, 2):
            y16 = torch.full((B, T, C), NAN, device="cuda", dtype=DT16[prec])
            check_status(lib().cfm_dwconv_bn_swish_fwd_out16_f32(prec, *args, y16.data_ptr(), B, T, C, K, ops._stream()),
                         "cfm_dwconv_bn_swish_fwd_out16_f32")
            assert torch.equal(y16, y32.to(DT16[prec])), (K, C, T, prec)


# ==== the bounds are tight enough (CPU, float64) ===============================================================================
def _rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _window(C=256, frames=13, F1=39, seed=0):
    """One checked window at the benchmark's F1: h1 (2 frames + 1, F1, C) >= 0, w2, b2 and the pre-activation (frames, F2, C)."""
    h1 = _rnd(2 * frames + 1, F1, C, seed=seed).relu()
    w2, b2 = _rnd(C, C, 3, 3, seed=seed + 1) / math.sqrt(9 * C), _rnd(C, seed=seed + 2) * 0.1
    return h1, w2, b2


def _conv(h1, w2, b2):
    return Fn.conv2d(h1.permute(2, 1, 0)[None], w2, b2, stride=2)[0].permute(2, 1, 0)


def test_bounds_discriminate_dropped_tap_and_shifted_class_row():
    """One tap (of nine) dropped at one output position of a window, and one class row of dh1 written one class position off."""
    h1, w2, b2 = _window()
    pre = _conv(h1, w2, b2)
    ref = pre.relu()
    for t2, f2, kt, kf in ((0, 0, 0, 0), (6, 9, 1, 2), (12, 18, 2, 2)):
        wrong = pre.clone()
        wrong[t2, f2] -= w2[:, :, kf, kt] @ h1[2 * t2 + kt, 2 * f2 + kf]
        assert rel_l2(wrong.relu(), ref) > 10 * TOL, (t2, f2, kt, kf)
    dz2 = _rnd(1, 256, 19, 6, seed=5)                                      # (1, C, F2, T2): dh1 of 13 frames
    dh1 = Fn.conv_transpose2d(dz2, w2, stride=2)[0].permute(2, 1, 0)       # (13, 39, C)
    for t1, f1 in ((0, 0), (5, 36), (12, 20)):
        wrong = dh1.clone()
        wrong[t1, f1 + 2 if f1 + 2 < 39 else f1 - 2] = dh1[t1, f1]           # the next position of the same class takes the row
        assert rel_l2(wrong, dh1) > 10 * TOL, (t1, f1)


@PRECS
def test_bounds_discriminate_unrounded_h1(prec):
    """A reference of the unrounded h1 (a kernel that skipped the rounding while staging) against the rounded one.  bf16: 1.7e-3.
    fp16: 2.0e-4 to 2.1e-4 at C = 256, which is 10x the bound with nothing to spare (the rms of an 11-bit rounding); what holds the
    kernels there is the bitwise equality of the fp32-h1 forms with the 16-bit-h1 form, whose h1 torch rounds."""
    dt = DT16[prec]
    h1, w2, b2 = _window()
    h1, w2r = h1.float(), w2.float().to(dt).double()
    ref = _conv(h1.to(dt).double(), w2r, b2).relu()
    wrong = _conv(h1.double(), w2r, b2).relu()
    e = rel_l2(wrong, ref)
    print(f"h1 left unrounded, {dt}: {e:.2e}")
    assert e > 10 * TOL
