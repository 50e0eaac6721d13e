"""Property-based shape sweeps of the TRAINING kernels (the backward counterpart of tests/test_property_gpu.py).

Hypothesis draws the geometry (derandomised: the same examples every run, one process) for every backward kernel whose edge
handling depends on it: LayerNorm (both sides of the one-pass / two-kernel split at d = 2048), every route of linear_bwd (fp32,
16-bit operands, 16-bit dY / dx, the swish' epilogue, dropout, the padded dY of N % 4 != 0), depthwise conv + train-mode
BatchNorm + Swish (segment and channel-block raggedness), the conv-subsampling stem, the three LSTM BPTT kernels, CTC (any
blank, every waves-per-workgroup choice of the gradient kernel, the feasibility bound) and the small elementwise pieces.
Reference: torch autograd on the CPU in float64 (through oracle/conformer_oracle.py or a few lines of plain torch); under a
16-bit precision mode the reference takes its GEMM operands rounded to that type.  Each family also asserts, on the CPU in
float64, that a plausible wrong answer lies well outside its tolerance.
"""
import math

import pytest
import torch
import torch.nn.functional as F

hypothesis = pytest.importorskip("hypothesis")
from hypothesis import example, given, settings, strategies as st, HealthCheck  # noqa: E402

from oracle import conformer_oracle as O  # noqa: E402
from tests.util import Calls as _Calls, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 2e-5                   # fp32 kernels
TOL_ATOMIC = 5e-5            # fp32 kernels whose reductions are split over workgroups (atomics / split-K)
TOL16 = {1: 1e-2, 2: 4e-3}   # PREC_BF16 / PREC_FP16 where a kernel rounds INTERMEDIATES to the 16-bit type (LSTM, stem); the
                             # linear_bwd products round their operands only: TOL / TOL_ATOMIC against the rounded operands
DT16 = {1: torch.bfloat16, 2: torch.float16}
SET = dict(deadline=None, derandomize=True, suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conformer_amd import ops as _ops
    return _ops


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def r16(t, prec):
    """t rounded to the 16-bit type of `prec` (identity for fp32), as float64."""
    return (t.to(DT16[prec]) if prec else t).double()


def leaf(t):
    return t.double().clone().requires_grad_(True)


def dswish(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


# ---- 1. LayerNorm: forward statistics + backward (one pass for d <= 2048, dx kernel + parameter kernel above) --------------
def _ln_ref(x, w, b, dy):
    xd, wd, bd = leaf(x), leaf(w), leaf(b)
    F.layer_norm(xd, (x.shape[-1],), wd, bd, 1e-5).backward(dy.double())
    return xd.grad, wd.grad, bd.grad


@settings(max_examples=24, **SET)
@given(rows=st.integers(1, 2000), big=st.booleans(), k=st.integers(1, 512), with_dres=st.booleans(), seed=st.integers(0, 10 ** 6))
@example(rows=1, big=True, k=1, with_dres=True, seed=7).via("d = 8192, one row")
@example(rows=513, big=False, k=512, with_dres=False, seed=8).via("d = 2048: the last one-pass width")
def test_layernorm_train_and_bwd_any_shape(ops, rows, big, k, with_dres, seed):
    """d = 4k on both sides of 2048 (one-pass kernel; dx kernel + parameter kernel), with and without dres."""
    d4 = 2048 - 3 * (k - 1) if big else k            # big: 515 .. 2048 (d = 2060 .. 8192)
    d = 4 * d4
    rows = max(1, min(rows, (1 << 22) // d))            # (CPU float64 autograd budget)
    x = rnd(rows, d, seed=seed) * 2 + 0.5
    w, b, dy = rnd(d, seed=seed + 1), rnd(d, seed=seed + 2), rnd(rows, d, seed=seed + 3)
    dres = rnd(rows, d, seed=seed + 4) if with_dres else None
    y, mean, rstd = ops.layernorm_train(x.cuda(), w.cuda(), b.cuda())
    xd = x.double()
    mu = xd.mean(-1)
    assert rel_l2(y, O.layer_norm(xd, w.double(), b.double())) < TOL
    assert rel_l2(mean, mu) < TOL
    assert rel_l2(rstd, 1 / torch.sqrt(((xd - mu[:, None]) ** 2).mean(-1) + 1e-5)) < TOL
    dx, dw, db = ops.layernorm_bwd(x.cuda(), w.cuda(), dy.cuda(), mean, rstd, dres=None if dres is None else dres.cuda())
    gx, gw, gb = _ln_ref(x, w, b, dy)
    if dres is not None:
        gx = gx + dres.double()
    assert rel_l2(dx, gx) < TOL_ATOMIC
    assert rel_l2(dw, gw) < TOL_ATOMIC and rel_l2(db, gb) < TOL_ATOMIC


def test_layernorm_bwd_tolerance_discriminates():
    """The LayerNorm input gradient without its mean term is far outside the bound."""
    rows, d = 64, 144
    x, w, b, dy = rnd(rows, d, seed=1) * 2 + 0.5, rnd(d, seed=2), rnd(d, seed=3), rnd(rows, d, seed=4)
    gx, _, _ = _ln_ref(x, w, b, dy)
    xd = x.double()
    rs = 1 / torch.sqrt(xd.var(-1, unbiased=False, keepdim=True) + 1e-5)
    xh = (xd - xd.mean(-1, keepdim=True)) * rs
    gy = dy.double() * w.double()
    right = rs * (gy - gy.mean(-1, keepdim=True) - xh * (gy * xh).mean(-1, keepdim=True))
    wrong = rs * (gy - xh * (gy * xh).mean(-1, keepdim=True))
    assert rel_l2(right, gx) < 1e-12
    assert rel_l2(wrong, gx) > 100 * TOL_ATOMIC


# ---- 2. linear_bwd: every route -------------------------------------------------------------------------------------------
def test_dropout_apply_reproduces_the_gemm_mask(ops):
    """dropout_apply(ones, p, seed) is the mask the training GEMM epilogue applied to its (M, N) result (the mask the
    backward replays): the linear_bwd reference below is built from it."""
    M, N, K, p, seed = 77, 52, 36, 0.3, 12345
    a, w, b = rnd(M, K, seed=1), rnd(N, K, seed=2) / 6, rnd(N, seed=3)
    c, z = ops.linear_train("swish", a.cuda(), w.cuda(), b.cuda(), drop_p=p, seed=seed, save_z=True)
    mask = ops.dropout_apply(torch.ones(M, N, device="cuda"), p, seed).cpu()
    vals = torch.unique(mask).tolist()
    assert len(vals) == 2 and vals[0] == 0.0 and abs(vals[1] * (1 - p) - 1) < 1e-6, vals
    assert 0.15 < float((mask == 0).double().mean()) < 0.45
    assert rel_l2(c, O.swish(z.double().cpu()) * mask.double()) < TOL
    other = ops.dropout_apply(torch.ones(M, N, device="cuda"), p, seed + 1).cpu()
    assert not torch.equal(mask, other)


def _linear_bwd_case(ops, M, N, K, prec, data):
    """Draw one linear_bwd call (route flags) for a precision mode; returns the call's inputs and flags."""
    seed = data.draw(st.integers(0, 10 ** 6))
    use_z = data.draw(st.sampled_from([None, "contig", "strided"]))
    f = dict(alpha=data.draw(st.sampled_from([1.0, 0.5, -1.75])),
             need_dx=data.draw(st.booleans()) if use_z is None else True,
             drop_p=data.draw(st.sampled_from([0.0, 0.0, 0.2])) if use_z else 0.0,
             x16=bool(prec) and data.draw(st.booleans()),
             dy16=bool(prec) and data.draw(st.booleans()),
             dx16=bool(prec) and use_z is not None and data.draw(st.booleans()),
             use_z=use_z, drop_seed=seed * 7 + 1)
    x, w, dy = rnd(M, K, seed=seed), rnd(N, K, seed=seed + 1) / math.sqrt(K), rnd(M, N, seed=seed + 2)
    # Z: contiguous, or a column slice of a wider tensor (row stride K + 4: not a multiple of 8 when K is)
    z = None if use_z is None else rnd(M, K + (4 if use_z == "strided" else 0), seed=seed + 3)
    return x, w, dy, z, f


def _run_linear_bwd(ops, prec, x, w, dy, z, f):
    dev = "cuda"
    xg = x.to(dev).to(DT16[prec]) if f["x16"] else x.to(dev)
    dyg = dy.to(dev).to(DT16[prec]) if f["dy16"] else dy.to(dev)
    zg = None if z is None else z.to(dev)[:, :x.shape[1]]
    with ops.precision(prec):
        return ops.linear_bwd(xg, w.to(dev), dyg, alpha=f["alpha"], Z=zg, need_dx=f["need_dx"], drop_p=f["drop_p"],
                              drop_seed=f["drop_seed"], dx16=f["dx16"])


def _linear_bwd_ref(ops, prec, x, w, dy, z, f):
    """(dx, dw, db) in float64.  The products take their operands rounded to the 16-bit type; db sums dY AS STORED (fp32 unless the
    caller stored it in the 16-bit type): neither cfm_colsum_f32 nor the fused weight-gradient kernel rounds what it sums."""
    xr, wr, dyr = r16(x, prec), r16(w, prec), r16(dy, prec)
    dy_stored = dyr if f["dy16"] else dy.double()
    z = None if z is None else z[:, :x.shape[1]]
    a = f["alpha"]
    dx = None
    if f["need_dx"]:
        dx = a * (dyr @ wr)
        if z is not None:
            dx = dx * dswish(z.double())
            if f["drop_p"] > 0:
                dx = dx * ops.dropout_apply(torch.ones(z.shape, device="cuda"), f["drop_p"], f["drop_seed"]).double().cpu()
    return dx, a * dyr.t() @ xr, a * dy_stored.sum(0)


def _assert_linear_bwd(ops, prec, x, w, dy, z, f, got, want16):
    """dx (fp32) to TOL, dw and db (atomics) to TOL_ATOMIC, under every precision mode; a 16-bit dx is, bit for bit, the fp32 dx
    of the same call with dx16=False cast to the type ("identical results"), and that fp32 dx is held to TOL."""
    dx, dw, db = got
    rdx, rdw, rdb = _linear_bwd_ref(ops, prec, x, w, dy, z, f)
    if f["need_dx"]:
        assert dx.dtype == (DT16[prec] if want16 else torch.float32), (dx.dtype, f)
        assert dx.shape == x.shape
        if want16:
            dx32 = _run_linear_bwd(ops, prec, x, w, dy, z, dict(f, dx16=False))[0]
            assert dx32.dtype == torch.float32
            assert torch.equal(dx, dx32.to(DT16[prec])), ("dx16 is not the fp32 dx rounded", f)
            dx = dx32
        e = rel_l2(dx, rdx)
        assert e < TOL, ("dx", e, f)
    else:
        assert dx is None
    assert dw.dtype == torch.float32 and db.dtype == torch.float32
    ew, eb = rel_l2(dw, rdw), rel_l2(db, rdb)
    assert ew < TOL_ATOMIC, ("dw", ew, f)
    assert eb < TOL_ATOMIC, ("db", eb, f)


def _check_linear_bwd(ops, M, N, K, prec, data):
    x, w, dy, z, f = _linear_bwd_case(ops, M, N, K, prec, data)
    got = _run_linear_bwd(ops, prec, x, w, dy, z, f)
    # dx16 is honoured exactly where the 16-bit consumer can take it (the swish' routes with n, k % 8 == 0)
    want16 = bool(prec and f["dx16"] and z is not None and N % 8 == 0 and K % 8 == 0)
    _assert_linear_bwd(ops, prec, x, w, dy, z, f, got, want16)


@settings(max_examples=30, **SET)
@given(M=st.integers(1, 1100), N=st.integers(1, 300), K4=st.integers(1, 80), data=st.data())
def test_linear_bwd_fp32_any_shape(ops, M, N, K4, data):
    """fp32 routes: ragged M / N / K (N % 4 != 0: the padded dY copy), alpha, swish' (contiguous and strided Z), dropout,
    need_dx=False."""
    _check_linear_bwd(ops, M, N, 4 * K4, 0, data)


@settings(max_examples=30, **SET)
@given(M=st.integers(1, 1100), N8=st.integers(1, 40), ragged_n=st.booleans(), K4=st.integers(1, 80),
       prec=st.sampled_from([1, 2]), data=st.data())
def test_linear_bwd_16bit_routes(ops, M, N8, ragged_n, K4, prec, data):
    """16-bit modes with random combinations of the route flags (16-bit x / dY / dx16, alpha, Z, dropout, ragged n and k);
    every route is pinned on its own by test_linear_bwd_16bit_route_pinned."""
    N = 8 * N8 - (data.draw(st.integers(1, 7)) if ragged_n else 0)
    _check_linear_bwd(ops, M, N, 4 * K4, prec, data)


_GEMM16, _GEMM16_BWD, _DW16 = "cfm_gemm_mfma16_f32", "cfm_gemm_bwd_batched_mfma16_f32", "cfm_linear_bwd_weight_mfma16_f32"
# route -> (flags, K % 8 == 4, ragged n, entry points that must run, entry points that must not run, dx in the 16-bit type)
LINEAR16_ROUTES = {
    # dX = dY.W on the forward kernel (16-bit dY, no Z, alpha = 1) + the fused weight gradient reading the 16-bit dY
    "dy16_dx_forward_kernel": (dict(dy16=True), False, False, {_GEMM16, _DW16}, {_GEMM16_BWD}, False),
    # swish' epilogue on the forward kernel (z_ok), fp32 dY, dropout; dW on the general kernel
    "z_ok": (dict(use_z="contig", alpha=-1.75, drop_p=0.2), False, False, {_GEMM16, _GEMM16_BWD}, {_DW16}, False),
    "z_ok_dx16": (dict(use_z="contig", dx16=True, alpha=0.5), False, False, {_GEMM16, _GEMM16_BWD}, {_DW16}, True),
    "z_ok_dy16_dx16": (dict(use_z="contig", dy16=True, dx16=True, drop_p=0.2), False, False, {_GEMM16, _DW16}, {_GEMM16_BWD}, True),
    # the fused weight-gradient kernel with a 16-bit dY only, a 16-bit x only, and both
    "fused_dw_dy16": (dict(dy16=True, need_dx=False), False, False, {_DW16}, {_GEMM16, _GEMM16_BWD}, None),
    "fused_dw_x16": (dict(x16=True, need_dx=False), False, False, {_DW16}, {_GEMM16, _GEMM16_BWD}, None),
    "fused_dw_x16_dy16": (dict(x16=True, dy16=True, alpha=1.0), False, False, {_GEMM16, _DW16}, {_GEMM16_BWD}, False),
    # Z whose row stride is not a multiple of 8: the general kernel writes the 16-bit dx (c16)
    "c16": (dict(use_z="strided", dx16=True, drop_p=0.2), False, False, {_GEMM16_BWD}, {_GEMM16, _DW16}, True),
    # 16-bit dY at k % 8 == 4: widened, general kernels only
    "widened_dy16": (dict(dy16=True, use_z="contig", dx16=True), True, False, {_GEMM16_BWD}, {_GEMM16, _DW16}, False),
    # ragged n: Z is not z_ok, dx16 is not honoured
    "general_ragged_n": (dict(use_z="contig", dx16=True, alpha=0.5), False, True, {_GEMM16_BWD}, {_GEMM16, _DW16}, False),
}


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("route", list(LINEAR16_ROUTES))
@settings(max_examples=6, **SET)
@given(M=st.integers(1, 1100), n8=st.integers(1, 40), k8=st.integers(1, 40), r=st.integers(1, 7), seed=st.integers(0, 10 ** 6))
def test_linear_bwd_16bit_route_pinned(ops, route, prec, M, n8, k8, r, seed):
    """Each 16-bit route of linear_bwd under bf16 and fp16, at drawn ragged M and aligned (or, where the route needs it,
    ragged) N / K: the library entry points that ran are asserted, and so is the dtype of dx."""
    flags, k_off, n_off, must, must_not, want16 = LINEAR16_ROUTES[route]
    N, K = 8 * n8 - (r if n_off else 0), 8 * k8 - (4 if k_off else 0)
    f = dict(alpha=1.0, need_dx=True, drop_p=0.0, x16=False, dy16=False, dx16=False, use_z=None, drop_seed=seed * 7 + 1)
    f.update(flags)
    x, w, dy = rnd(M, K, seed=seed), rnd(N, K, seed=seed + 1) / math.sqrt(K), rnd(M, N, seed=seed + 2)
    z = None if f["use_z"] is None else rnd(M, K + (4 if f["use_z"] == "strided" else 0), seed=seed + 3)
    with _Calls(_GEMM16, _GEMM16_BWD, _DW16) as seen:
        got = _run_linear_bwd(ops, prec, x, w, dy, z, f)
    assert must <= seen and not (must_not & seen), (route, sorted(seen))
    _assert_linear_bwd(ops, prec, x, w, dy, z, f, got, bool(want16))


@pytest.mark.parametrize("M,N,K,prec", [(1, 8, 4, 1), (37, 16, 12, 2), (300, 40, 36, 1)])
def test_linear_bwd_16bit_x_with_k_off_8(ops, M, N, K, prec):
    """A 16-bit x whose rows are not 8-element aligned (K % 8 == 4) is widened for the general weight-gradient kernel
    (found by the sweep above at M = 1, N = 8, K = 4: the kernel refused the 16-bit B operand)."""
    x, w, dy = rnd(M, K, seed=M), rnd(N, K, seed=N) / math.sqrt(K), rnd(M, N, seed=K)
    f = dict(alpha=1.0, need_dx=True, drop_p=0.0, x16=True, dy16=False, dx16=False, use_z=None, drop_seed=0)
    _assert_linear_bwd(ops, prec, x, w, dy, None, f, _run_linear_bwd(ops, prec, x, w, dy, None, f), False)


def test_linear_bwd_refuses_mismatched_16bit_x(ops):
    x = torch.randn(8, 16, device="cuda").to(torch.float16)
    with ops.precision(ops.PREC_BF16):
        with pytest.raises(ops._lib.ConformerHipError):
            ops.linear_bwd(x, torch.randn(16, 16, device="cuda"), torch.randn(8, 16, device="cuda"))
    with pytest.raises(ops._lib.ConformerHipError):
        ops.linear_bwd(x, torch.randn(16, 16, device="cuda"), torch.randn(8, 16, device="cuda"))


def test_linear_bwd_refuses_mismatched_16bit_dy(ops):
    dy = torch.randn(8, 16, device="cuda").to(torch.float16)
    with ops.precision(ops.PREC_BF16):
        with pytest.raises(ops._lib.ConformerHipError):
            ops.linear_bwd(torch.randn(8, 16, device="cuda"), torch.randn(16, 16, device="cuda"), dy)
    with pytest.raises(ops._lib.ConformerHipError):
        ops.linear_bwd(torch.randn(8, 16, device="cuda"), torch.randn(16, 16, device="cuda"), dy)


def test_linear_bwd_tolerance_discriminates(ops):
    """A dropout mask drawn with the wrong seed gives a dx far outside the bound."""
    M, N, K, p = 64, 48, 40, 0.2
    dy, w, z = rnd(M, N, seed=1), rnd(N, K, seed=2) / math.sqrt(K), rnd(M, K, seed=3)
    base = (dy.double() @ w.double()) * dswish(z.double())
    m1 = ops.dropout_apply(torch.ones(M, K, device="cuda"), p, 11).double().cpu()
    m2 = ops.dropout_apply(torch.ones(M, K, device="cuda"), p, 12).double().cpu()
    assert rel_l2(base * m2, base * m1) > 10 * TOL16[1]


# ---- 3. depthwise conv + BatchNorm (train / eval) + Swish -----------------------------------------------------------------
def _dwconv_ref(g, w, b, bw, bb, rm, rv, dy, train):
    """float64 autograd: returns (grads of g, w, b, bw, bb), dc (the conv-output gradient), batch mean, biased var."""
    gd, wd, bd, bwd, bbd = leaf(g), leaf(w), leaf(b), leaf(bw), leaf(bb)
    K = w.shape[-1]
    C = g.shape[-1]
    c = F.conv1d(gd.transpose(1, 2), wd, bd, padding=K // 2, groups=C)                     # (B,C,T)
    c.retain_grad()
    if train:
        mean = c.mean((0, 2))
        var = ((c - mean[None, :, None]) ** 2).mean((0, 2))
    else:
        mean, var = rm.double(), rv.double()
    bn = (c - mean[None, :, None]) / torch.sqrt(var[None, :, None] + 1e-5) * bwd[:, None] + bbd[:, None]
    (O.swish(bn) * dy.double().transpose(1, 2)).sum().backward()
    return (gd.grad, wd.grad, bd.grad, bwd.grad, bbd.grad), c.grad, mean.detach(), var.detach()


@settings(max_examples=25, **SET)
@given(B=st.integers(1, 6), T=st.integers(1, 700), C=st.integers(1, 600), K=st.sampled_from([3, 7, 15, 31]),
       train=st.booleans(), seed=st.integers(0, 10 ** 6))
@example(B=1, T=2, C=70, K=31, train=True, seed=3).via("B*T < 3: statistics only")
@example(B=2, T=64, C=64, K=3, train=True, seed=4).via("one statistics segment, whole channel block")
def test_dwconv_bn_swish_train_any_geometry(ops, B, T, C, K, train, seed):
    """T below K, one segment, crossing the 32-frame (backward) and 64-frame (statistics) segment roundings; C in ragged
    64-channel blocks; train-mode statistics + running update, or fixed (eval) statistics; every gradient."""
    T = max(1, min(T, 400_000 // (B * C)))            # (CPU float64 autograd budget)
    g, w, b = rnd(B, T, C, seed=seed), rnd(C, 1, K, seed=seed + 1) / 3, rnd(C, seed=seed + 2) * 0.3
    bw, bb = rnd(C, seed=seed + 3) * 0.2 + 1, rnd(C, seed=seed + 4) * 0.1
    rm, rv = rnd(C, seed=seed + 5) * 0.1, rnd(C, seed=seed + 6).abs() + 0.5
    dy = rnd(B, T, C, seed=seed + 7)
    G = [t.cuda() for t in (g, w, b, bw, bb)]
    n = B * T
    grads, dc, mean_r, var_r = _dwconv_ref(g, w, b, bw, bb, rm, rv, dy, train)
    if train:
        rmg, rvg = rm.cuda(), rv.cuda()
        mean, var = ops.dwconv_bn_batch_stats(G[0], G[1], G[2], rmg, rvg, 0.1)
        assert rel_l2(mean, mean_r) < TOL and rel_l2(var, var_r) < TOL
        assert rel_l2(rmg, 0.9 * rm.double() + 0.1 * mean_r) < TOL
        assert rel_l2(rvg, 0.9 * rv.double() + 0.1 * var_r * n / max(n - 1, 1)) < TOL
        if n < 3:       # rstd ~ 1/sqrt(eps) amplifies fp32 noise in the coupled gradient (test_backward_gpu.py, modules_d32_t1)
            return
    else:
        mean, var = rm.cuda(), rv.cuda()
    out = ops.dwconv_bn_swish_bwd(G[0], dy.cuda(), G[1], G[2], G[3], G[4], mean, var, train_stats=train)
    for name, got, ref in zip(("dg", "dw", "db", "dgamma", "dbeta"), out, grads):
        if name == "db" and train:
            # sum_t dc = 0 exactly under batch statistics: the bias gradient is rounding noise, bounded on dc's scale
            assert float((got.cpu().double() - ref).norm()) < TOL_ATOMIC * float(dc.norm()), name
        else:
            assert rel_l2(got, ref) < TOL_ATOMIC, (name, B, T, C, K, train)


def test_dwconv_bn_train_tolerance_discriminates():
    """With train statistics in force, the gradient that treats them as constants (the eval formula) is far outside the bound."""
    B, T, C, K = 2, 40, 24, 7
    g, w, b = rnd(B, T, C, seed=1), rnd(C, 1, K, seed=2) / 3, rnd(C, seed=3) * 0.3
    bw, bb, dy = rnd(C, seed=4) * 0.2 + 1, rnd(C, seed=5) * 0.1, rnd(B, T, C, seed=6)
    tr, _, mean, var = _dwconv_ref(g, w, b, bw, bb, None, None, dy, True)
    ev, _, _, _ = _dwconv_ref(g, w, b, bw, bb, mean.float(), var.float(), dy, False)
    assert rel_l2(ev[0], tr[0]) > 100 * TOL_ATOMIC        # dg
    assert rel_l2(ev[1], tr[1]) > 100 * TOL_ATOMIC        # dw


# ---- 4. conv-subsampling stem backward ------------------------------------------------------------------------------------
class _Round16(torch.autograd.Function):
    """Rounds the forward value (fwd=True) and / or the incoming gradient (bwd=True) to a 16-bit type: the points where the
    16-bit stem stores a tensor in that type (h1; dz2 = relu'(h2) * dh2; dh1)."""

    @staticmethod
    def forward(ctx, t, dt, fwd, bwd):
        ctx.dt, ctx.bwd = dt, bwd
        return t.to(dt).double() if fwd else t.clone()

    @staticmethod
    def backward(ctx, g):
        return (g.to(ctx.dt).double() if ctx.bwd else g), None, None, None


def _stem_ref(x, w1, b1, w2, b2, dh2, prec):
    """float64 autograd through the lines of oracle.conv_subsampling; under a 16-bit mode the conv2 weight and the stored
    tensors (h1, dz2, dh1) are rounded where the kernels store them.  dh2 is channel-last (B, T2, F2*C) like the kernel's h2."""
    ps = [leaf(w1), leaf(b1), leaf(w2), leaf(b2)]
    pre = "s."
    if not prec:
        P = dict(zip([pre + "conv_1.weight", pre + "conv_1.bias", pre + "conv_2.weight", pre + "conv_2.bias"], ps))
        y = O.conv_subsampling(x.double(), P, pre)                        # (B, T2, C*F2), feature c*F2 + f
    else:
        dt = DT16[prec]
        h1 = F.relu(F.conv2d(x.double()[:, None], ps[0], ps[1], stride=2))
        h1 = _Round16.apply(h1, dt, True, True)                           # h1 stored 16-bit; dh1 written 16-bit
        z2 = F.conv2d(h1, _Round16.apply(ps[2], dt, True, False), ps[3], stride=2)
        h2 = F.relu(_Round16.apply(z2, dt, False, True))                  # dz2 written 16-bit
        Bn, C, Fp, Tp = h2.shape
        y = h2.permute(0, 3, 1, 2).reshape(Bn, Tp, C * Fp)
    B, T2, CF = y.shape
    C = w1.shape[0]
    y = y.view(B, T2, C, CF // C).transpose(2, 3).reshape(B, T2, CF)    # -> [f][c]
    (y * dh2.double()).sum().backward()
    return y.detach(), [p.grad for p in ps]


def _check_stem(ops, B, Fm, T, C, prec, seed):
    x = rnd(B, Fm, T, seed=seed)
    w1, b1 = rnd(C, 1, 3, 3, seed=seed + 1) / 3, rnd(C, seed=seed + 2) * 0.1
    w2, b2 = rnd(C, C, 3, 3, seed=seed + 3) / math.sqrt(9 * C), rnd(C, seed=seed + 4) * 0.1
    F2, T2 = ((Fm - 1) // 2 - 1) // 2, ((T - 1) // 2 - 1) // 2
    dh2 = rnd(B, T2, F2 * C, seed=seed + 5)
    X, W1, B1, W2, B2 = (t.cuda() for t in (x, w1, b1, w2, b2))
    with ops.precision(prec):
        h2, h1 = ops.subsample_stem_train(X, W1, B1, ops.pack_conv2_weight(W2), B2)
        out = ops.subsample_stem_bwd(X, W1, B1, W2, h1, h2, dh2.cuda())
    assert h1.dtype == (DT16[prec] if prec else torch.float32)          # the 16-bit class-gather path really ran
    y, grads = _stem_ref(x, w1, b1, w2, b2, dh2, prec)
    tol = TOL16[prec] if prec else TOL_ATOMIC
    assert rel_l2(h2, y) < (tol if prec else TOL)
    assert [got.shape for got in out] == [ref.shape for ref in grads]
    errs = {name: rel_l2(got, ref) for name, got, ref in zip(("dw1", "db1", "dw2", "db2"), out, grads)}
    assert max(errs.values()) < tol, (errs, B, Fm, T, C, prec)


def _stem_budget(B, Fm, T, C):
    F2 = ((Fm - 1) // 2 - 1) // 2
    return max(7, min(T, 4 * (2_000_000 // (B * F2 * C * C)) + 6))          # (CPU float64 conv budget)


@settings(max_examples=15, **SET)
@given(B=st.integers(1, 3), Fm=st.integers(7, 300), T=st.integers(7, 300), c16=st.integers(1, 15).filter(lambda c: c % 4),
       seed=st.integers(0, 10 ** 6))
@example(B=1, Fm=7, T=7, c16=1, seed=1).via("F2 = T2 = 1")
def test_stem_bwd_fp32_any_shape(ops, B, Fm, T, c16, seed):
    """fp32 stem backward: F and T odd and even from 7 (T2 = 1) up, C % 64 != 0 (the training conv2 takes C % 16 == 0)."""
    C = 16 * c16
    _check_stem(ops, B, Fm, _stem_budget(B, Fm, T, C), C, 0, seed)


def test_stem_train_refuses_channels_off_16(ops):
    x, w1, b1 = torch.randn(1, 20, 20, device="cuda"), torch.randn(12, 1, 3, 3, device="cuda"), torch.randn(12, device="cuda")
    w2, b2 = torch.randn(12, 12, 3, 3, device="cuda"), torch.randn(12, device="cuda")
    with pytest.raises(ops._lib.ConformerHipError):
        ops.subsample_stem_train(x, w1, b1, ops.pack_conv2_weight(w2), b2)


@settings(max_examples=12, **SET)
@given(B=st.integers(1, 3), Fm=st.integers(7, 300), T=st.integers(7, 300), C=st.sampled_from([64, 128, 256]),
       prec=st.sampled_from([1, 2]), seed=st.integers(0, 10 ** 6))
@example(B=1, Fm=7, T=7, C=64, prec=1, seed=0).via("F2 = T2 = 1 under bf16")
def test_stem_bwd_16bit_any_shape(ops, B, Fm, T, C, prec, seed):
    """16-bit class-gather stem backward (16-bit h1, dz2, dh1) under bf16 and fp16.
    (h2 and dh1 themselves, per window and on every block tile, against float64 at 2e-5: tests/test_property_stem16_gpu.py.)"""
    _check_stem(ops, B, Fm, _stem_budget(B, Fm, T, C), C, prec, seed)


def test_stem_bwd_tolerance_discriminates():
    """dw2 with its two spatial taps swapped (a transposed kernel walk) is far outside the bound."""
    B, Fm, T, C = 1, 23, 19, 8
    x, w1, b1 = rnd(B, Fm, T, seed=1), rnd(C, 1, 3, 3, seed=2) / 3, rnd(C, seed=3) * 0.1
    w2, b2 = rnd(C, C, 3, 3, seed=4) / math.sqrt(9 * C), rnd(C, seed=5) * 0.1
    F2, T2 = ((Fm - 1) // 2 - 1) // 2, ((T - 1) // 2 - 1) // 2
    dh2 = rnd(B, T2, F2 * C, seed=6)
    _, g = _stem_ref(x, w1, b1, w2, b2, dh2, 0)
    assert rel_l2(g[2].transpose(2, 3), g[2]) > 10 * TOL16[1]
    _, g16 = _stem_ref(x, w1, b1, w2, b2, dh2, 1)          # the rounded reference is itself within the bf16 bound
    assert all(rel_l2(a, b) < TOL16[1] for a, b in zip(g16, g))


# ---- 5. LSTM BPTT: row-major (H % 16 != 0), fragment fp32 (H % 16 == 0), 16-bit (bf16 and fp16) ---------------------------
LSTM_BWD = {"row": "cfm_lstm_bwd_f32", "frag": "cfm_lstm_bwd_frag_f32", "bf16": "cfm_lstm_bwd_mfma16_f32", "fp16": "cfm_lstm_bwd_mfma16_f32"}


@settings(max_examples=30, **SET)
@given(B=st.integers(1, 80), T=st.integers(1, 40), d4=st.integers(1, 16), kind=st.sampled_from(["row", "frag", "bf16", "fp16"]),
       hk=st.integers(1, 24), seed=st.integers(0, 10 ** 6))
@example(B=40, T=12, d4=3, kind="row", hk=9, seed=1).via("row-major BPTT: recurrence over two 32-utterance tiles")
@example(B=70, T=25, d4=5, kind="row", hk=5, seed=2).via("row-major BPTT: three tiles, H = 20")
@example(B=33, T=9, d4=4, kind="frag", hk=2, seed=3).via("fragment BPTT: one utterance past two 16-utterance tiles")
@example(B=33, T=17, d4=4, kind="bf16", hk=3, seed=4).via("16-bit BPTT under bf16 past one 32-utterance tile")
@example(B=48, T=20, d4=2, kind="fp16", hk=2, seed=5).via("16-bit BPTT under fp16, three 16-utterance tiles")
def test_lstm_bptt_any_geometry(ops, B, T, d4, kind, hk, seed):
    """B across the 16- and 32-utterance tiles, ragged descending lengths with 1 and repeats; every gradient against
    autograd through oracle.lstm_layer, y exactly zero beyond each length; the BPTT kernel that ran is asserted.  The 1e-2
    free-run bound of the 16-bit kinds is the end-to-end check; the kernels are held per element, one step at a time, in
    test_lstm_step_gpu.py."""
    from conformer_amd.autograd import LstmFn
    H = 4 * (hk + (hk % 4 == 0)) if kind == "row" else 16 * ((hk - 1) % 6 + 1)        # row: H % 16 != 0
    prec = {"row": 0, "frag": 0, "bf16": 1, "fp16": 2}[kind]
    lens = sorted(torch.randint(1, T + 1, (B,), generator=torch.Generator().manual_seed(seed + 11)).tolist(), reverse=True)
    lens[-1] = 1
    if B > 2:
        lens[1] = lens[0]
    D = 4 * d4
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, D, generator=g)
    k = 1.0 / H ** 0.5
    ps = [(torch.rand(4 * H, D, generator=g) * 2 - 1) * k, (torch.rand(4 * H, H, generator=g) * 2 - 1) * k,
          (torch.rand(4 * H, generator=g) * 2 - 1) * k, (torch.rand(4 * H, generator=g) * 2 - 1) * k]
    w = torch.randn(B, T, H, generator=g)
    L = torch.tensor(lens, dtype=torch.int64)
    xr = leaf(r16(x, prec))
    pr = [leaf(r16(p, prec)) if i < 2 else leaf(p) for i, p in enumerate(ps)]
    ref = O.lstm_layer(xr, L, *pr)
    (ref * w.double()).sum().backward()
    xd = x.cuda().requires_grad_(True)
    pd = [p.cuda().requires_grad_(True) for p in ps]
    with _Calls(*sorted(set(LSTM_BWD.values()))) as seen:
        if prec:
            with torch.autocast("cuda", dtype=DT16[prec]):
                y = LstmFn.apply(xd, *pd, L.cuda())
        else:
            y = LstmFn.apply(xd, *pd, L.cuda())
        (y.float() * w.cuda()).sum().backward()
    assert seen == {LSTM_BWD[kind]}, (kind, H, seen)
    tol = TOL16[prec] if prec else TOL
    assert y.dtype == torch.float32 and rel_l2(y, ref.detach()) < tol
    for b in range(B):
        assert not y[b, lens[b]:].any(), b
    assert rel_l2(xd.grad, xr.grad) < tol
    for a, r, name in zip(pd, pr, ("w_ih", "w_hh", "b_ih", "b_hh")):
        assert rel_l2(a.grad, r.grad) < tol, (name, B, T, H, kind)


def test_lstm_bptt_tolerance_discriminates():
    """Treating every utterance as full length (ignoring the packed lengths) moves the gradients far outside the bound."""
    B, T, D, H = 4, 9, 8, 8
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, D, generator=g)
    ps = [(torch.rand(4 * H, s, generator=g) * 2 - 1) / H ** 0.5 for s in (D, H)] + \
         [(torch.rand(4 * H, generator=g) * 2 - 1) / H ** 0.5 for _ in range(2)]
    w = torch.randn(B, T, H, generator=g)
    out = []
    for L in (torch.tensor([9, 9, 5, 1]), None):
        pr = [leaf(p) for p in ps]
        (O.lstm_layer(x.double(), L, *pr) * w.double()).sum().backward()
        out.append(pr[1].grad)
    assert rel_l2(out[1], out[0]) > 10 * TOL16[1]


# ---- 6. CTC loss: any blank, every waves-per-workgroup choice of the gradient kernel, the feasibility bound ------------------
def _ctc_need(lab):
    return len(lab) + sum(1 for i in range(1, len(lab)) if lab[i] == lab[i - 1])


def _ctc_draw(data, B, V, blank, Lmax):
    """Targets from the non-blank ids with adjacent repeats; input lengths at the feasibility bound, one frame below it,
    or above it."""
    labs, il = [], []
    for _ in range(B):
        L = data.draw(st.integers(1, Lmax))
        ids = data.draw(st.lists(st.integers(0, V - 2), min_size=L, max_size=L))
        lab = [i + (i >= blank) for i in ids]
        for i in range(1, L):                                              # some adjacent repeats
            if data.draw(st.integers(0, 4)) == 0:
                lab[i] = lab[i - 1]
        labs.append(lab)
        il.append((_ctc_need(lab), data.draw(st.sampled_from(["at", "below", "above"]))))
    T = max(n for n, _ in il) + data.draw(st.integers(0, 6))
    in_len = [n if m == "at" else (n - 1 if m == "below" else data.draw(st.integers(n, T))) for n, m in il]
    return labs, in_len, T


def _ctc_check(ops, labs, in_len, T, V, blank, grad_out, seed):
    B = len(labs)
    tl = [len(l) for l in labs]
    tg = torch.zeros(B, max(tl), dtype=torch.int64)
    for b, l in enumerate(labs):
        tg[b, :len(l)] = torch.tensor(l)
    x = rnd(B, T, V, seed=seed) * 2
    loss_o, nll_o, grad_o = O.ctc_lattice(x, tg, torch.tensor(in_len), torch.tensor(tl), blank=blank)
    loss, ctx = ops.ctc_loss_forward(x.cuda(), tg.cuda(), torch.tensor(in_len).cuda(), torch.tensor(tl).cuda(), blank=blank)
    assert abs(float(loss) - loss_o) <= 1e-5 * max(1.0, abs(loss_o))
    nll = ops.ctc_nll(ctx).cpu().double()
    fin = torch.isfinite(nll_o)
    assert torch.equal(torch.isfinite(nll), fin)
    if fin.any():
        assert rel_l2(nll[fin], nll_o[fin]) < 1e-5
    dl = ops.ctc_loss_backward(ctx, torch.tensor(grad_out, device="cuda")).cpu()
    assert torch.isfinite(dl).all()
    want = grad_out * grad_o
    assert rel_l2(dl, want) < 1e-4 if float(want.norm()) > 0 else not dl.any()
    for b in range(B):
        assert not dl[b, in_len[b]:].any(), b                  # frames beyond the length: exact zeros
        if not fin[b]:
            assert not dl[b].any(), b                          # infeasible utterance: zeroed term, exact zero gradient
    return ctx


# V on both sides of the 4 -> 2 -> 1 waves-per-workgroup boundaries of cfm_ctc_loss_bwd_f32 (per-wave LDS (V + 128 P) * 4 bytes)
CTC_V_P1 = [3968, 3969, 8064, 8065, 16256]          # P = 1 (longest target <= 63)
CTC_V_P2 = [3840, 3841, 7936, 7937, 16128]          # P = 2 (64 .. 127)


@settings(max_examples=20, **SET)
@given(B=st.integers(1, 3), long=st.booleans(), data=st.data())
def test_ctc_loss_any_blank_and_vocabulary(ops, B, long, data):
    """Random blank, vocabulary, targets and lengths; the wave-count bounds themselves are pinned by
    test_ctc_loss_wave_boundaries."""
    V = data.draw(st.one_of(st.sampled_from(CTC_V_P2 if long else CTC_V_P1), st.integers(2, 400)))
    blank = data.draw(st.sampled_from([0, V - 1, V // 2]))
    Lmax = 100 if long else 20
    labs, in_len, T = _ctc_draw(data, B, V, blank, Lmax)
    if long:
        labs[0] = (labs[0] * (64 // len(labs[0]) + 1))[:64 + data.draw(st.integers(0, 36))]    # P = 2
        in_len[0] = _ctc_need(labs[0])
        T = max(T, in_len[0])
    grad_out = data.draw(st.sampled_from([1.0, 0.37, -2.5]))
    _ctc_check(ops, labs, in_len, T, V, blank, grad_out, data.draw(st.integers(0, 10 ** 6)))


@pytest.mark.parametrize("V,long", [(v, False) for v in CTC_V_P1] + [(v, True) for v in CTC_V_P2])
def test_ctc_loss_wave_boundaries(ops, V, long):
    """Both sides of every waves-per-workgroup bound (4 -> 2 -> 1) at P = 1 and P = 2, pinned; blank rotates over 0, V-1
    and a middle id; one utterance at the feasibility bound, one a frame below it (zeroed), one above it."""
    g = torch.Generator().manual_seed(V)
    blank = [0, V - 1, V // 2][V % 3]
    labs = []
    for L in ((64 + V % 37, 20, 9) if long else (20, 13, 5)):
        lab = (torch.randint(0, V - 1, (L,), generator=g) + 0).tolist()
        lab = [i + (i >= blank) for i in lab]
        for i in range(2, L, 5):                                           # adjacent repeats
            lab[i] = lab[i - 1]
        labs.append(lab)
    need = [_ctc_need(l) for l in labs]
    in_len = [need[0], need[1] - 1, need[2] + 3]
    _ctc_check(ops, labs, in_len, max(in_len), V, blank, 0.37, V + 1)


def test_ctc_loss_criterion_passes_blank_through(ops):
    """ConformerCriterion(blank_id=V-1) reaches the kernels: loss and gradient match the lattice with that blank."""
    from conformer_amd.evaluation import ConformerCriterion
    B, T, V = 2, 12, 9
    tg = torch.tensor([[1, 2, 2, 3], [0, 7, 0, 0]])
    il, tl = torch.tensor([12, 9]), torch.tensor([4, 3])
    x = rnd(B, T, V, seed=5)
    loss_o, _, grad_o = O.ctc_lattice(x, tg, il, tl, blank=V - 1)
    xd = x.cuda().requires_grad_()
    loss = ConformerCriterion(blank_id=V - 1).ctc_loss(xd, tg.cuda(), il.cuda(), tl.cuda())
    loss.backward()
    assert abs(float(loss) - loss_o) <= 1e-5 * abs(loss_o)
    assert rel_l2(xd.grad, grad_o) < 1e-4


@pytest.mark.parametrize("V,Lmax", [(16257, 20), (16129, 80)])
def test_ctc_loss_bwd_refuses_rows_beyond_lds(ops, V, Lmax):
    """Above the one-wave LDS bound the forward still runs (it does not stage the row) and the backward raises."""
    from conformer_amd import _lib
    B, T = 1, Lmax + 3
    tg = (torch.arange(Lmax) % (V - 1) + 1)[None]
    x = rnd(B, T, V, seed=1)
    loss_o, _, _ = O.ctc_lattice(x, tg, [T], [Lmax])
    loss, ctx = ops.ctc_loss_forward(x.cuda(), tg.cuda(), torch.tensor([T]).cuda(), torch.tensor([Lmax]).cuda())
    assert abs(float(loss) - loss_o) <= 1e-5 * abs(loss_o)
    with pytest.raises(_lib.ConformerHipError):
        ops.ctc_loss_backward(ctx, torch.tensor(1.0, device="cuda"))


def test_ctc_tolerance_discriminates():
    """The gradient computed with the wrong blank id is far outside the bound."""
    B, T, V = 2, 10, 7
    tg = torch.tensor([[1, 2, 3], [2, 2, 4]])
    x, il, tl = rnd(B, T, V, seed=2), torch.tensor([10, 8]), torch.tensor([3, 3])
    _, _, g0 = O.ctc_lattice(x, tg, il, tl, blank=6)
    _, _, g1 = O.ctc_lattice(x, tg, il, tl, blank=0)
    assert rel_l2(g1, g0) > 100 * 1e-4


# ---- 7. small elementwise pieces: decoder Swish + BatchNorm, GLU, colsum --------------------------------------------------------
def _swish_bn_ref(h, rm, rv, bw, bb, dz, train):
    hd, bwd, bbd = leaf(h), leaf(bw), leaf(bb)
    s = O.swish(hd)
    if train:
        mean, var = s.mean(0), s.var(0, unbiased=False)
    else:
        mean, var = rm.double(), rv.double()
    z = (s - mean) / torch.sqrt(var + 1e-5) * bwd + bbd
    (z * dz.double()).sum().backward()
    return z.detach(), (hd.grad, bwd.grad, bbd.grad), mean.detach(), var.detach()


@settings(max_examples=25, **SET)
@given(rows=st.integers(1, 3000), c4=st.integers(1, 200), train=st.booleans(), seed=st.integers(0, 10 ** 6))
def test_swish_bn_any_shape(ops, rows, c4, train, seed):
    C = 4 * c4
    h, dz = rnd(rows, C, seed=seed) * 1.5, rnd(rows, C, seed=seed + 1)
    bw, bb = rnd(C, seed=seed + 2) * 0.2 + 1, rnd(C, seed=seed + 3) * 0.1
    rm, rv = rnd(C, seed=seed + 4) * 0.1, rnd(C, seed=seed + 5).abs() + 0.5
    z_r, grads, mean_r, var_r = _swish_bn_ref(h, rm, rv, bw, bb, dz, train)
    H = h.cuda()
    if train:
        rmg, rvg = rm.cuda(), rv.cuda()
        mean, var = ops.swish_bn_batch_stats(H, rmg, rvg, 0.1)
        assert rel_l2(mean, mean_r) < TOL and rel_l2(var, var_r) < TOL
        assert rel_l2(rmg, 0.9 * rm.double() + 0.1 * mean_r) < TOL
        assert rel_l2(rvg, 0.9 * rv.double() + 0.1 * var_r * rows / max(rows - 1, 1)) < TOL
        if rows < 3:
            return
    else:
        mean, var = rm.cuda(), rv.cuda()
    assert rel_l2(ops.swish_bn_eval(H, mean, var, bw.cuda(), bb.cuda()), z_r) < TOL
    out = ops.swish_bn_bwd(H, dz.cuda(), mean, var, bw.cuda(), train_stats=train)
    for name, got, ref in zip(("dh", "dgamma", "dbeta"), out, grads):
        assert rel_l2(got, ref) < TOL_ATOMIC, (name, rows, C, train)


def test_swish_bn_tolerance_discriminates():
    """With batch statistics in force, the eval-statistics gradient is far outside the bound."""
    rows, C = 50, 12
    h, dz, bw, bb = rnd(rows, C, seed=1) * 1.5, rnd(rows, C, seed=2), rnd(C, seed=3) * 0.2 + 1, rnd(C, seed=4) * 0.1
    _, tr, mean, var = _swish_bn_ref(h, None, None, bw, bb, dz, True)
    _, ev, _, _ = _swish_bn_ref(h, mean.float(), var.float(), bw, bb, dz, False)
    assert rel_l2(ev[0], tr[0]) > 100 * TOL_ATOMIC


@settings(max_examples=25, **SET)
@given(rows=st.integers(1, 3000), n4=st.integers(1, 150), prec=st.sampled_from([0, 1, 2]), seed=st.integers(0, 10 ** 6))
@example(rows=37, n4=6, prec=1, seed=1).via("16-bit dz under bf16 (n % 8 == 0)")
@example(rows=300, n4=36, prec=2, seed=2).via("16-bit dz under fp16 (n % 8 == 0)")
@example(rows=65, n4=5, prec=1, seed=3).via("bf16 mode, n % 8 == 4: fp32 dz")
def test_glu_fwd_bwd_any_shape(ops, rows, n4, prec, seed):
    """GLU forward / backward for ragged rows; under a 16-bit mode with n % 8 == 0 the for_gemm gradient is written in that type."""
    n = 4 * n4
    z, dy = rnd(rows, 2 * n, seed=seed), rnd(rows, n, seed=seed + 1)
    zd = leaf(z)
    y_r = zd[:, :n] * torch.sigmoid(zd[:, n:])
    (y_r * dy.double()).sum().backward()
    Z, DY = z.cuda(), dy.cuda()
    assert rel_l2(ops.glu_fwd(Z), y_r.detach()) < TOL
    with ops.precision(prec):
        dz = ops.glu_bwd(Z, DY, for_gemm=True)
    want16 = bool(prec and n % 8 == 0)
    assert dz.dtype == (DT16[prec] if want16 else torch.float32)
    assert rel_l2(dz, zd.grad) < (TOL16[prec] if want16 else TOL)
    assert rel_l2(ops.glu_bwd(Z, DY), zd.grad) < TOL


@settings(max_examples=25, **SET)
@given(rows=st.integers(1, 3000), cols=st.integers(1, 500), pad=st.integers(1, 9), alpha=st.sampled_from([1.0, -0.5, 3.25]),
       seed=st.integers(0, 10 ** 6))
@example(rows=64, cols=64, pad=4, alpha=1.0, seed=0).via("one workgroup's rows exactly (vector form)")
@example(rows=129, cols=3, pad=1, alpha=-0.5, seed=0).via("one row beyond two workgroups' (scalar form)")
def test_colsum_any_shape(ops, rows, cols, pad, alpha, seed):
    """alpha * column sums of a (rows, cols) view with row stride ld > cols; rows above and below one workgroup's share
    (64 rows in the vector form, ld % 4 == 0 and cols % 4 == 0; 128 in the scalar form)."""
    ld = cols + pad
    x = rnd(rows, ld, seed=seed)
    out = ops.colsum(x.cuda(), alpha, rows=rows, cols=cols, ld=ld)
    assert out.shape == (cols,)
    assert rel_l2(out, alpha * x.double()[:, :cols].sum(0)) < TOL_ATOMIC
