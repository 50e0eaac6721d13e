"""LayerNorm, the folded LayerNorm (producers and consumers) and the BatchNorm statistics at ill-conditioned rows: offset, flat,
near-flat, common-sign, outlier and interleaved rows (tests/stats_conditioning.py), each kernel against float64 under

    C[family] * EPS32 * kappa_class,        kappa = sqrt(1 + (mean * rstd)^2)

-- the bound that holds a two-pass / Chan-merged fp32 algorithm and rejects a one-pass E[x^2] - mean^2 one by a factor of ten and
more (test_stats_conditioning_cpu.py).  Also the multi-row walks of the LayerNorm kernels (rows per wave > 1), which the other
float64 tests never reach.  `MEASURED` collects the largest err / (EPS32 * kappa_class) per family; the last test prints it
(pytest -s) -- the `gpu` column of stats_conditioning.TABLE.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import stats_conditioning as S
from tests.util import merged, ref_partials

pytestmark = pytest.mark.gpu
TOL = 2e-5                   # the fp32 bound of the per-op tests (well-conditioned rows)
TOL_ATOMIC = 5e-5            # ... where reductions are split over workgroups (test_property_train_gpu.py)
EPS = S.LN_EPS
NAN = float("nan")
MEASURED = {}
NAMES = tuple(S.CLASSES)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conformer_amd import _lib, ops as _ops
    assert _lib.load().cfm_device_check() == 0, "not a gfx950 device"
    return _ops


def G(t):
    return t.cuda()


def rnd(*shape, seed=0, scale=1.0):
    return S.noise(*shape, seed=seed) * scale                    # (the same bits on every host: the recorded ratios reproduce)


def hold(family, err, rows, what, factor=1.0, floor=0.0):
    """err <= factor * C[family] * EPS32 * kappa_class (+ floor), kappa_class from `rows` (the rows whose statistics are taken)."""
    unit = S.EPS32 * float(S.kappa(rows, EPS).max())
    ratio = max(0.0, err - floor) / unit / factor
    MEASURED[family] = max(MEASURED.get(family, 0.0), ratio)
    print(f"{family:8s} {ratio:9.3f} of C = {S.C[family]:g}  {what}")
    assert ratio <= S.C[family], (family, what, ratio, err, unit)


def lin(n, k, seed):
    return rnd(n, k, seed=seed) / math.sqrt(k), 0.1 * rnd(n, seed=seed + 1)


def swish(t):
    return t * torch.sigmoid(t)


def stats32(x, parts):
    """The float64 statistics partials of x's rows, rounded to fp32: what an exact producer would have written."""
    return G(ref_partials(x, x.shape[1] // parts).float().contiguous())


# ---- 1. LayerNorm forward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [32, 512, 1024, 2048, 2052])
@pytest.mark.parametrize("name", NAMES)
def test_layernorm_forward(ops, name, d):
    """layernorm, layernorm(emit_stats) and layernorm_train on every class; d = one width per float4-vectors-per-lane instantiation
    (1, 2, 4, 8, 32)."""
    x = S.make(name, 70, d, seed=d)
    gamma, beta = S.ln_params(d)
    ref = S.layernorm64(x, gamma, beta)
    y = ops.layernorm(G(x), G(gamma), G(beta))
    hold("ln_out", S.rel_l2(y, ref), x, f"layernorm {name} d={d}")
    y1, st = ops.layernorm(G(x), G(gamma), G(beta), emit_stats=True)
    assert torch.equal(y1, y) and st.shape == (70, 1, 2)
    assert bool(torch.isfinite(st).all()) and float(st[..., 1].min()) >= 0
    mean, var = merged(st, d)
    hold("merged", S.stats_err(mean, 1 / torch.sqrt(var + EPS), y1.cpu()), y1.cpu(), f"layernorm emit_stats {name} d={d}")
    y2, mean, rstd = ops.layernorm_train(G(x), G(gamma), G(beta))
    assert torch.equal(y2, y) and bool(torch.isfinite(rstd).all())
    hold("ln_stats", S.stats_err(mean, rstd, x), x, f"layernorm_train {name} d={d}")


@pytest.mark.parametrize("d", [32, 512, 1024, 2048, 2052])
def test_layernorm_out16_equals_fp32_rounded_on_mixed_rows(ops, d):
    """test_property_stem16_gpu.py::test_layernorm_out16_equals_fp32_rounded, on the interleaved rows."""
    from conformer_amd import _lib
    lib, rows = _lib.load(), 70
    x = G(S.make("mixed", rows, d, seed=d + 1))
    gamma, beta = (G(t) for t in S.ln_params(d))
    y32, mean32, rstd32 = ops.layernorm_train(x, gamma, beta)
    assert bool(torch.isfinite(y32).all())
    for prec, dt in ((1, torch.bfloat16), (2, torch.float16)):
        y16 = torch.full((rows, d), NAN, device="cuda", dtype=dt)
        mean, rstd = torch.full((rows,), NAN, device="cuda"), torch.full((rows,), NAN, device="cuda")
        _lib.check(lib.cfm_layernorm_fwd_out16_f32(prec, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y16.data_ptr(), mean.data_ptr(),
                                                   rstd.data_ptr(), rows, d, EPS, ops._stream()), "cfm_layernorm_fwd_out16_f32")
        assert torch.equal(y16, y32.to(dt)), (d, prec)
        assert torch.equal(mean, mean32) and torch.equal(rstd, rstd32)


# ---- 2. LayerNorm backward ---------------------------------------------------------------------------------------------------
def ln_bwd_ref(x, w, dy, dres):
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, torch.zeros_like(w)))
    F.layer_norm(xd, (x.shape[-1],), wd, bd, EPS).backward(dy.double())
    return xd.grad + (0 if dres is None else dres.double()), wd.grad, bd.grad


def ln_bwd_run(ops, x, w, dy, dres):
    """layernorm_bwd with the float64 mean / rstd rounded to fp32: only its own (x - mean) * rstd is judged."""
    mu, _, rs = S.stats64(x)
    return ops.layernorm_bwd(G(x), G(w), G(dy), G(mu.float()), G(rs.float()), dres=None if dres is None else G(dres))


@pytest.mark.parametrize("with_dres", [False, True], ids=["nodres", "dres"])
@pytest.mark.parametrize("d", [512, 2052], ids=["d512-fused", "d2052-dx+params"])
@pytest.mark.parametrize("name", ["offset+30", "offset-30", "offset+300", "offset-300", "offset+3000", "nearflat", "mixed"])
def test_layernorm_backward(ops, name, d, with_dres):
    rows = 70
    x = S.make(name, rows, d, seed=d + 2)
    w, dy = 1 + 0.3 * rnd(d, seed=1), rnd(rows, d, seed=2)
    dres = rnd(rows, d, seed=3) if with_dres else None
    got = ln_bwd_run(ops, x, w, dy, dres)
    for what, a, r in zip(("dx", "dgamma", "dbeta"), got, ln_bwd_ref(x, w, dy, dres)):
        hold("ln_out", S.rel_l2(a, r), x, f"layernorm_bwd {what} {name} d={d} dres={with_dres}")


# ---- 3. the multi-row walks ----------------------------------------------------------------------------------------------------
def fwd_rpw(rows):
    return max(1, min(4, rows // 16384))           # layernorm_launch (layernorm.hip)


def bwd_rpw(rows):
    return max(1, min(8, rows // 2048))            # ln_bwd_rows_per_wave (backward_ew.hip)


FWD_ROWS = [32768 + 5, 65536 + 3]
BWD_ROWS = [4097, 6146, 15936, 16384 + 7]          # 4097: 1 row in the last workgroup (8 per workgroup); 6146: 2 (12 per workgroup)


def test_row_counts_reach_the_routes_they_name():
    assert [fwd_rpw(r) for r in FWD_ROWS] == [2, 4] and [bwd_rpw(r) for r in BWD_ROWS] == [2, 3, 7, 8]
    assert [r % (4 * bwd_rpw(r)) for r in BWD_ROWS] == [1, 2, 4, 7]


@pytest.mark.parametrize("name", [S.WELL, "offset+300"])
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("rows", FWD_ROWS, ids=[f"rows{r}-rpw{fwd_rpw(r)}" for r in FWD_ROWS])
def test_layernorm_forward_row_walk(ops, rows, d, name):
    x = S.make(name, rows, d, seed=rows + d)
    gamma, beta = S.ln_params(d)
    ref = S.layernorm64(x, gamma, beta)
    mu, _, rs = S.stats64(x)
    y, mean, rstd = ops.layernorm_train(G(x), G(gamma), G(beta))
    y1, st = ops.layernorm(G(x), G(gamma), G(beta), emit_stats=True)
    assert torch.equal(y1, y) and torch.equal(ops.layernorm(G(x), G(gamma), G(beta)), y)
    m1, v1 = merged(st, d)
    if name == S.WELL:
        assert S.rel_l2(y, ref) < TOL and S.rel_l2(mean, mu) < TOL and S.rel_l2(rstd, rs) < TOL
        yd = y.double().cpu()
        assert S.rel_l2(m1, yd.mean(-1)) < TOL and S.rel_l2(v1, yd.var(-1, unbiased=False)) < TOL
    else:
        hold("ln_out", S.rel_l2(y, ref), x, f"row walk fwd y rows={rows} d={d}")
        hold("ln_stats", S.stats_err(mean, rstd, x), x, f"row walk fwd mean/rstd rows={rows} d={d}")
        hold("merged", S.stats_err(m1, 1 / torch.sqrt(v1 + EPS), y.cpu()), y.cpu(), f"row walk fwd emit_stats rows={rows} d={d}")


@pytest.mark.parametrize("name", [S.WELL, "offset+300"])
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("rows", BWD_ROWS, ids=[f"rows{r}-rpw{bwd_rpw(r)}" for r in BWD_ROWS])
def test_layernorm_backward_row_walk(ops, rows, d, name):
    x = S.make(name, rows, d, seed=rows + d + 1)
    w, dy, dres = 1 + 0.3 * rnd(d, seed=4), rnd(rows, d, seed=5), rnd(rows, d, seed=6)
    got = ln_bwd_run(ops, x, w, dy, dres)
    for what, a, r in zip(("dx", "dgamma", "dbeta"), got, ln_bwd_ref(x, w, dy, dres)):
        if name == S.WELL:
            assert S.rel_l2(a, r) < TOL_ATOMIC, (what, rows, d)
        else:
            hold("ln_out", S.rel_l2(a, r), x, f"row walk bwd {what} rows={rows} d={d}")


# ---- 4. fold producers -------------------------------------------------------------------------------------------------------
def hold_partials(st, stored, parts, what):
    """The partials of the STORED rows: right shape, finite, M2 >= 0, and merged (tests.util.merged) they give the float64 mean and
    rstd of those rows."""
    stored = stored.detach().cpu().reshape(-1, stored.shape[-1])
    d = stored.shape[1]
    assert st.shape == (stored.shape[0], parts, 2), what
    assert bool(torch.isfinite(st).all()) and float(st[..., 1].min()) >= 0, what
    mean, var = merged(st, d)
    assert bool(torch.isfinite(1 / torch.sqrt(var + EPS)).all()), what
    hold("merged", S.stats_err(mean, 1 / torch.sqrt(var + EPS), stored), stored, what)


BIAS_ROWS = {"offset+30": (1.0, 30.0), "offset-30": (1.0, -30.0), "offset+300": (1.0, 300.0), "offset-300": (1.0, -300.0),
             "offset+3000": (1.0, 3000.0), "flat0": (0.0, 0.0), "flat1": (0.0, 1.0), "flat7.3": (0.0, 7.3), "flat-1000": (0.0, -1000.0),
             "nearflat": (1e-2, 73.0)}             # (scale of the product, bias): the product's rows are rows of that class


@pytest.mark.parametrize("N", [32, 128, 512])
@pytest.mark.parametrize("name", list(BIAS_ROWS))
def test_producer_gemm_whose_bias_carries_the_offset(ops, name, N):
    M, K = 70, 48
    scale, off = BIAS_ROWS[name]
    a, w, b = rnd(M, K, seed=N) * scale, rnd(N, K, seed=N + 1) / math.sqrt(K), torch.full((N,), off)
    c0 = ops.linear(G(a), G(w), G(b))
    c1, st = ops.linear(G(a), G(w), G(b), emit_stats=True)
    assert torch.equal(c0, c1)
    hold_partials(st, c1, N // 32, f"linear emit_stats {name} N={N}")


@pytest.mark.parametrize("rows", [70, 257])
@pytest.mark.parametrize("d", [32, 128, 512])
@pytest.mark.parametrize("name", NAMES)
def test_producer_residual_gemm(ops, name, d, rows):
    """The identity epilogue of test_lnfold_gpu.py (x = 1.0 * (0 . W^T + 0) + x) on every class, and a real product whose residual
    carries the class."""
    x = S.make(name, rows, d, seed=rows + d)
    xg, st = ops.linear_residual(G(torch.zeros(rows, 16)), G(torch.zeros(d, 16)), G(torch.zeros(d)), G(x), 1.0, emit_stats=True)
    assert torch.equal(xg.cpu(), x)
    hold_partials(st, xg, d // 32, f"linear_residual identity {name} d={d} rows={rows}")
    a, (w, b) = rnd(rows, 48, seed=7), lin(d, 48, 8)
    c0 = ops.linear_residual(G(a), G(w), G(b), G(x), 0.5)
    c1, st = ops.linear_residual(G(a), G(w), G(b), G(x), 0.5, emit_stats=True)
    assert torch.equal(c0, c1)
    hold_partials(st, c1, d // 32, f"linear_residual product {name} d={d} rows={rows}")


_FFN = {}


def ffn_params(ops, d, seed=10):
    """(raw float32 parameters, (packed weights, folded bias, colsum)) of a feed-forward module of width d, hidden 4 d."""
    if d not in _FFN:
        lw, lb = S.ln_params(d, seed)
        (w1, b1), (w2, b2) = lin(4 * d, d, seed + 2), lin(d, 4 * d, seed + 4)
        wf, bf, cs = ops.fold_layernorm(G(w1), G(b1), G(lw), G(lb))
        _FFN[d] = ((lw, lb, w1, b1, w2, b2), (ops.ffn_pack(wf, G(w2)), bf, cs))
    return _FFN[d]


def ffn64(x, lw, lb, w1, b1, w2, b2, alpha):
    """(x + alpha FFN(x), alpha FFN(x)) in float64."""
    h = swish(S.layernorm64(x, lw, lb) @ w1.double().T + b1.double())
    inc = alpha * (h @ w2.double().T + b2.double())
    return x.double() + inc, inc


def closing(d, offset):
    g2, bt2 = S.ln_params(d, 60)
    return g2, bt2 + offset


@pytest.mark.parametrize("d", [128, 512])
@pytest.mark.parametrize("name", NAMES)
def test_producer_ffn_fused_and_rowchain_statistics(ops, name, d):
    """The statistics ffn_fused writes for its result (d / 32 partials; behind the closing LayerNorm one partial of ITS output) and
    the ones rowchain_pw2_ffn_ln writes; the closing LayerNorm's bias carries an offset of 300, so its output rows are
    ill-conditioned whatever the input."""
    rows = 70
    x = S.make(name, rows, d, seed=d + 3)
    raw, (wp, bf, cs) = ffn_params(ops, d)
    st_in = stats32(x, d // 32)
    y, st = ops.ffn_fused(G(x), st_in, wp, bf, cs, G(raw[5]), 0.5, EPS, emit_stats=True)
    hold_partials(st, y, d // 32, f"ffn_fused emit_stats {name} d={d}")
    g2, bt2 = closing(d, 300.0)
    y2, st2 = ops.ffn_fused(G(x), st_in, wp, bf, cs, G(raw[5]), 0.5, EPS, emit_stats=True, closing_ln=(G(g2), G(bt2), EPS))
    hold_partials(st2, y2, 1, f"ffn_fused closing_ln emit_stats {name} d={d}")
    c, (w2, b2) = rnd(rows, d, seed=9), lin(d, d, 40)
    out, st3 = ops.rowchain_pw2_ffn_ln(G(c), ops.rowgemm_pack(G(w2)), G(b2), G(x), (wp, bf, cs), G(raw[5]), 0.5, EPS, (G(g2), G(bt2), EPS),
                                       want_stats=True)
    hold_partials(st3, out, 1, f"rowchain_pw2_ffn_ln statistics {name} d={d}")


@pytest.mark.parametrize("d", [32, 512, 2052])
def test_producer_layernorm_output_with_offset_bias(ops, d):
    """layernorm(emit_stats) writes the statistics of its OUTPUT: a bias of -300 makes those rows ill-conditioned."""
    x = S.make("mixed", 70, d, seed=d + 4)
    gamma, beta = S.ln_params(d)
    y, st = ops.layernorm(G(x), G(gamma), G(beta - 300.0), emit_stats=True)
    hold_partials(st, y, 1, f"layernorm emit_stats, bias -300, d={d}")


# ---- 5. fold consumers -------------------------------------------------------------------------------------------------------
SHARP_MAX = 4096.0


def hold_increment(y, ref, inc, x, what):
    """y = x + inc with |inc| = O(1): rel-L2 of y is blind at |x| >> 1, so the increment y - x is held as well, on the rows whose
    magnitude leaves it representable (|x| <= 4096: half an ulp of y is 1.2e-4 <= EPS32 * |x|, one unit of the bound's own form).
    The increment also carries the rounding of its own fp32 products (contraction up to 4 d), which does not scale with kappa:
    the per-op TOL of those kernels is added to its bound."""
    hold("fold", S.rel_l2(y, ref), x, what)
    keep = x.abs().amax(-1) <= SHARP_MAX
    got = (y.detach().double().cpu() - x.double())[keep]
    hold("fold", S.rel_l2(got, inc[keep]), x, what + " (increment)", floor=TOL)


@pytest.mark.parametrize("rows", [70, 257])
@pytest.mark.parametrize("d", [32, 128, 512])
@pytest.mark.parametrize("name", NAMES)
def test_consumer_linear_lnfold(ops, name, d, rows):
    """act none / swish / glu against float64 LayerNorm + Linear, the statistics as one partial and as d / 32 partials (exact ones,
    rounded to fp32) and as the producing GEMM wrote them."""
    N = 96
    x = S.make(name, rows, d, seed=rows + d + 5)
    (w, b, gamma, beta), _ = S.fold_params(N, d)
    ref = S.fold64(x, w, b, gamma, beta)
    wf, bf, cs = ops.fold_layernorm(G(w), G(b), G(gamma), G(beta))
    xg, st_gemm = ops.linear_residual(G(torch.zeros(rows, 16)), G(torch.zeros(d, 16)), G(torch.zeros(d)), G(x), 1.0, emit_stats=True)
    for tag, st in (("1 partial", stats32(x, 1)), (f"{d // 32} partials", stats32(x, d // 32)), ("GEMM partials", st_gemm)):
        what = f"linear_lnfold {name} d={d} rows={rows} {tag}"
        hold("fold", S.rel_l2(ops.linear_lnfold(xg, st, wf, bf, cs, EPS), ref), x, what)
        hold("fold", S.rel_l2(ops.linear_lnfold(xg, st, wf, bf, cs, EPS, act="swish"), swish(ref)), x, what + " swish")
        n = N // 2
        hold("fold", S.rel_l2(ops.linear_lnfold(xg, st, wf, bf, cs, EPS, glu=True), ref[:, :n] * torch.sigmoid(ref[:, n:])), x, what + " glu")


@pytest.mark.parametrize("rows", [70, 257])
@pytest.mark.parametrize("d", [128, 512])
@pytest.mark.parametrize("name", NAMES)
def test_consumer_ffn_fused(ops, name, d, rows):
    """All three finish modes against float64; behind the closing LayerNorm the bound doubles (test_property_gpu.py)."""
    x = S.make(name, rows, d, seed=rows + d + 6)
    raw, (wp, bf, cs) = ffn_params(ops, d)
    ref, inc = ffn64(x, *raw, 0.5)
    g2, bt2 = closing(d, 0.0)
    ref2 = S.layernorm64(ref, g2, bt2)
    for parts in (1, d // 32):
        st_in = stats32(x, parts)
        what = f"ffn_fused {name} d={d} rows={rows} parts={parts}"
        y0 = ops.ffn_fused(G(x), st_in, wp, bf, cs, G(raw[5]), 0.5, EPS)
        hold_increment(y0, ref, inc, x, what)
        y1, _ = ops.ffn_fused(G(x), st_in, wp, bf, cs, G(raw[5]), 0.5, EPS, emit_stats=True)
        assert torch.equal(y1, y0)
        y2 = ops.ffn_fused(G(x), st_in, wp, bf, cs, G(raw[5]), 0.5, EPS, closing_ln=(G(g2), G(bt2), EPS))
        hold("fold", S.rel_l2(y2, ref2), torch.cat([x.double(), ref]), what + " closing_ln", factor=2.0)


@pytest.mark.parametrize("rows", [70, 257])
@pytest.mark.parametrize("d", [128, 512])
@pytest.mark.parametrize("name", NAMES)
def test_consumer_row_chains(ops, name, d, rows):
    """K1 (FFN + folded q|k|v), K2 (out_proj + residual, statistics in the kernel, folded GLU) and K3 (pw2 + residual, FFN, closing
    LayerNorm): the class enters as the rows (K1) or as the residual (K2, K3), so the rows the kernels normalise are of that class."""
    x = S.make(name, rows, d, seed=rows + d + 7)
    raw, ffn = ffn_params(ops, d)
    # K1
    law, lab = S.ln_params(d, 20)
    wq, bq = lin(3 * d, d, 22)
    wqf, bqf, csq = ops.fold_layernorm(G(wq), G(bq), G(law), G(lab))
    y, qkv = ops.rowchain_ffn_qkv(G(x), stats32(x, d // 32), ffn, G(raw[5]), 0.5, EPS, ops.rowgemm_pack(wqf), bqf, csq, EPS)
    y_ref, inc = ffn64(x, *raw, 0.5)
    hold_increment(y, y_ref, inc, x, f"rowchain_ffn_qkv y {name} d={d} rows={rows}")
    q_ref = S.layernorm64(y_ref, law, lab) @ wq.double().T + bq.double()
    # two folded LayerNorms in a row (of x, then of y, which carries the first one's error): kappa over both sets of rows, twice
    hold("fold", S.rel_l2(qkv, q_ref), torch.cat([x.double(), y_ref]), f"rowchain_ffn_qkv qkv {name} d={d} rows={rows}", factor=2.0)
    # K2
    ctx, (wo, bo), (wg, bg) = rnd(rows, d, seed=2), lin(d, d, 30), lin(2 * d, d, 32)
    lcw, lcb = S.ln_params(d, 34)
    wgf, bgf, csg = ops.fold_layernorm(G(wg), G(bg), G(lcw), G(lcb))
    y2, g = ops.rowchain_out_glu(G(ctx), ops.rowgemm_pack(G(wo)), G(bo), G(x), ops.rowgemm_pack(wgf, glu=True), bgf, csg, EPS)
    inc2 = ctx.double() @ wo.double().T + bo.double()
    y2_ref = inc2 + x.double()
    hold_increment(y2, y2_ref, inc2, x, f"rowchain_out_glu y2 {name} d={d} rows={rows}")
    h = S.layernorm64(y2_ref, lcw, lcb) @ wg.double().T + bg.double()
    hold("fold", S.rel_l2(g, h[:, :d] * torch.sigmoid(h[:, d:])), y2_ref, f"rowchain_out_glu g {name} d={d} rows={rows}")
    # K3
    c, (w2, b2) = rnd(rows, d, seed=4), lin(d, d, 40)
    g2, bt2 = closing(d, 0.0)
    out, _ = ops.rowchain_pw2_ffn_ln(G(c), ops.rowgemm_pack(G(w2)), G(b2), G(x), ffn, G(raw[5]), 0.5, EPS, (G(g2), G(bt2), EPS))
    y3 = c.double() @ w2.double().T + b2.double() + x.double()
    y4 = ffn64(y3, *raw, 0.5)[0]
    hold("fold", S.rel_l2(out, S.layernorm64(y4, g2, bt2)), torch.cat([y3, y4]), f"rowchain_pw2_ffn_ln {name} d={d} rows={rows}", factor=2.0)


@pytest.mark.parametrize("B,T,C,K", [(1, 70, 64, 31), (1, 257, 128, 15), (2, 300, 512, 31)])
def test_convmod_fused_keeps_its_bits_on_mixed_rows(ops, B, T, C, K):
    x = G(S.make("mixed", B * T, C, seed=T))
    stats = stats32(x.cpu(), C // 32)
    (w, b), (gamma, beta) = lin(2 * C, C, 50), S.ln_params(C, 52)
    fold = ops.fold_layernorm(G(w), G(b), G(gamma), G(beta))
    dw = (G(0.2 * rnd(C, 1, K, seed=54)), G(0.1 * rnd(C, seed=55)), G(1 + 0.2 * rnd(C, seed=56)), G(0.1 * rnd(C, seed=57)),
          G(0.2 * rnd(C, seed=58)), G(rnd(C, seed=59).abs() + 0.5))
    ref = ops.dwconv_bn_swish(ops.linear_lnfold(x.view(B, T, C), stats, *fold, EPS, glu=True), *dw, EPS)
    got = ops.convmod_glu_dwconv(x.view(B, T, C), stats, *fold, EPS, *dw, EPS)
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {ref.numel()} elements differ"


# ---- 6. BatchNorm statistics ---------------------------------------------------------------------------------------------------
def hold_channels(mean, var, values, groups, what):
    """Per class of channels: mean and the rstd of the returned variance against the float64 statistics of `values` (C, n)."""
    for name, idx in groups.items():
        v = values[idx]
        hold("bn", S.stats_err(mean.cpu()[idx], 1 / torch.sqrt(var.double().cpu()[idx] + EPS), v), v, f"{what} {name}")


DW_KINDS = ("bias0", "bias30", "bias300", "bias3000", "zerotap", "nearconst")


@pytest.mark.parametrize("K", [3, 31])
def test_dwconv_bn_statistics_and_eval_forward(ops, K):
    """B = 2, T = 200, C = 70: several time segments, a ragged channel block.  Channel c is of kind c % 6: conv bias 0 / 30 / 300 /
    3000 times the channel's spread, all-zero taps (constant output 7.3) or a spread of 1e-2 on a bias of 73 (near-constant).
    The running buffers start at zero, so that what the update adds is held by itself (the (1 - momentum) term:
    test_property_train_gpu.py)."""
    B, T, C, mom = 2, 200, 70, 0.1
    g, w = rnd(B, T, C, seed=K), rnd(C, 1, K, seed=K + 1) / 3
    kind = torch.arange(C) % len(DW_KINDS)
    spread = w.reshape(C, K).norm(dim=1)
    b = torch.zeros(C)
    for i, m in enumerate((0.0, 30.0, 300.0, 3000.0)):
        b[kind == i] = m * spread[kind == i]
    w[kind == 4] = 0.0
    b[kind == 4] = 7.3
    w[kind == 5] *= (1e-2 / spread[kind == 5])[:, None, None]
    b[kind == 5] = 73.0
    groups = {nm: (kind == i).nonzero()[:, 0] for i, nm in enumerate(DW_KINDS)}
    c64 = F.conv1d(g.double().transpose(1, 2), w.double(), b.double(), padding=K // 2, groups=C)         # (B, C, T)
    vals = c64.transpose(0, 1).reshape(C, B * T)
    n = B * T
    rm, rv = G(torch.zeros(C)), G(torch.zeros(C))
    mean, var = ops.dwconv_bn_batch_stats(G(g), G(w), G(b), rm, rv, mom)
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(var).all()) and float(var.min()) >= 0
    hold_channels(mean, var, vals, groups, f"dwconv_bn_batch_stats K={K}")
    hold_channels(rm.double().cpu() / mom, rv.double().cpu() / mom * ((n - 1) / n), vals, groups, f"dwconv_bn_batch_stats K={K} running")
    bw, bb = 1 + 0.2 * rnd(C, seed=5), 1 + 0.1 * rnd(C, seed=6)
    y = ops.dwconv_bn_swish(G(g), G(w), G(b), G(bw), G(bb), mean.clone(), var.clone(), EPS)
    mu, v64 = vals.mean(1), vals.var(1, unbiased=False)
    ref = swish((c64 - mu[None, :, None]) / torch.sqrt(v64[None, :, None] + EPS) * bw.double()[None, :, None] + bb.double()[None, :, None])
    for name, idx in groups.items():
        hold("bn", S.rel_l2(y.transpose(1, 2)[:, idx], ref[:, idx]), vals[idx], f"dwconv_bn_swish K={K} {name}")


def test_swish_bn_statistics_and_eval_forward(ops):
    """rows = 300, C = 64; the columns of swish(h) play the classes (S.BN_CLASSES in turn; h = the class where it is positive).
    Running buffers from zero, as above."""
    rows, C, mom = 300, 64, 0.1
    names = [S.BN_CLASSES[j % len(S.BN_CLASSES)] for j in range(C)]
    h = S.bn_columns(rows, names, seed=400)
    vals = swish(h.double()).t().contiguous()                                                              # (C, rows)
    groups = {nm: torch.tensor([j for j in range(C) if names[j] == nm]) for nm in S.BN_CLASSES}
    rm, rv = G(torch.zeros(C)), G(torch.zeros(C))
    mean, var = ops.swish_bn_batch_stats(G(h), rm, rv, mom)
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(var).all()) and float(var.min()) >= 0
    hold_channels(mean, var, vals, groups, "swish_bn_batch_stats")
    hold_channels(rm.double().cpu() / mom, rv.double().cpu() / mom * ((rows - 1) / rows), vals, groups, "swish_bn_batch_stats running")
    bw, bb = 1 + 0.2 * rnd(C, seed=7), 1 + 0.1 * rnd(C, seed=8)
    z = ops.swish_bn_eval(G(h), mean.clone(), var.clone(), G(bw), G(bb), EPS)
    mu, v64 = vals.mean(1), vals.var(1, unbiased=False)
    ref = (vals.t() - mu) / torch.sqrt(v64 + EPS) * bw.double() + bb.double()
    for name, idx in groups.items():
        hold("bn", S.rel_l2(z[:, idx], ref[:, idx]), vals[idx], f"swish_bn_eval {name}")


def test_zz_report_measured_constants():
    """Prints the largest err / (EPS32 * kappa_class) per family seen in this run (the `gpu` column of stats_conditioning.TABLE)."""
    print("\nMEASURED", {k: round(v, 3) for k, v in sorted(MEASURED.items())})
    for fam, r in MEASURED.items():
        assert r <= S.C[fam]
