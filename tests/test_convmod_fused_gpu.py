"""The one-kernel middle of ConvolutionModule (csrc/convmod_fused_f32.hip; fp32 inference): pointwise_conv_1 + GLU with the
LayerNorm folded, depthwise conv, BatchNorm (eval) and Swish.  The yardstick is exact: the fused kernel must return, bit for bit,
what ops.linear_lnfold(..., glu=True) followed by ops.dwconv_bn_swish returns (same accumulation chains, same epilogue helpers,
same fmaf order), so every comparison is torch.equal and no tolerance is chosen.  The op is called directly: the shape predicate
ops.convmod_fused_ok only guards the module's choice."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, T', C, K): an utterance shorter than the halo, exact tile fill, chunk seams (257 / 300 / 483 frames), two channel groups
# (value / gate pairing across groups), every tap count, and the full K = 512 loop
CASES = [(1, 1, 64, 31), (2, 15, 64, 31), (2, 16, 64, 7), (3, 31, 128, 31), (2, 249, 128, 31), (1, 256, 64, 31), (1, 257, 64, 31),
         (2, 300, 128, 15), (1, 483, 64, 3), (1, 256, 512, 31)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conformer_amd import _lib, ops as _ops
    assert _lib.load().cfm_device_check() == 0, "not a gfx950 device"
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def inputs(ops, B, T, C, K):
    """x = rows written by a residual GEMM together with their statistics partials (common offset 3: the variance is a small
    difference of large sums unless the partials are merged Chan-style), folded pointwise_conv_1, random taps and BN statistics."""
    s = 1000 * K + C + T
    a, w, b = rnd(B * T, C, seed=s), rnd(C, C, seed=s + 1, scale=1 / math.sqrt(C)), rnd(C, seed=s + 2, scale=0.1)
    res = rnd(B * T, C, seed=s + 3) + 3.0
    x, stats = ops.linear_residual(a, w, b, res, 1.0, emit_stats=True)
    pw_w, pw_b = rnd(2 * C, C, 1, seed=s + 4, scale=1 / math.sqrt(C)), rnd(2 * C, seed=s + 5, scale=0.1)
    gamma, beta = 1 + rnd(C, seed=s + 6, scale=0.3), rnd(C, seed=s + 7, scale=0.2)
    wf, bf, cs = ops.fold_layernorm(pw_w, pw_b, gamma, beta)
    dw_w, dw_b = rnd(C, 1, K, seed=s + 8, scale=0.2), rnd(C, seed=s + 9, scale=0.1)
    bn = (1 + rnd(C, seed=s + 10, scale=0.2), rnd(C, seed=s + 11, scale=0.1), rnd(C, seed=s + 12, scale=0.2),
          rnd(C, seed=s + 13).abs() + 0.5)
    return x.view(B, T, C), stats, (wf, bf, cs), (dw_w, dw_b) + bn


def two_kernels(ops, x, stats, fold, dw):
    g = ops.linear_lnfold(x, stats, *fold, 1e-5, glu=True)
    return ops.dwconv_bn_swish(g, *dw, 1e-5)


@pytest.mark.parametrize("B,T,C,K", CASES)
def test_bit_equal_to_glu_gemm_then_depthwise_kernel(ops, B, T, C, K):
    x, stats, fold, dw = inputs(ops, B, T, C, K)
    ref = two_kernels(ops, x, stats, fold, dw)
    got = ops.convmod_glu_dwconv(x, stats, *fold, 1e-5, *dw, 1e-5)
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {ref.numel()} elements differ, max {float((got - ref).abs().max()):.3e}"


@pytest.mark.parametrize("T", [249, 257])
def test_nothing_outside_the_output_is_written(ops, T):
    """y points into a sentinel-filled arena: clamped rows (frames >= T' of the last tile) and recomputed margin rows must never
    be stored, so every value outside the B * T' * C outputs stays what it was."""
    from conformer_amd import _lib
    B, C, K, GUARD, SENT = 2, 128, 31, 300 * 128, -7.25
    x, stats, fold, dw = inputs(ops, B, T, C, K)
    ref = two_kernels(ops, x, stats, fold, dw)
    n = B * T * C
    arena = torch.full((n + 2 * GUARD,), SENT, device="cuda", dtype=torch.float32)
    y = arena[GUARD:GUARD + n]
    st = _lib.load().cfm_convmod_glu_dwconv_f32(x.data_ptr(), C, stats.data_ptr(), stats.shape[1], 1e-5, fold[0].data_ptr(),
                                                fold[1].data_ptr(), fold[2].data_ptr(), *[t.data_ptr() for t in dw], 1e-5,
                                                y.data_ptr(), C, B, T, C, K, torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    assert bool((arena[:GUARD] == SENT).all()) and bool((arena[GUARD + n:] == SENT).all())
    assert torch.equal(y.view(B, T, C), ref)


def test_block_takes_the_fused_kernel_and_keeps_its_bits(ops):
    """One ConformerBlock at (B, T', d) = (32, 249, 512) in fused_chain with the switch on and off: equal outputs and statistics;
    with the switch on the depthwise entry is not called and the block is one launch shorter."""
    from conformer_amd import _lib
    from conformer_amd.model.utils.block import ConformerBlock
    torch.manual_seed(11)
    d, B, T, H = 512, 32, 249, 8
    blk = ConformerBlock(d, H, 31).cuda().eval()
    lib = _lib.load()
    called = []
    real = lib.cfm_dwconv_bn_swish_fwd_f32

    class Counting:
        def __call__(self, *a):
            called.append(1)
            return real(*a)

    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
        blk.conv.batch_norm.running_mean.normal_(0, 0.2); blk.conv.batch_norm.running_var.uniform_(0.5, 1.5)
        x = torch.randn(B, T, d, device="cuda") + 0.2
        _, st = ops.linear_residual(torch.zeros(B * T, 32, device="cuda"), torch.zeros(d, 32, device="cuda"),
                                    torch.zeros(d, device="cuda"), x.view(-1, d), 1.0, emit_stats=True)   # the partials of x's rows
        table = ops.relpos_table(torch.exp(torch.arange(0, d, 2, device="cuda") * -(math.log(10000.0) / d))[None], T)
        L = torch.randint(100, T + 1, (B,), device="cuda"); L[0] = T
        assert ops.convmod_fused_ok(B, T, d, 31)
        prev = ops.set_convmod_fused(False)
        lib.cfm_dwconv_bn_swish_fwd_f32 = Counting()
        try:
            blk.fused_chain(x, table, L, x_stats=st, want_stats=True)    # (the one-time weight packs are C-ABI calls too)
            called.clear()
            n0 = _lib.CALLS[0]
            ref, st_ref = blk.fused_chain(x, table, L, x_stats=st, want_stats=True)
            calls_off, dw_off = _lib.CALLS[0] - n0, len(called)
            ops.set_convmod_fused(True)
            n0 = _lib.CALLS[0]
            out, st_out = blk.fused_chain(x, table, L, x_stats=st, want_stats=True)
            calls_on, dw_on = _lib.CALLS[0] - n0, len(called) - dw_off
        finally:
            lib.cfm_dwconv_bn_swish_fwd_f32 = real
            ops.set_convmod_fused(prev)
    assert dw_off == 1 and dw_on == 0
    assert calls_on == calls_off - 1 == 8
    assert torch.equal(out, ref) and torch.equal(st_out, st_ref)
