"""Every site that draws the dropout mask against the integer restatement of the contract (tests/dropout_restatement.py): the
zero pattern must equal it EXACTLY, a kept value is float32(1 / (1 - p)) (or that value rounded to the output type).

  a. the stand-alone kernels (cfm_dropout_f32, cfm_dropout_out16_f32 in bf16 and fp16);
  b. the training forward GEMM, ops.linear_train -- its own kernel instantiations (EPF_F32_OUT, Z-save and mask code), which the
     forward sweep of tests/test_property_gemm_gpu.py never runs: every fp32 tile by shape, every 16-bit tile, 16-bit C / Z,
     the per-element epilogue.  Product one (A = 1, W = 1 / K, b = 0) makes C the mask itself; product two (random operands)
     goes against float64 x the restated mask on the check_rows subset;
  c. the attention forward, fp32 and both 16-bit routes: q = k = 0 and V = identity make the context the mask, so the mask the
     forward applies (dropout_keep4u at odd T) is observed directly and not through a backward that replays it;
  d. the modules, with the masks restated and not extracted from the device: ConvolutionModule, the encoder's input projection,
     a whole ConformerBlock step (seven seeds in draw order), in fp32 and under autocast.

Bars: TOL = 2e-5 forward (tests/test_property_gemm_gpu.py), 5e-5 gradients (tests/test_dropout_gpu.py), 1e-2 per tensor under
autocast (tests/autocast_cases.py).  No site was found to deviate from the index maps of the restatement.
"""
import contextlib
import math

import numpy as np
import pytest
import torch

from oracle import conformer_oracle as O
from tests import dropout_restatement as R
from tests.autocast_cases import ZERO_GRAD
from tests.test_property_gemm_gpu import (DT16, F16, F32, F32_CELLS, TILE16, TOL, assert_close, check_rows, force16, grnd,
                                          last_tile)
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
P = R.SITE_P
TOL_GRAD = 5e-5
BAR16 = 1e-2
PRECS = [1, 2]
PREC_IDS = ["bf16", "fp16"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(dev):
    from conformer_amd import _lib, ops as _ops
    assert _lib.load().cfm_device_check() == 0, "not a gfx950 device"
    return _ops


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def rmask(shape, p, seed):
    """The restated mask as a float64 tensor."""
    return torch.from_numpy(R.mask(shape, p, seed)).double()


def ulp_of(value: float, dtype) -> float:
    return torch.finfo(dtype).eps * 2.0 ** math.floor(math.log2(abs(value)))


def assert_is_mask(y, keep, p, what, ulps=2):
    """y (any shape, C-order) is the mask: zero exactly where the restatement drops, else within `ulps` ulp of inv_keep in y's
    type (0: the same bits -- the device divides and multiplies in IEEE fp32)."""
    kd = torch.from_numpy(np.ascontiguousarray(keep).reshape(tuple(y.shape))).to(y.device)
    nz = y != 0
    if not torch.equal(nz, kd):
        bad = (nz != kd).reshape(-1).nonzero().reshape(-1)
        raise AssertionError(f"{what}: zero pattern differs from the restatement at {bad.numel()} of {y.numel()} elements, "
                             f"first flat indices {bad[:8].tolist()}")
    if bool(kd.any()):
        want = torch.tensor(float(R.inv_keep(p)), dtype=torch.float32).to(y.dtype)
        err = float((y[kd].float() - want.float()).abs().max())
        assert err <= ulps * ulp_of(float(want), y.dtype), f"{what}: a kept value is {err:.3e} from {float(want)!r}"


# ==== a. stand-alone kernels =================================================================================================
@pytest.mark.parametrize("seed", R.SEEDS, ids=[f"seed{i}" for i in range(len(R.SEEDS))])
def test_standalone_kernels_are_the_restated_mask(ops, dev, seed):
    """cfm_dropout_f32 and cfm_dropout_out16_f32 (bf16, fp16) on ones: n = 4 and 8 (one and two hashes), 1024 and 1032 (one
    workgroup exactly; one more group of eight), 2^20 (where ceil against floor in the threshold shows, see the CPU tests)."""
    for n in R.STANDALONE_SIZES:
        ones = torch.ones(n, device=dev)
        for p in R.STANDALONE_P:
            keep = R.keep_range(n, p, seed)
            assert_is_mask(ops.dropout_apply(ones, p, seed), keep, p, f"f32 n {n} p {p}")
            for prec in PRECS:
                with ops.precision(prec):
                    y = ops.dropout_apply(ones, p, seed, for_gemm=True)
                assert y.dtype == (DT16[prec] if n % 8 == 0 else torch.float32)     # (n = 4: no group of eight, the fp32 kernel)
                assert_is_mask(y, keep, p, f"out16 {PREC_IDS[prec - 1]} n {n} p {p}")
    # any input: one IEEE multiply per element
    x = torch.randn(1032, generator=torch.Generator().manual_seed(3)).to(dev)
    m = torch.from_numpy(R.mask((1032,), 0.25, seed)).to(dev)
    assert torch.equal(ops.dropout_apply(x, 0.25, seed), x * m)


def test_standalone_p_zero_and_p_one(ops, dev):
    from conformer_amd._lib import ConformerHipError
    x = torch.randn(16, 72, generator=torch.Generator().manual_seed(4)).to(dev)
    assert ops.dropout_apply(x, 0.0, 0) is x
    for prec in PRECS:
        with ops.precision(prec):
            y = ops.dropout_apply(x, 0.0, 0, for_gemm=True)
            assert y.dtype == DT16[prec] and torch.equal(y, x.to(DT16[prec]))        # p = 0: the plain cast
            for p in (1.0, 1.5):
                with pytest.raises(ConformerHipError):
                    ops.dropout_apply(x, p, 7, for_gemm=True)
    for p in (1.0, 1.5):
        with pytest.raises(ConformerHipError):
            ops.dropout_apply(x, p, 7)
        with pytest.raises(ConformerHipError):
            ops.linear_train("bias", x, x[:8], x[0, :8].contiguous(), drop_p=p, seed=7)


# ==== b. ops.linear_train ====================================================================================================
def train_gemm(ops, epi, a, w, b, r, seed, for_gemm=False):
    """(C, Z or None) of the training forward with the epilogues the modules use: bias, Swish with Z saved, residual at 0.5."""
    if epi == "bias":
        return ops.linear_train("bias", a, w, b, drop_p=P, seed=seed, for_gemm=for_gemm), None
    if epi == "swish":
        return ops.linear_train("swish", a, w, b, drop_p=P, seed=seed, save_z=True, for_gemm=for_gemm)
    return ops.linear_train("residual", a, w, b, residual=r, alpha=0.5, drop_p=P, seed=seed, for_gemm=for_gemm), None


def gemm_site(ops, dev, prec, M, N, K, epis, family, tile, force=0, c16=False):
    """Both products at one (precision, tile) cell, both seeds.  prec 0: fp32; else the 16-bit routes under ops.precision.
    c16: additionally the 16-bit C / Z outputs (for_gemm=True) of the bias and Swish epilogues, which must be the fp32 outputs
    rounded."""
    assert K & (K - 1) == 0, "product one needs K a power of two"
    mode = ops.precision(prec) if prec else contextlib.nullcontext()
    rows = check_rows(M)
    rd = rows.to(dev)

    def check_tile(what):
        rec = last_tile(family)
        want = (*tile, 4, 1) if family == F32 else tile
        assert rec[:len(want)] == want, (what, M, N, K, rec)
        return rec

    a, w = grnd(M, K, seed=M + N), grnd(N, K, seed=M + N + 1, scale=1 / math.sqrt(K))
    b, r = grnd(N, seed=M + N + 2), grnd(M, N, seed=M + N + 3)
    dt = DT16[prec] if prec else torch.float32
    y = a[rd].to(dt).double().cpu() @ w.to(dt).double().cpu().t() + b.double().cpu()       # (the operands as the route rounds them)
    rr = r[rd].double().cpu()
    ones, wk, b0 = torch.ones(M, K, device=dev), torch.full((N, K), 1.0 / K, device=dev), torch.zeros(N, device=dev)
    with mode, force16(force):
        for seed in R.SITE_SEEDS:
            keep = R.keep_range(M * N, P, seed).reshape(M, N)
            # product one: C is the mask
            c, _ = train_gemm(ops, "bias", ones, wk, b0, None, seed)
            check_tile("product one")
            assert c.dtype == torch.float32
            assert_is_mask(c, keep, P, f"product one {M}x{N}x{K} seed {seed}", ulps=0)         # bit for bit
            if c16:
                c, _ = train_gemm(ops, "bias", ones, wk, b0, None, seed, for_gemm=True)
                assert check_tile("product one, 16-bit C")[5] == 1 and c.dtype == dt
                assert_is_mask(c, keep, P, f"product one, 16-bit C {M}x{N}x{K} seed {seed}")
            # product two: random operands against float64 x the restated mask
            m = torch.from_numpy(keep[rows.numpy()]).double() * float(R.inv_keep(P))
            dropped = m == 0
            for epi in epis:
                c, z = train_gemm(ops, epi, a, w, b, r, seed)
                check_tile(epi)
                got = c[rd].double().cpu()
                what = f"{epi} {M}x{N}x{K} seed {seed}"
                if epi == "bias":
                    ref = y * m
                elif epi == "swish":
                    ref = O.swish(y) * m
                    assert_close(z, y, rows, M, tile[0], tile[1], TOL, what + " Z (the unmasked pre-activation)")
                else:
                    ref = 0.5 * y * m + rr
                assert_close(c, ref, rows, M, tile[0], tile[1], TOL, what)
                if epi == "residual":          # a dropped element is the residual itself (a kept one missing: assert_close above)
                    assert bool((got == rr)[dropped].all()), what + ": C == R where the mask drops"
                else:
                    assert torch.equal(got == 0, dropped), what + ": C == 0 exactly where the mask drops"
                if c16 and epi != "residual":
                    c2, z2 = train_gemm(ops, epi, a, w, b, r, seed, for_gemm=True)
                    assert check_tile(epi + ", 16-bit C")[5] == 1
                    assert c2.dtype == dt and torch.equal(c2, c.to(dt)), what + ": 16-bit C != fp32 C rounded"
                    if z is not None:
                        assert z2.dtype == dt and torch.equal(z2, z.to(dt)), what + ": 16-bit Z != fp32 Z rounded"


@pytest.mark.parametrize("cell", list(R.GEMM_F32))
def test_linear_train_f32_every_tile(ops, dev, cell):
    """choose_tile's four tiles through cfm_gemm_train_f32, which records its tile as the inference entries do.  The smallest M
    and N of each cell of F32_CELLS that serves bias / Swish / residual, with its first K.  Every such N is 1 mod 4: the
    per-element epilogue in every tile."""
    M, N, K, epis, tile = R.GEMM_F32[cell]
    (mlo, _), (nlo, _), Ks, cell_epis, cell_tile = F32_CELLS[cell]
    assert (M, N, K, tile) == (mlo, nlo, Ks[0], cell_tile)
    assert epis == tuple(e for e in ("bias", "swish", "residual") if {"residual": "resid"}.get(e, e) in cell_epis)
    gemm_site(ops, dev, 0, M, N, K, epis, F32, tile)


@pytest.mark.parametrize("cell", list(R.GEMM_F32_VEC))
def test_linear_train_f32_big_tiles_vectorised(ops, dev, cell):
    """The big fp32 tiles again at N % 4 == 0, three columns further into their cells: the vectorised epilogue, one hash per four
    columns (the FFN1 product of a training step runs the 128x64 tile this way)."""
    M, _, K, epis, tile = R.GEMM_F32[cell]
    gemm_site(ops, dev, 0, M, R.GEMM_F32_VEC[cell], K, epis, F32, tile)


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("cell", list(R.GEMM_16))
def test_linear_train_16bit_every_tile(ops, dev, cell, prec):
    """Every tile of the 16-bit family through cfm_debug_gemm_mfma16_force_tile (the 128x128 tile also needs its shape, t128 >=
    512), fp32 C and 16-bit C / Z.  The forced 128x64 tile serves bias and residual only (launch_t sends Swish to 64x64)."""
    M, N, K = R.GEMM_16[cell]
    force, tile, cell_epis, _ = TILE16[cell]
    epis = tuple(e for e in ("bias", "swish", "residual") if {"residual": "resid"}.get(e, e) in cell_epis)
    gemm_site(ops, dev, prec, M, N, K, epis, F16, tile, force=force, c16=True)


@pytest.mark.parametrize("prec", [0, 1, 2], ids=["f32"] + PREC_IDS)
@pytest.mark.parametrize("shape", R.GEMM_ODD_N, ids=[f"n_mod4_{s[1] % 4}" for s in R.GEMM_ODD_N])
def test_linear_train_per_element_epilogue(ops, dev, shape, prec):
    """N % 4 in {1, 2, 3}: the scalar path of gemm_epilogue_at (dropout_keep, one hash per element) at the fp32 default tile and
    the 16-bit 64x64 tile, more than one tile either way."""
    M, N, K = shape
    gemm_site(ops, dev, prec, M, N, K, ("bias", "swish", "residual"), F16 if prec else F32, (64, 64, 4) if prec else (64, 64),
              force=5 if prec else 0)


# ==== c. attention forward ===================================================================================================
@pytest.mark.parametrize("prec", [0, 1, 2], ids=["f32"] + PREC_IDS)
@pytest.mark.parametrize("case", R.ATTENTION, ids=[f"T{c[2]}" for c in R.ATTENTION])
def test_attention_forward_context_is_the_mask(ops, dev, case, prec):
    """q = k = 0, zero biases and positions: every valid key of a row has probability 1 / L_b.  V[b, k, h, :] = e_k, so
    ctx[b, i, h, k] = keep[b, h, i, k] * inv_keep / L_b: the context shows the mask the forward applied, at the index
    ((b H + h) T + i) T + k.  T = 61 and 63: rows start at every alignment (dropout_keep4u, two hashes per four keys); T = 64:
    aligned rows; lengths [T, 37]: a ragged last key tile.  The 16-bit routes round p * keep to the 16-bit type before the
    P.V product; the normalisation by 1 / L is fp32 in all three: a reciprocal and a product, each rounded once (2^-24), so
    kept weight x L is within 2^-23 of inv_keep as the route rounds it; the bar is four times that."""
    B, H, T = case
    dh, d = 64, 128
    lengths = [T, 37]
    qkv = torch.zeros(B, T, 3 * d)
    for h in range(H):
        qkv[:, torch.arange(T), 2 * d + h * dh + torch.arange(T)] = 1.0
    pos, u, v = torch.zeros(2 * T - 1, d, device=dev), torch.zeros(H, dh, device=dev), torch.zeros(H, dh, device=dev)
    L = torch.tensor(lengths, device=dev)
    inv = torch.tensor(float(R.inv_keep(P)), dtype=torch.float32)
    inv_route = float(inv.to(DT16[prec]).float()) if prec else float(inv)
    for seed in R.SITE_SEEDS:
        with (ops.precision(prec) if prec else contextlib.nullcontext()):
            ctx, lse = ops.relpos_attention_train(qkv.to(dev), pos, u, v, L, H, drop_p=P, seed=seed)
        keep = R.keep(seed, R.attention_index(B, H, T), P)                                   # (B, H, T, T)
        assert np.array_equal(keep, R.keep_range(B * H * T * T, P, seed).reshape(B, H, T, T))
        got = ctx.view(B, T, H, dh).permute(0, 2, 1, 3).double().cpu()                       # (B, H, T (query), dh (= key))
        for b in range(B):
            Lb = lengths[b]
            k_b = torch.from_numpy(keep[b, :, :, :Lb])
            g = got[b, :, :, :Lb]
            assert torch.equal(g != 0, k_b), f"T {T} seed {seed} batch {b}: zero pattern of the context != restated mask"
            assert not bool(got[b, :, :, Lb:].any()), "masked keys and unused dimensions carry no weight"
            err = float(((g * Lb)[k_b] - inv_route).abs().max() / inv_route)
            assert err <= 2.0 ** -21, f"T {T} seed {seed} batch {b}: kept weight x L is {err:.2e} from {inv_route!r}"
        assert rel_l2(lse, torch.log(torch.tensor(lengths, dtype=torch.float64))[:, None, None].expand(B, H, T)) < 1e-6


# ==== d. modules =============================================================================================================
def params64(Pm, pre):
    """The sub-module's parameters and buffers in float64; the floating-point ones are leaves that collect gradients."""
    out = {}
    for k, t in Pm.items():
        if k.startswith(pre):
            out[k[len(pre):]] = t.double().requires_grad_(True) if t.is_floating_point() else t
    return out


def ffn_ref(x, Pd, pre, m1, m2):
    h = O.layer_norm(x, Pd[pre + "layer_norm.weight"], Pd[pre + "layer_norm.bias"])
    h = O.swish(h @ Pd[pre + "hidden_linear.weight"].t() + Pd[pre + "hidden_linear.bias"]) * m1
    return 0.5 * ((h @ Pd[pre + "out_linear.weight"].t() + Pd[pre + "out_linear.bias"]) * m2) + x


def attention_ref(x, pe, L, Pd, pre, H, ma, mo):
    """attention.py:14-18,47-102 with dropout on the probabilities (ma, (B,H,T,T)) and on the projected context (mo)."""
    B, T, d = x.shape
    dh = d // H
    a = pre + "attention."
    xn = O.layer_norm(x, Pd[pre + "layer_norm.weight"], Pd[pre + "layer_norm.bias"])
    q = (xn @ Pd[a + "query_proj.weight"].t() + Pd[a + "query_proj.bias"]).view(B, T, H, dh)
    k = (xn @ Pd[a + "key_proj.weight"].t() + Pd[a + "key_proj.bias"]).view(B, T, H, dh)
    v = (xn @ Pd[a + "value_proj.weight"].t() + Pd[a + "value_proj.bias"]).view(B, T, H, dh)
    pp = (pe.double() @ Pd[a + "pos_proj.weight"].t() + Pd[a + "pos_proj.bias"]).view(2 * T - 1, H, dh)
    content = torch.einsum("bihc,bkhc->bhik", q + Pd[a + "content_bias"], k)
    full = torch.einsum("bihc,jhc->bhij", q + Pd[a + "position_bias"], pp)
    idx = ((T - 1) - (torch.arange(T)[:, None] - torch.arange(T)[None, :])).expand(B, H, T, T)
    s = (content + full.gather(-1, idx)) / math.sqrt(dh)
    s = s.masked_fill((torch.arange(T)[None, :] >= L[:, None])[:, None, None, :], float("-inf"))
    att = torch.softmax(s, -1) * ma
    ctx = torch.einsum("bhik,bkhc->bihc", att, v).reshape(B, T, d)
    return (ctx @ Pd[a + "out_proj.weight"].t() + Pd[a + "out_proj.bias"]) * mo + x


def conv_ref(x, Pd, pre, m):
    """convolution.py:21-32 in training mode (batch statistics) + dropout + the residual of block.py:23."""
    return O.conv_module(x, Pd, pre, training=True) * m + x


def block_ref(x, pe, L, Pd, H, seeds):
    """block.py:17-29 with the seven masks of `seeds`, in draw order: ffn_1 (hidden, out), attention (probabilities, out),
    conv, ffn_2 (hidden, out)."""
    B, T, d = x.shape
    rows = B * T
    m = lambda n, s: rmask((rows, n), P, s).view(B, T, n)
    y = ffn_ref(x, Pd, "ffn_1.", m(4 * d, seeds[0]), m(d, seeds[1]))
    y = attention_ref(y, pe, L, Pd, "attention.", H, rmask((B, H, T, T), P, seeds[2]), m(d, seeds[3]))
    y = conv_ref(y, Pd, "conv.", m(d, seeds[4]))
    y = ffn_ref(y, Pd, "ffn_2.", m(4 * d, seeds[5]), m(d, seeds[6]))
    return O.layer_norm(y, Pd["layer_norm.weight"], Pd["layer_norm.bias"])


def drawn_seeds(ops, s, n):
    """The next n seeds after torch.manual_seed(s); leaves the generator re-seeded, so the module draws the same ones."""
    torch.manual_seed(s)
    seeds = ops.new_seeds(n)
    torch.manual_seed(s)
    return seeds


def compare(mod, y, ref, xg, xd, Pd, prec, what, own_drift=None):
    """Output, input gradient and every parameter gradient against the float64 model; under a 16-bit precision the per-tensor
    autocast bar, with reference gradients below ZERO_GRAD taken as zero (key / position biases, the depthwise bias in front
    of a train-mode BatchNorm: tests/autocast_cases.py).  own_drift: per parameter, the reference model's own autocast drift on
    this case; a parameter gradient may be as far from float64 as the reference's is (the rule of
    tests/test_autocast_golden_gpu.py).  Every figure is printed; all misses are reported together."""
    fwd, grad = (BAR16, BAR16) if prec else (TOL, TOL_GRAD)
    own_drift = own_drift or {}
    rows = [("y", rel_l2(y.float(), ref), fwd)]
    if xg is not None:
        rows.append(("dx", rel_l2(xg.grad, xd.grad), grad))
    refs = {n: Pd[n].grad for n, _ in mod.named_parameters() if n in Pd and Pd[n].grad is not None}
    scale = max(float(g.abs().max()) for g in refs.values())
    for n, p_ in mod.named_parameters():
        if n not in refs:
            assert p_.grad is None or not bool(p_.grad.any()), f"{what}: {n} has a gradient the float64 model does not give"
            continue
        gr = refs[n]
        if float(gr.norm()) < (ZERO_GRAD if prec else 1e-6):
            rows.append((n + " (zero)", float(p_.grad.abs().max()) / scale, BAR16 if prec else 1e-4))
        else:
            rows.append((n, rel_l2(p_.grad, gr), max(grad, own_drift.get(n, 0.0))))
    for name, err, bar in rows:
        print(f"{what} {name}: {err:.3e} (bar {bar:.0e})")
    bad = [(name, f"{err:.3e}", bar) for name, err, bar in rows if not err < bar]
    assert not bad, f"{what}: {bad}"


def autocast_of(prec):
    return torch.autocast("cuda", dtype=DT16[prec]) if prec else contextlib.nullcontext()


@pytest.mark.parametrize("prec", [0, 1, 2], ids=["f32"] + PREC_IDS)
def test_conv_module_with_restated_mask(ops, dev, prec):
    """ConvolutionModule in training mode: the mask of pointwise_conv_2's result, (B T, d) at row * d + col, restated."""
    from model.utils.convolution import ConvolutionModule
    d, B, T, K = 64, 3, 21, 7
    Pm = O.make_params(vocab=5, n_mel=80, n_blocks=1, d=d, n_heads=4, ksize=K, lstm_hidden=4, seed=6, with_decoder=False)
    pre = "encoder.layers.0.conv."
    mod = ConvolutionModule(d, K, dropout_rate=P)
    mod.load_state_dict({k[len(pre):]: v for k, v in Pm.items() if k.startswith(pre)})
    mod = mod.to(dev).train()
    x, w = rnd(B, T, d, seed=11), rnd(B, T, d, seed=12)
    seed, = drawn_seeds(ops, 21, 1)
    xg = x.to(dev).requires_grad_(True)
    with autocast_of(prec):
        y = mod.fused(xg, residual=xg)
    (y.float() * w.to(dev)).sum().backward()
    Pd = params64(Pm, pre)
    xd = x.double().requires_grad_(True)
    ref = conv_ref(xd, Pd, "", rmask((B * T, d), P, seed).view(B, T, d))
    (ref * w.double()).sum().backward()
    compare(mod, y, ref, xg, xd, Pd, prec, f"conv {(['f32'] + PREC_IDS)[prec]}")


@pytest.mark.parametrize("prec", [0, 1, 2], ids=["f32"] + PREC_IDS)
def test_encoder_input_projection_with_restated_mask(ops, dev, prec):
    """Encoder without blocks: stem -> input Linear (LinearFn on the re-laid-out weight) -> dropout.  The mask is (B T', d) at
    row * d + col whatever the column order of the packed weight; the gradients land in the reference's weight layout."""
    from model.modules.encoder import Encoder
    d, B, T = 64, 3, 103
    Pm = O.make_params(vocab=5, n_mel=80, n_blocks=0, d=d, n_heads=4, ksize=7, lstm_hidden=4, seed=8, with_decoder=False)
    mod = Encoder(80, 0, d, 4, 7, dropout_rate=P)
    mod.load_state_dict({k[len("encoder."):]: v for k, v in Pm.items() if k.startswith("encoder.")})
    mod = mod.to(dev).train()
    x = rnd(B, 80, T, seed=13)
    lengths = torch.tensor([103, 80, 31])
    T2 = O.subsampled_frames(T)
    w = rnd(B, T2, d, seed=14)
    seed, = drawn_seeds(ops, 22, 1)
    with autocast_of(prec):
        y, out_len = mod(x.to(dev), lengths.to(dev))
    (y.float() * w.to(dev)).sum().backward()
    assert y.shape == (B, T2, d) and torch.equal(out_len.cpu(), O.subsampled_lengths(lengths))
    mask = rmask((B * T2, d), P, seed).view(B, T2, d)

    def model(Pq, dtype, auto):
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=auto):
            h = O.conv_subsampling(x.to(dtype), Pq, "downsampling_conv.")
            out = (h @ Pq["linear.weight"].t() + Pq["linear.bias"]) * mask.to(dtype)
        (out.to(dtype) * w.to(dtype)).sum().backward()
        return out

    Pd = params64(Pm, "encoder.")
    ref = model(Pd, torch.float64, False)
    own = None
    if prec:
        # The stem's parameter gradients pass two ReLU gates taken from 16-bit products and travel as 16-bit tensors: the
        # reference model's own bf16 autocast (the fp32 oracle under torch.autocast on the host, same mask) is 6e-2 from float64
        # on them.  That drift is their bar in both 16-bit types (fp16 carries three more bits than bf16; the reference's fp16
        # autocast without a loss scale underflows on the host and gives no figure).
        Pa = {k: v.detach().float().requires_grad_(True) for k, v in Pd.items() if torch.is_tensor(v) and v.is_floating_point()}
        model(Pa, torch.float32, True)
        own = {n: rel_l2(Pa[n].grad, Pd[n].grad) for n in Pa if n.startswith("downsampling_conv.") and Pa[n].grad is not None}
    compare(mod, y, ref, None, None, Pd, prec, f"encoder projection {(['f32'] + PREC_IDS)[prec]}", own_drift=own)


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
def test_ffn_and_attention_modules_under_autocast(ops, dev, prec):
    """The two sites tests/test_dropout_gpu.py holds in fp32, under autocast with the masks restated."""
    from model.utils.attention import MultiHeadSelfAttentionModule
    from model.utils.ffn import FeedForwardModule
    d, H, B, T = 64, 4, 2, 21
    Pm = O.make_params(vocab=5, n_mel=80, n_blocks=1, d=d, n_heads=H, ksize=7, lstm_hidden=4, seed=9, with_decoder=False)
    x, w = rnd(B, T, d, seed=15), rnd(B, T, d, seed=16)
    L = torch.tensor([T, 13])
    pe = O.relpos_table(T, Pm["encoder.rel_pe.div_term"])
    # feed-forward
    pre = "encoder.layers.0.ffn_1."
    mod = FeedForwardModule(d, dropout_rate=P)
    mod.load_state_dict({k[len(pre):]: v for k, v in Pm.items() if k.startswith(pre)})
    mod = mod.to(dev).train()
    s1, s2 = drawn_seeds(ops, 23, 2)
    xg = x.to(dev).requires_grad_(True)
    with autocast_of(prec):
        y = mod.fused(xg, residual=xg, alpha=0.5)
    (y.float() * w.to(dev)).sum().backward()
    Pd = params64(Pm, pre)
    xd = x.double().requires_grad_(True)
    ref = ffn_ref(xd, Pd, "", rmask((B * T, 4 * d), P, s1).view(B, T, 4 * d), rmask((B * T, d), P, s2).view(B, T, d))
    (ref * w.double()).sum().backward()
    compare(mod, y, ref, xg, xd, Pd, prec, f"ffn {PREC_IDS[prec - 1]}")
    # attention
    pre = "encoder.layers.0.attention."
    mod = MultiHeadSelfAttentionModule(d, H, dropout_rate=P)
    mod.load_state_dict({k[len(pre):]: v for k, v in Pm.items() if k.startswith(pre)})
    mod = mod.to(dev).train()
    s1, s2 = drawn_seeds(ops, 24, 2)
    xg = x.to(dev).requires_grad_(True)
    with autocast_of(prec):
        y = mod.fused(xg, pe.to(dev), L.to(dev), residual=xg)
    (y.float() * w.to(dev)).sum().backward()
    Pd = params64(Pm, pre)
    xd = x.double().requires_grad_(True)
    ref = attention_ref(xd, pe, L, Pd, "", H, rmask((B, H, T, T), P, s1), rmask((B * T, d), P, s2).view(B, T, d))
    (ref * w.double()).sum().backward()
    compare(mod, y, ref, xg, xd, Pd, prec, f"attention {PREC_IDS[prec - 1]}")


@pytest.mark.parametrize("prec", [0, 1, 2], ids=["f32"] + PREC_IDS)
def test_conformer_block_step_draws_seven_masks_in_order(ops, dev, prec):
    """One whole training step of a ConformerBlock (d = 64, 4 heads, T = 50, B = 2, ragged lengths) against the float64 block
    with the seven restated masks in draw order -- ffn_1 x 2, attention x 2, conv, ffn_2 x 2 --; all seven differ; a second
    step draws the next seven; re-seeding replays the first seven bit for bit."""
    from model.utils.block import ConformerBlock
    d, H, B, T, K = 64, 4, 2, 50, 7
    Pm = O.make_params(vocab=5, n_mel=80, n_blocks=1, d=d, n_heads=H, ksize=K, lstm_hidden=4, seed=10, with_decoder=False)
    pre = "encoder.layers.0."
    mod = ConformerBlock(d, H, K, dropout_rate=P)
    mod.load_state_dict({k[len(pre):]: v for k, v in Pm.items() if k.startswith(pre)})
    mod = mod.to(dev).train()
    x, w = rnd(B, T, d, seed=17), rnd(B, T, d, seed=18)
    L = torch.tensor([T, 33])
    pe = O.relpos_table(T, Pm["encoder.rel_pe.div_term"])
    seeds = drawn_seeds(ops, 25, 14)
    assert len(set(seeds)) == 14
    shapes = [(B * T, 4 * d), (B * T, d), (B, H, T, T), (B * T, d), (B * T, d), (B * T, 4 * d), (B * T, d)]
    same_shape = [1, 3, 4, 6]                                             # the four (B T, d) masks: pairwise different
    masks = [R.mask(shapes[i], P, seeds[i]) for i in same_shape]
    assert all(not np.array_equal(masks[i], masks[j]) for i in range(4) for j in range(i))
    assert not np.array_equal(R.mask(shapes[0], P, seeds[0]), R.mask(shapes[5], P, seeds[5]))

    def step(backward):
        xg = x.to(dev).requires_grad_(backward)
        with autocast_of(prec):
            y = mod.fused(xg, pe.to(dev), L.to(dev))
        if backward:
            (y.float() * w.to(dev)).sum().backward()
        return xg, y

    xg, y1 = step(True)
    Pd = params64(Pm, pre)
    xd = x.double().requires_grad_(True)
    ref = block_ref(xd, pe, L, Pd, H, seeds[:7])
    (ref * w.double()).sum().backward()
    compare(mod, y1, ref, xg, xd, Pd, prec, f"block {(['f32'] + PREC_IDS)[prec]}")
    # the second step draws the next seven
    _, y2 = step(False)
    with torch.no_grad():
        ref2 = block_ref(x.double(), pe, L, {k: v.detach() if torch.is_tensor(v) else v for k, v in Pd.items()}, H, seeds[7:])
    e2, e_wrong = rel_l2(y2.float(), ref2), rel_l2(y2.float(), ref.detach())
    print(f"block second step: {e2:.3e} against masks 8-14, {e_wrong:.3e} against masks 1-7")
    assert e2 < (BAR16 if prec else TOL) and e_wrong > 10 * (BAR16 if prec else TOL)
    # re-seeding replays the first seven
    torch.manual_seed(25)
    _, y3 = step(False)
    assert torch.equal(y3, y1)


