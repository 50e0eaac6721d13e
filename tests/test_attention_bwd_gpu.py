"""The fused attention backward (attention_bwd_flash_f32.hip, attention_bwd_flash_mfma16.hip) against the float64
restatement of tests/attention_bwd_restatement.py, op by op and slice by slice.

`ops.relpos_attention_train` then `ops.relpos_attention_bwd` run directly (both under one autocast for the 16-bit paths), with
a non-zero context gradient on every row, padded query rows included.  Errors are measured per (b, h) slice of dq / dk / dv,
per 32-row band of dpos and per head of du / dvb: a wrong key block, wave, band carry or query tile shows up in its own slice
instead of vanishing in one global number.  Where the backward is structurally zero (masked keys, table rows outside every
utterance's band) the kernels must write exactly 0.0.

Each path is compared with the restatement that replays its operand rounding and is fed the device forward's context (the
kernels read it for D_i = dO_i.O_i); the 16-bit paths are also held to the 16-bit budget of the forward test against the
unrounded float64 backward.  A slice whose reference norm is below 1 % of the mean slice norm of its tensor is measured against
that 1 % instead of its own norm.

The value projections carry a common offset per dimension (a value-projection bias): the context then keeps a mean component,
and D_i = dO_i.O_i is large enough that computing it from the unrounded dO would show (a designed rounding point of the 16-bit
kernel, attention_bwd_flash_mfma16.hip)."""
import contextlib
import math

import pytest
import torch

from tests.attention_bwd_restatement import attention_bwd

pytestmark = pytest.mark.gpu

BF16, FP16 = torch.bfloat16, torch.float16

# Bounds per path, each at most 4x the largest value measured on an MI355X over this file's cases (in brackets).
#   grad:   per-slice rel-L2 against the restatement that replays the path's rounding.  For the 16-bit paths it sits below the
#           distance between the rounded and the unrounded float64 backward (checked: gap > 1.5 grad), so a rounding point
#           moved or dropped cannot hide in it;
#   lse:    max |lse - ref| (its fp32 maximum comes from the sharp-softmax case);
#   inv:    the softmax shift invariances on the device result, per (b, h) |sum_k dK| / |dK| and per head |sum_j dpos| / |dpos|.
#           Under autocast D_i = round(dO_i).O_i cancels sum_k P o dW only up to the forward's rounding of P for P.V;
#   budget: per-tensor rel-L2 against the unrounded float64 backward: the 16-bit budget of test_mfma16_attention_forward.
TOL = {
    "f32":       dict(grad=1.5e-5, lse=2.5e-5, inv=1.5e-4),                  # [4.1e-6, 6.8e-6, 4.0e-5]
    "prec_bf16": dict(grad=2e-6, lse=3.5e-6, inv=1.6e-2, budget=1e-2),       # [5.9e-7, 8.5e-7, 4.1e-3]
    "prec_fp16": dict(grad=2e-6, lse=3.5e-6, inv=2.5e-3, budget=2e-3),       # [5.6e-7, 8.5e-7, 6.7e-4]
    "bf16":      dict(grad=6e-4, lse=3.5e-6, inv=2.5e-2, budget=1e-2),       # [1.9e-4, 9.0e-7, 7.2e-3]
    "fp16":      dict(grad=1.5e-4, lse=3.5e-6, inv=2.5e-3, budget=2e-3),     # [5.5e-5, 9.2e-7, 6.4e-4]
}
RESID = 7e-7        # mathematically zero score gradients (one visible key): fp32 residue relative to the dV slice norm [1.8e-7]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def make_inputs(B, T, H, dh, seed=0, sharp=False):
    d = H * dh
    qkv = rnd(B, T, 3 * d, seed=seed) * 0.5
    qkv[..., 2 * d:] += rnd(d, seed=seed + 7)                   # value-projection bias: a common offset of every key's V
    if sharp:
        qkv[..., :2 * d] *= 6.0                                 # near one-hot rows (test_relpos_attention_sharp_softmax)
    pos = rnd(2 * T - 1, d, seed=seed + 1) * 0.5
    u, v = rnd(H, dh, seed=seed + 2) * 0.3, rnd(H, dh, seed=seed + 3) * 0.3
    dctx = rnd(B, T, d, seed=seed + 4)
    return dict(qkv=qkv, pos=pos, u=u, v=v, dctx=dctx, B=B, T=T, H=H, dh=dh)


def path_of(amp, dh):
    if amp is None:
        return "f32"
    name = "bf16" if amp == BF16 else "fp16"
    return "prec_" + name if dh <= 16 else name                # ops sends dh <= 16 to the fp32 kernel with `prec`


def run_device(dev, x, L, amp=None, drop_p=0.0, seed=0, direct16=None):
    """ctx, lse, dqkv, dpos, du, dvb on the CPU.  direct16: call the 16-bit kernel's C entry with that precision code instead of
    ops.relpos_attention_bwd (which never sends it heads of <= 16 dims); the forward then runs under ops.precision."""
    from conformer_amd import ops, _lib
    G = lambda t: t.to(dev)
    qkv, pos, u, v, dctx = G(x["qkv"]), G(x["pos"]), G(x["u"]), G(x["v"]), G(x["dctx"])
    Lg = None if L is None else G(L)
    H = x["H"]
    if direct16 is not None:
        with ops.precision(direct16):
            ctx, lse = ops.relpos_attention_train(qkv, pos, u, v, Lg, H, drop_p, seed)
        B, T, d3 = qkv.shape
        d, dh = d3 // 3, d3 // 3 // H
        dqkv = torch.zeros(B, T, d3, device=dev)
        dpos = torch.zeros(2 * T - 1, d, device=dev)
        du, dvb = torch.zeros(H, dh, device=dev), torch.zeros(H, dh, device=dev)
        base, dbase = qkv.data_ptr(), dqkv.data_ptr()
        st = _lib.load().cfm_relpos_attention_bwd_mfma16_f32(
            direct16, base, base + 4 * d, base + 8 * d, d3, pos.data_ptr(), pos.stride(0), u.data_ptr(), v.data_ptr(),
            None if Lg is None else Lg.data_ptr(), ctx.data_ptr(), dctx.data_ptr(), d, lse.data_ptr(), dbase, dbase + 4 * d,
            dbase + 8 * d, d3, dpos.data_ptr(), d, du.data_ptr(), dvb.data_ptr(), B, T, H, dh, float(drop_p), int(seed),
            torch.cuda.current_stream().cuda_stream)
        _lib.check(st, "cfm_relpos_attention_bwd_mfma16_f32")
    else:
        with (torch.autocast("cuda", dtype=amp) if amp is not None else contextlib.nullcontext()):
            ctx, lse = ops.relpos_attention_train(qkv, pos, u, v, Lg, H, drop_p, seed)
            dqkv, dpos, du, dvb = ops.relpos_attention_bwd(qkv, pos, u, v, Lg, H, ctx, lse, dctx, drop_p, seed)
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in dict(ctx=ctx, lse=lse, dqkv=dqkv, dpos=dpos, du=du, dvb=dvb).items()}


def dropout_mask(dev, B, H, T, p, seed):
    """The weight-dropout keep mask of the attention kernels (flat index ((b*H + h)*T + i)*T + k), scaled by 1/(1-p)."""
    from conformer_amd import ops
    return ops.dropout_apply(torch.ones(B, H, T, T, device=dev), p, seed).cpu().double()


def restate(x, L, mode="f32", dt16=None, mask=None, o=None):
    B, T, H, dh = x["B"], x["T"], x["H"], x["dh"]
    d = H * dh
    q, k, v = (t.reshape(B, T, H, dh) for t in x["qkv"].split(d, dim=-1))
    return attention_bwd(q, k, v, x["pos"].view(2 * T - 1, H, dh), x["u"], x["v"], L, x["dctx"], mode, dt16, mask=mask, o=o)


def live_utterances(x, L):
    """(B,) bool: utterances with at least two visible keys.  With one visible key (T = 1 or L = 1) P = 1 and the score gradient
    P o (dW - D) is zero in exact arithmetic, so dq, dk, dpos, du and dvb are mathematically zero; with none (L <= 0) the
    kernels skip the score gradient and write exact zeros (structural_zero_violations)."""
    B, T = x["B"], x["T"]
    n = torch.full((B,), T) if L is None else L.clamp(max=T)
    return n >= 2


def _slice_rel(err, ref):
    """err, ref: per-slice norms -> per-slice relative errors (tiny slices against 1 % of the mean slice norm)."""
    floor = 1e-2 * float(ref.mean()) if ref.numel() else 0.0
    return err / torch.clamp(ref, min=max(floor, 1e-300))


def slice_errors(out, ref, x, live):
    """Max per-slice rel-L2 of dq, dk, dv ((b, h) slices), dpos (32-row bands), du, dvb (heads), over the live utterances; and
    `resid`: where the score gradient is zero in exact arithmetic (utterances with one visible key), the norm of what the
    kernel wrote there (fp32 cancellation in dW - D) relative to the mean (b, h) slice norm of dV."""
    B, T, H, dh = x["B"], x["T"], x["H"], x["dh"]
    o3 = out["dqkv"].double().view(B, T, 3, H, dh)
    r3 = ref["dqkv"].view(B, T, 3, H, dh)
    scale = float(r3[:, :, 2].norm(dim=(1, 3)).mean())
    res, resid = {}, 0.0
    for s, name in enumerate(("dq", "dk", "dv")):
        keep = torch.ones(B, dtype=torch.bool) if name == "dv" else live
        if keep.any():
            e = (o3[keep][:, :, s] - r3[keep][:, :, s]).norm(dim=(1, 3))       # (b, h)
            res[name] = float(_slice_rel(e, r3[keep][:, :, s].norm(dim=(1, 3))).max())
        if not keep.all():
            resid = max(resid, float(o3[~keep][:, :, s].norm(dim=(1, 3)).max()) / scale)
    P = 2 * T - 1
    nb = (P + 31) // 32
    pad = lambda t: torch.cat([t, torch.zeros(nb * 32 - P, t.shape[1], dtype=t.dtype)]).view(nb, -1)
    od, rd = pad(out["dpos"].double()), pad(ref["dpos"])
    if live.any():
        res["dpos"] = float(_slice_rel((od - rd).norm(dim=1), rd.norm(dim=1)).max())
        for name in ("du", "dvb"):
            res[name] = float(_slice_rel((out[name].double() - ref[name]).norm(dim=1), ref[name].norm(dim=1)).max())
    else:
        resid = max([resid, float(od.norm(dim=1).max()) / scale] + [float(out[n].double().norm(dim=1).max()) / scale
                                                                     for n in ("du", "dvb")])
    return res, resid


def tensor_errors(out, ref, x, live):
    """Per-tensor rel-L2 of dq, dk (live utterances), dv, dpos, du, dvb (if any utterance is live)."""
    d = x["H"] * x["dh"]
    res = {}
    for s, name in enumerate(("dq", "dk", "dv")):
        keep = torch.ones(x["B"], dtype=torch.bool) if name == "dv" else live
        if keep.any():
            a, b = out["dqkv"][keep][..., s * d:(s + 1) * d].double(), ref["dqkv"][keep][..., s * d:(s + 1) * d]
            res[name] = float((a - b).norm() / max(float(b.norm()), 1e-300))
    if live.any():
        for name in ("dpos", "du", "dvb"):
            res[name] = float((out[name].double() - ref[name]).norm() / max(float(ref[name].norm()), 1e-300))
    return res


def structural_zero_violations(out, x, L):
    """Names of outputs that are not exactly 0.0 where the backward is structurally zero."""
    B, T, H, dh = x["B"], x["T"], x["H"], x["dh"]
    d = H * dh
    bad = []
    Ls = [T] * B if L is None else [int(n) for n in L]
    for b, n in enumerate(Ls):
        if n <= 0:                                                # uniform weights: no score gradient anywhere
            if (out["dqkv"][b, :, :2 * d] != 0).any():
                bad.append(f"dq/dk of b={b} (L=0)")
        elif n < T and (out["dqkv"][b, n:, d:] != 0).any():
            bad.append(f"dk/dv of masked keys b={b}")
    vis = [min(n, T) for n in Ls if n > 0]
    first = T - 1 + max(vis) if vis else 0                        # table rows j >= T-1+L are outside utterance b's band
    if (out["dpos"][first:] != 0).any():
        bad.append(f"dpos rows >= {first}")
    return bad


def invariants(out, x, live):
    """The two softmax shift invariances on a device result, over the live utterances: max over (b, h) of |sum_k dK| / |dK|
    (the zero key_proj.bias gradient) and max over h of |sum_j dpos| / |dpos| (the zero pos_proj.bias gradient)."""
    B, T, H, dh = x["B"], x["T"], x["H"], x["dh"]
    d = H * dh
    if not live.any():
        return 0.0, 0.0
    dK = out["dqkv"][live][..., d:2 * d].double().reshape(-1, T, H, dh)
    ik = float((dK.sum(1).norm(dim=-1) / dK.norm(dim=(1, 3))).max())
    dp = out["dpos"].double().view(2 * T - 1, H, dh)
    ip = float((dp.sum(0).norm(dim=-1) / dp.norm(dim=(0, 2))).max())
    return ik, ip


def lse_error(out, ref, L, T):
    err = float((out["lse"].double() - ref["lse"]).abs().max())
    if L is not None:
        for b, n in enumerate(L.tolist()):
            if n <= 0:
                err = max(err, float((out["lse"][b].double() - math.log(T)).abs().max()))
    return err


def measure(dev, B, T, H, dh, lengths, amp=None, drop_p=0.0, sharp=False, direct16=None, seed=0):
    """Every error metric of one case: dict(path, grad (per-slice maxima), resid, lse, inv (dK, dpos), zeros (violations),
    budget / gap (16-bit: per-tensor rel-L2 to the unrounded backward, and that of the rounded restatement))."""
    x = make_inputs(B, T, H, dh, seed=seed + T + dh, sharp=sharp)
    L = None if lengths is None else torch.tensor(lengths, dtype=torch.int64)
    live = live_utterances(x, L)
    dseed = 1234 + T
    out = run_device(dev, x, L, amp, drop_p, dseed, direct16)
    M = dropout_mask(dev, B, H, T, drop_p, dseed) if drop_p > 0 else None
    if direct16 is not None:
        amp = BF16 if direct16 == 1 else FP16
        path, mode = ("bf16" if amp == BF16 else "fp16"), "mfma16"
    else:
        path = path_of(amp, dh)
        mode = "f32" if amp is None else ("f32_prec" if dh <= 16 else "mfma16")
    ref = restate(x, L, mode, amp, M, o=out["ctx"])
    grad, resid = slice_errors(out, ref, x, live)
    res = dict(path=path, grad=grad, resid=resid, lse=lse_error(out, ref, L, T), inv=invariants(out, x, live),
               zeros=structural_zero_violations(out, x, L))
    if amp is not None:
        exact = restate(x, L, "f32", None, M)
        res["budget"] = tensor_errors(out, exact, x, live)
        res["gap"] = tensor_errors(ref, exact, x, live)
    return res


def check(res):
    tol = TOL[res["path"]]
    assert not res["zeros"], res["zeros"]
    for name, e in res["grad"].items():
        assert e < tol["grad"], (name, res["grad"])
    assert res["resid"] < RESID, res["resid"]
    assert res["lse"] < tol["lse"], res["lse"]
    assert max(res["inv"]) < tol["inv"], res["inv"]
    if "budget" in res:
        for name, e in res["budget"].items():
            assert e < tol["budget"], (name, res["budget"])
        for name, e in res["gap"].items():
            assert e > 1.5 * tol["grad"], (name, res["gap"])


F32_CASES = [  # B, T, H, dh, lengths
    (1, 1, 1, 4, None),                 # smallest, <1,1>
    (2, 33, 4, 12, [33, 32]),           # query-tile edge, <2,1>
    (3, 128, 2, 16, [128, 127, 1]),     # exactly one key block
    (2, 129, 2, 20, [129, 64]),         # second key block, fully masked for b=1
    (2, 161, 2, 32, [161, 97]),         # the 160-row table ring wraps, <4,1>
    (2, 249, 8, 64, [249, 131]),        # the training shape, <8,2>
    (2, 257, 4, 36, [257, 0]),          # three key blocks, a uniform utterance, <5,2>
    (1, 300, 2, 40, None),              # top of <5,2>
    (2, 200, 2, 44, [200, 150]),        # <8,2> with masked head dims
    (1, 1000, 2, 64, [1000]),           # long band: 8 key blocks, 1999 dpos rows
]


@pytest.mark.parametrize("B,T,H,dh,lengths", F32_CASES)
def test_f32_backward(dev, B, T, H, dh, lengths):
    check(measure(dev, B, T, H, dh, lengths))


def test_f32_backward_sharp_softmax(dev):
    """Near one-hot rows: P recomputed from the forward's log-sum-exp must still be right."""
    check(measure(dev, 1, 200, 2, 64, None, sharp=True))


@pytest.mark.parametrize("B,T,H,dh,lengths,drop_p", [(2, 249, 8, 64, [249, 131], 0.1), (2, 129, 2, 20, [129, 64], 0.25)])
def test_f32_backward_dropout(dev, B, T, H, dh, lengths, drop_p):
    """Weight dropout: every key block must draw the forward's mask elements (dV from P o M, dS from P o (dW o M - D))."""
    check(measure(dev, B, T, H, dh, lengths, drop_p=drop_p))


AMP_CASES = [  # B, T, H, dh, lengths, drop_p
    (1, 1, 1, 8, None, 0.0),            # fp32 kernel with prec
    (2, 33, 2, 16, [33, 0], 0.0),       # fp32 kernel with prec
    (2, 300, 1, 8, [300, 211], 0.0),    # fp32 kernel with prec, three key blocks
    (2, 129, 2, 20, [129, 64], 0.0),    # relpos_attn_bwd16_kernel<2,1>
    (2, 249, 2, 32, [249, 0], 0.0),     # <2,1>, a uniform utterance
    (2, 129, 2, 36, [129, 100], 0.25),  # <3,2>, dropout
    (1, 300, 2, 48, None, 0.0),         # <3,2>
    (2, 249, 4, 64, [249, 131], 0.0),   # <4,2>, the training shape
]


@pytest.mark.parametrize("amp", [BF16, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,T,H,dh,lengths,drop_p", AMP_CASES)
def test_autocast_backward(dev, B, T, H, dh, lengths, drop_p, amp):
    check(measure(dev, B, T, H, dh, lengths, amp=amp, drop_p=drop_p))


@pytest.mark.parametrize("dh", [8, 16])
def test_mfma16_kernel_small_heads_direct(dev, dh):
    """relpos_attn_bwd16_kernel<1,1> (dh <= 16) is reachable only through the C entry: ops keeps such heads on the fp32
    kernel.  It must still compute the 16-bit backward it is declared to compute."""
    check(measure(dev, 2, 129, 2, dh, [129, 70], direct16=1))


@pytest.mark.parametrize("amp", [None, BF16], ids=["f32", "bf16"])
def test_backward_run_to_run(dev, amp):
    """dk / dv are written by one wave each, without atomics: bitwise reproducible.  dq, dpos, du and dvb are fp32 atomic sums
    over key blocks / waves: equal up to the order of the additions."""
    B, T, H, dh = 2, 249, 8, 64
    x = make_inputs(B, T, H, dh, seed=3)
    L = torch.tensor([249, 131])
    a, b = run_device(dev, x, L, amp, 0.1, 77), run_device(dev, x, L, amp, 0.1, 77)
    d = H * dh
    assert torch.equal(a["dqkv"][..., d:], b["dqkv"][..., d:])
    assert torch.equal(a["ctx"], b["ctx"]) and torch.equal(a["lse"], b["lse"])
    for name, s in (("dq", a["dqkv"][..., :d]), ("dpos", a["dpos"]), ("du", a["du"]), ("dvb", a["dvb"])):
        t = b["dqkv"][..., :d] if name == "dq" else b[name]
        assert float((s - t).double().norm() / t.double().norm()) <= 1e-6, name


def test_strided_pos_matches_contiguous(dev):
    """Training passes a column slice of the stacked table (row stride L*d): same results as a contiguous copy."""
    from conformer_amd import ops
    B, T, H, dh = 2, 70, 2, 32
    d = H * dh
    x = make_inputs(B, T, H, dh, seed=5)
    wide = rnd(2 * T - 1, 3 * d, seed=9).to(dev)
    wide[:, d:2 * d] = x["pos"].to(dev)
    strided = wide[:, d:2 * d]
    assert strided.stride() == (3 * d, 1)
    G = lambda t: t.to(dev)
    L = G(torch.tensor([70, 41]))
    outs = []
    for pos in (strided, strided.contiguous()):
        ctx, lse = ops.relpos_attention_train(G(x["qkv"]), pos, G(x["u"]), G(x["v"]), L, H)
        outs.append((ctx, lse) + tuple(ops.relpos_attention_bwd(G(x["qkv"]), pos, G(x["u"]), G(x["v"]), L, H, ctx, lse,
                                                                 G(x["dctx"]))))
    (c0, l0, g0, p0, u0, v0), (c1, l1, g1, p1, u1, v1) = outs
    assert torch.equal(c0, c1) and torch.equal(l0, l1) and torch.equal(g0[..., d:], g1[..., d:])
    for s, t in ((g0[..., :d], g1[..., :d]), (p0, p1), (u0, u1), (v0, v1)):
        assert float((s - t).double().norm() / t.double().norm()) <= 1e-6


def test_training_wrappers_refuse_bad_arguments(dev):
    """Every refusal happens in the wrapper, before a kernel is launched on a pointer it cannot read."""
    from conformer_amd import ops, _lib
    B, T, H, dh = 2, 9, 2, 8
    d = H * dh
    G = lambda t: t.to(dev)
    x = make_inputs(B, T, H, dh, seed=1)
    qkv, pos, u, v, dctx = G(x["qkv"]), G(x["pos"]), G(x["u"]), G(x["v"]), G(x["dctx"])
    L = G(torch.tensor([9, 5]))
    ctx, lse = ops.relpos_attention_train(qkv, pos, u, v, L, H)
    torch.cuda.synchronize()
    bad_pos = [pos.to(torch.bfloat16), pos[:-1], pos.reshape(-1), pos.t().contiguous().t(),
               torch.zeros(2 * T - 1, 2 * d, device=dev)[:, ::2], pos.cpu()]
    for p in bad_pos:
        with pytest.raises(_lib.ConformerHipError):
            ops.relpos_attention_train(qkv, p, u, v, L, H)
    bad_len = [L.cpu(), L.to(torch.int32), L.double(), L[:1]]
    for n in bad_len:
        with pytest.raises(_lib.ConformerHipError):
            ops.relpos_attention_train(qkv, pos, u, v, n, H)
        with pytest.raises(_lib.ConformerHipError):
            ops.relpos_attention_bwd(qkv, pos, u, v, n, H, ctx, lse, dctx)
    for args in ((pos[:-1], ctx, lse, dctx), (pos.reshape(-1), ctx, lse, dctx), (pos, ctx[:, :-1], lse, dctx),
                 (pos, ctx, lse[:, :1], dctx), (pos, ctx, lse, dctx[:1]), (pos, ctx, lse, dctx[..., :-4])):
        with pytest.raises(_lib.ConformerHipError):
            ops.relpos_attention_bwd(qkv, args[0], u, v, L, H, args[1], args[2], args[3])
    torch.cuda.synchronize()
