"""CPU checks of the float64 attention-backward restatement (tests/attention_bwd_restatement.py): it equals torch autograd
through the oracle's attention core, keeps the two softmax shift invariances, and is exactly zero where the backward is
structurally zero.  The GPU kernels are checked against it in tests/test_attention_bwd_gpu.py."""
import math

import pytest
import torch

from oracle import conformer_oracle as O
from tests.attention_bwd_restatement import attention_bwd, band_index


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def inputs(B, T, H, dh, seed=0):
    q, k, v = rnd(B, T, H, dh, seed=seed) * 0.7, rnd(B, T, H, dh, seed=seed + 1) * 0.7, rnd(B, T, H, dh, seed=seed + 2)
    pp = rnd(2 * T - 1, H, dh, seed=seed + 3) * 0.7
    u, vb = rnd(H, dh, seed=seed + 4) * 0.3, rnd(H, dh, seed=seed + 5) * 0.3
    dctx = rnd(B, T, H * dh, seed=seed + 6)
    return q, k, v, pp, u, vb, dctx


def keep_mask(B, H, T, p, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, H, T, T, generator=g, dtype=torch.float64) >= p).double() / (1.0 - p)


def masked_core(q, k, v, pp, u, vb, lengths, M):
    """relpos_attention_core with the weight-dropout keep mask applied after the softmax (attention.py:67)."""
    B, T, H, dh = q.shape
    content = torch.einsum("bihc,bkhc->bhik", q + u, k)
    full = torch.einsum("bihc,jhc->bhij", q + vb, pp)
    s = (content + full.gather(-1, band_index(T).expand(B, H, T, T))) / math.sqrt(dh)
    if lengths is not None:
        pad = torch.arange(T)[None, :] >= lengths[:, None]
        s = s.masked_fill(pad[:, None, None, :], torch.finfo(s.dtype).min)
    a = torch.softmax(s, dim=-1) * M
    return torch.einsum("bhik,bkhc->bihc", a, v).reshape(B, T, H * dh)


def autograd_bwd(q, k, v, pp, u, vb, lengths, dctx, M=None):
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v, pp, u, vb)]
    if M is None:
        out = O.relpos_attention_core(*leaves, lengths)
    else:
        out = masked_core(*leaves, lengths, M)
    (out * dctx).sum().backward()
    gq, gk, gv, gp, gu, gvb = (t.grad for t in leaves)
    B, T, H, dh = q.shape
    d = H * dh
    return dict(dqkv=torch.cat([gq.reshape(B, T, d), gk.reshape(B, T, d), gv.reshape(B, T, d)], dim=-1),
                dpos=gp.reshape(2 * T - 1, d), du=gu, dvb=gvb)


def rel(a, b):
    den = float(b.norm())
    return float((a - b).norm()) / (den if den > 0 else 1.0)


CASES = [  # B, T, H, dh, lengths, drop_p
    (1, 1, 1, 4, None, 0.0),
    (2, 7, 2, 4, None, 0.0),
    (3, 9, 2, 8, [9, 4, 0], 0.0),
    (2, 40, 1, 12, [40, 1], 0.0),
    (2, 33, 2, 8, [33, 0], 0.0),
    (2, 9, 2, 4, [9, 5], 0.25),
    (2, 12, 1, 8, [12, 0], 0.1),
]


@pytest.mark.parametrize("B,T,H,dh,lengths,drop_p", CASES)
def test_f32_restatement_equals_autograd(B, T, H, dh, lengths, drop_p):
    q, k, v, pp, u, vb, dctx = inputs(B, T, H, dh, seed=T)
    L = None if lengths is None else torch.tensor(lengths, dtype=torch.int64)
    M = keep_mask(B, H, T, drop_p, seed=T) if drop_p > 0 else None
    got = attention_bwd(q, k, v, pp, u, vb, L, dctx, mask=M)
    ref = autograd_bwd(q, k, v, pp, u, vb, L, dctx, M)
    for name in ("dqkv", "dpos", "du", "dvb"):
        assert rel(got[name], ref[name]) < 1e-12, name
    # the log-sum-exp: log T where every key is masked, otherwise that of the scaled scores over the visible keys
    content = torch.einsum("bihc,bkhc->bhik", q + u, k)
    full = torch.einsum("bihc,jhc->bhij", q + vb, pp)
    s = (content + full.gather(-1, band_index(T).expand(B, H, T, T))) / math.sqrt(dh)
    for b in range(B):
        n = T if L is None else int(L[b])
        want = torch.full((H, T), math.log(T), dtype=torch.float64) if n <= 0 else torch.logsumexp(s[b, :, :, :n], -1)
        assert torch.allclose(got["lse"][b], want, rtol=0, atol=1e-12)


def test_context_argument_is_the_forward_context():
    """Passing the forward's context W.V explicitly gives the same backward as letting the restatement form it."""
    B, T, H, dh = 2, 11, 2, 8
    q, k, v, pp, u, vb, dctx = inputs(B, T, H, dh, seed=5)
    L = torch.tensor([11, 6])
    M = keep_mask(B, H, T, 0.2, seed=3)
    ctx = masked_core(q, k, v, pp, u, vb, L, M)
    a = attention_bwd(q, k, v, pp, u, vb, L, dctx, mask=M)
    b = attention_bwd(q, k, v, pp, u, vb, L, dctx, mask=M, o=ctx)
    for name in ("dqkv", "dpos", "du", "dvb"):
        assert rel(b[name], a[name]) < 1e-12, name


@pytest.mark.parametrize("mode,dt16", [("f32", None), ("f32_prec", torch.bfloat16), ("f32_prec", torch.float16)])
@pytest.mark.parametrize("drop_p", [0.0, 0.2])
def test_shift_invariances(mode, dt16, drop_p):
    """Softmax is invariant to a per-row shift of the scores, so the key-projection bias (a shift of k_k along q_i+u) and the
    position-projection bias get zero gradient: sum_k dK[b,k,h] = 0 and sum_j dpos[j,h] = 0 -- with dropout too, because
    D_i = sum_k P o M o dW.  (The rounded "mfma16" mode rounds dS itself: there the sums are only zero to its rounding.)"""
    B, T, H, dh = 3, 37, 2, 8
    q, k, v, pp, u, vb, dctx = inputs(B, T, H, dh, seed=9)
    L = torch.tensor([37, 20, 0])
    M = keep_mask(B, H, T, drop_p, seed=4) if drop_p > 0 else None
    g = attention_bwd(q.float(), k.float(), v.float(), pp.float(), u.float(), vb.float(), L, dctx.float(), mode, dt16, mask=M)
    dK = g["dqkv"][..., H * dh:2 * H * dh].reshape(B, T, H, dh)
    dpos = g["dpos"].reshape(2 * T - 1, H, dh)
    assert float(dK.sum(1).norm()) <= 1e-12 * float(dK.norm())
    assert float(dpos.sum(0).norm()) <= 1e-12 * float(dpos.norm())


@pytest.mark.parametrize("mode,dt16", [("f32", None), ("f32_prec", torch.bfloat16), ("mfma16", torch.bfloat16),
                                       ("mfma16", torch.float16)])
def test_structural_zeros(mode, dt16):
    """Keys masked by `lengths` get exactly zero dK and dV (L = 0 excepted: uniform weights reach every key's dV), an
    L = 0 utterance gets zero dK everywhere, and the table rows j >= T + L - 1 of a single utterance get exactly zero dpos."""
    B, T, H, dh = 3, 40, 2, 8
    q, k, v, pp, u, vb, dctx = inputs(B, T, H, dh, seed=2)
    f = lambda t: t.float()
    L = torch.tensor([40, 13, 0])
    g = attention_bwd(f(q), f(k), f(v), f(pp), f(u), f(vb), L, f(dctx), mode, dt16, mask=keep_mask(B, H, T, 0.1, seed=1))
    d = H * dh
    dK, dV = g["dqkv"][..., d:2 * d], g["dqkv"][..., 2 * d:]
    assert (dK[1, 13:] == 0).all() and (dV[1, 13:] == 0).all()
    assert (dK[1, :13] != 0).any(dim=-1).all() and (dV[1, :13] != 0).any(dim=-1).all()
    assert (dK[2] == 0).all() and (dV[2] != 0).any(dim=-1).all()
    for n in (13, 1, T):
        one = attention_bwd(f(q[:1]), f(k[:1]), f(v[:1]), f(pp), f(u), f(vb), torch.tensor([n]), f(dctx[:1]), mode, dt16)
        assert (one["dpos"][T + n - 1:] == 0).all()
        if n > 1:                                   # (one visible key: P = 1 and dS = P o (dW - D) = 0 everywhere)
            assert (one["dpos"][:T + n - 1] != 0).any(dim=-1).all()
