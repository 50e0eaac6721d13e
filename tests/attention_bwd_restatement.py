"""Float64 restatement of the backward of the relative-position attention core (`oracle.relpos_attention_core`), written out
op by op -- no autograd -- for the fused backward kernels `attention_bwd_flash_f32.hip` and `attention_bwd_flash_mfma16.hip`.
Test helper only: not collected by pytest, imported by the attention-backward tests.

    s[i,k] = ((q_i+u).k_k + (q_i+v).p_{T-1-(i-k)}) / sqrt(dh)      masked to keys k < L (L <= 0: uniform weights)
    P = softmax_k(s) ;  W = P o M ;  O = W.V                        M: weight-dropout keep mask, already scaled by 1/(1-p)
    D_i = dO_i.O_i ;  dW = dO.V^T ;  dS = P o (dW o M - D) / sqrt(dh)   (dS = 0 on a row whose utterance has L <= 0)
    dV = W^T.dO ;  dK = dS^T.(Q+u) ;  d(Q+u) = dS.K ;  dG[i, T-1-(i-k)] = dS[i,k]
    d(Q+v) = dG.Pos ;  dPos = dG^T.(Q+v) ;  dq = d(Q+u) + d(Q+v) ;  du = sum_{b,i} d(Q+u) ;  dv = sum_{b,i} d(Q+v)

Query rows at or past an utterance's length are computed like any other row.  `mode` replays the operand rounding of each
device path (every product itself stays float64):
  * "f32":       nothing is rounded;
  * "f32_prec":  the fp32 kernel run with `prec` (autocast, dh <= 16).  Q+u, Q+v, K, V, the table rows and dO are rounded to
                 `dt16` where the kernel stages them; the K of d(Q+u) = dS.K is NOT rounded; P, W and dS stay unrounded;
  * "mfma16":    the 16-bit kernel.  Q+u, Q+v, K (both uses), V, the table rows and dO are rounded, and so are W = P o M (as
                 the dV operand) and dS (as the operand of dK, d(Q+u), d(Q+v) and dPos); P itself stays unrounded.
In both rounded modes D_i = round(dO_i).O_i.  O is the forward's context: by default O = W.V computed here (with the
rounded V in the rounded modes, so that sum_k P o (dW o M - D) = 0 holds exactly); a test replaying a device backward passes
the context that the device forward produced instead, as the kernel reads it.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

MODES = ("f32", "f32_prec", "mfma16")


def band_index(T: int) -> torch.Tensor:
    """(T,T) table row j = T-1-(i-k) of the relative position of query i and key k."""
    i = torch.arange(T)[:, None]
    k = torch.arange(T)[None, :]
    return (T - 1) - (i - k)


def attention_bwd(q, k, v, pp, u, vb, lengths: Optional[torch.Tensor], dctx, mode: str = "f32", dt16=None,
                  mask: Optional[torch.Tensor] = None, o: Optional[torch.Tensor] = None):
    """q, k, v: (B,T,H,dh); pp: (2T-1,H,dh) projected table; u, vb: (H,dh); lengths: (B,) or None; dctx: (B,T,H*dh);
    mask: (B,H,T,T) scaled keep mask or None; o: the forward's context (B,T,H*dh) or None.

    Returns a dict with the layouts of `ops.relpos_attention_bwd` and the forward's log-sum-exp:
    dqkv (B,T,3d), dpos (2T-1,d), du (H,dh), dvb (H,dh), lse (B,H,T); all float64."""
    assert mode in MODES and (mode == "f32" or dt16 in (torch.bfloat16, torch.float16))
    B, T, H, dh = q.shape
    d = H * dh
    f64 = lambda t: t.detach().cpu().double()
    if mode == "f32":
        r = f64
        qu, qv = f64(q) + f64(u), f64(q) + f64(vb)
    else:
        r = lambda t: t.detach().cpu().to(dt16).double()
        f32 = lambda t: t.detach().cpu().float()
        qu, qv = r(f32(q) + f32(u)), r(f32(q) + f32(vb))            # the kernels add the biases in fp32, then round
    K, V, Pt = r(k), r(v), r(pp)
    dO = r(dctx).view(B, T, H, dh)
    Kd = f64(k) if mode == "f32_prec" else K                            # the K of d(Q+u) = dS.K
    scale = 1.0 / math.sqrt(dh)

    # ---- forward recompute: scores, masked softmax, log-sum-exp
    j = band_index(T).expand(B, H, T, T)
    content = torch.einsum("bihc,bkhc->bhik", qu, K)
    full = torch.einsum("bihc,jhc->bhij", qv, Pt)                       # (B,H,T,2T-1)
    s = (content + full.gather(-1, j)) * scale
    Lv = torch.full((B,), T, dtype=torch.int64) if lengths is None else lengths.detach().cpu().to(torch.int64)
    uniform = Lv <= 0                                                   # every key masked: uniform weights, no score gradient
    keyok = torch.arange(T)[None, :] < Lv.clamp(min=1)[:, None]         # (B,T)
    s = s.masked_fill(~keyok[:, None, None, :], -math.inf)
    s = torch.where(uniform[:, None, None, None], torch.zeros_like(s), s)
    lse = torch.logsumexp(s, dim=-1)                                    # uniform rows: log T
    P = torch.exp(s - lse[..., None])
    M = torch.ones_like(P) if mask is None else f64(mask)
    W = P * M

    # ---- backward
    if o is None:
        O = torch.einsum("bhik,bkhc->bihc", W, V)
    else:
        O = f64(o).view(B, T, H, dh)
    D = torch.einsum("bihc,bihc->bhi", dO, O)
    dW = torch.einsum("bihc,bkhc->bhik", dO, V)
    dS = P * (dW * M - D[..., None]) * scale
    dS = torch.where(uniform[:, None, None, None], torch.zeros_like(dS), dS)
    if mode == "mfma16":
        W, dS = r(W), r(dS)
    dV = torch.einsum("bhik,bihc->bkhc", W, dO)
    dK = torch.einsum("bhik,bihc->bkhc", dS, qu)
    dQu = torch.einsum("bhik,bkhc->bihc", dS, Kd)
    dG = torch.zeros(B, H, T, 2 * T - 1, dtype=torch.float64).scatter_(-1, j, dS)
    dQv = torch.einsum("bhij,jhc->bihc", dG, Pt)
    dpos = torch.einsum("bhij,bihc->jhc", dG, qv)
    dq = dQu + dQv
    return dict(dqkv=torch.cat([dq.reshape(B, T, d), dK.reshape(B, T, d), dV.reshape(B, T, d)], dim=-1),
                dpos=dpos.reshape(2 * T - 1, d), du=dQu.sum((0, 1)), dvb=dQv.sum((0, 1)), lse=lse)
