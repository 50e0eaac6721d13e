"""Float64 restatement of bounded-history streaming (the windowed prefix rule of conformer_amd/streaming.py), for the tests.

Query frame i of a chunk that ends at frame e attends to the keys max(0, i - left) <= j < e.  The attention core below works
row by row and reads ONLY the keys inside the window and the table rows chosen by r = i - j: no masked score exists, so it
cannot share a masking mistake with a kernel.  Everything around it is the oracle's (oracle/conformer_oracle.py)."""
import math

import torch

from oracle import conformer_oracle as O


def visible_ends(chunk_ends, T):
    ends = [int(e) for e in chunk_ends]
    if ends[-1] != T or any(b <= a for a, b in zip(ends, ends[1:])):
        raise ValueError(f"chunk_ends must increase and finish at T'={T}")
    ve = torch.empty(T, dtype=torch.long)
    start = 0
    for e in ends:
        ve[start:e] = e
        start = e
    return ve


def window_attention_core(q, k, v, pp, u, vb, visible_end, left, q_pos=None):
    """q (B,Tq,H,dh): the queries at absolute frames q_pos (default 0 .. Tq-1); k, v (B,T,H,dh): the keys at frames 0 .. T-1;
    pp (2P-1,H,dh): projected table, row P-1-r for relative position r; visible_end (Tq): the chunk end of every query.
    Returns (B,Tq,H*dh), float64."""
    q, k, v, pp, u, vb = (t.double() for t in (q, k, v, pp, u, vb))
    B, Tq, H, dh = q.shape
    P = (pp.shape[0] + 1) // 2
    out = torch.zeros(B, Tq, H, dh, dtype=torch.float64)
    for n in range(Tq):
        i = n if q_pos is None else int(q_pos[n])
        lo, hi = max(0, i - int(left)), int(visible_end[n])
        rows = torch.tensor([P - 1 - (i - j) for j in range(lo, hi)])
        s = torch.einsum("bhc,bkhc->bhk", q[:, n] + u, k[:, lo:hi]) + torch.einsum("bhc,khc->bhk", q[:, n] + vb, pp[rows])
        a = torch.softmax(s / math.sqrt(dh), dim=-1)
        out[:, n] = torch.einsum("bhk,bkhc->bhc", a, v[:, lo:hi])
    return out.reshape(B, Tq, H * dh)


def mhsa_module_windowed(x, pe, p, pre, n_heads, visible_end, left):
    """oracle.mhsa_module with the windowed core (x float64)."""
    B, T, d = x.shape
    dh = d // n_heads
    a = pre + "attention."
    xn = O.layer_norm(x, p[pre + "layer_norm.weight"], p[pre + "layer_norm.bias"])
    q = (xn @ p[a + "query_proj.weight"].t() + p[a + "query_proj.bias"]).view(B, T, n_heads, dh)
    k = (xn @ p[a + "key_proj.weight"].t() + p[a + "key_proj.bias"]).view(B, T, n_heads, dh)
    v = (xn @ p[a + "value_proj.weight"].t() + p[a + "value_proj.bias"]).view(B, T, n_heads, dh)
    pp = (pe @ p[a + "pos_proj.weight"].t() + p[a + "pos_proj.bias"]).view(pe.shape[0], n_heads, dh)
    ctx = window_attention_core(q, k, v, pp, p[a + "content_bias"], p[a + "position_bias"], visible_end, left).to(x.dtype)
    return ctx @ p[a + "out_proj.weight"].t() + p[a + "out_proj.bias"]


def encoder_forward_windowed(x, p, n_blocks, n_heads, chunk_ends, left, pre="encoder."):
    """oracle.encoder_forward_chunked with the attention of every block bounded to `left` frames of history; the depthwise
    convolution, the stem and the rest follow the prefix rule unchanged.  x, p: float64."""
    h = O.conv_subsampling(x, p, pre + "downsampling_conv.")
    h = h @ p[pre + "linear.weight"].t() + p[pre + "linear.bias"]
    T = h.shape[1]
    ve = visible_ends(chunk_ends, T)
    pe = O.relpos_table(T, p[pre + "rel_pe.div_term"])
    for li in range(n_blocks):
        b = f"{pre}layers.{li}."
        y = 0.5 * O.ffn_module(h, p, b + "ffn_1.") + h
        y = mhsa_module_windowed(y, pe, p, b + "attention.", n_heads, ve, left) + y
        y = O.conv_module(y, p, b + "conv.", visible_end=ve) + y
        y = 0.5 * O.ffn_module(y, p, b + "ffn_2.") + y
        h = O.layer_norm(y, p[b + "layer_norm.weight"], p[b + "layer_norm.bias"])
    return h
