"""The four definitions of conformer_amd/csrc/conformer_hip3_pretrain.h restated in stock torch operators, with autograd for the
two backwards: the Gumbel quantizer (codes, gathered rows, marginal, perplexity; straight-through and perplexity gradients) and
the contrastive loss (per-frame loss, correctness; gradients into context and targets).  In float64 (the default) they are the
reference the kernels are held to; in float32, on whatever device the inputs live, they are the stock formulation whose own error
the GPU tests measure.  Only the argmax that picks a code is always taken in fp32, as the definition says: it is a discrete
choice between fp32 sums.  The *_scale functions return, per output element, the sum of the absolute values of the terms that
element is a sum of: what a rounding bound multiplies."""
import numpy as np
import torch

F64 = torch.float64


def codes_of(logits: torch.Tensor, noise) -> torch.Tensor:
    """(N,G) int64: argmax_v of the fp32 sum logits + noise, the lowest index on a tie"""
    x = logits.float() if noise is None else logits.float() + noise.float()
    return torch.from_numpy(np.argmax(x.cpu().numpy(), axis=-1).astype(np.int64)).to(logits.device)


def top_gap(logits: torch.Tensor, noise) -> float:
    """the smallest gap between the largest and second-largest fp32 logits + noise over the rows (inf for V = 1)"""
    x = logits.float() if noise is None else logits.float() + noise.float()
    if x.shape[-1] < 2:
        return float("inf")
    top = x.topk(2, dim=-1).values
    return float((top[..., 0] - top[..., 1]).min())


def marginal_of(probs: torch.Tensor, row_mask):
    """(sum over the rows that count (G,V), their number, at least 1)"""
    if row_mask is None:
        return probs.sum(0), probs.shape[0]
    keep = row_mask.bool()
    return (probs * keep[:, None, None]).sum(0), max(int(keep.sum()), 1)


def perplexity_of(probs: torch.Tensor, row_mask):
    """(perplexity, marginal sum (G,V)) of probs (N,G,V) over the rows of row_mask (N) bool, None = all"""
    total, count = marginal_of(probs, row_mask)
    m = total / count
    return torch.exp(-(m * torch.log(m + 1e-7)).sum(-1)).sum(), total


def quantize(logits, noise, codevectors, tau, row_mask=None, dtype=F64):
    """logits, noise (N,G,V), codevectors (G*V,dg).  Returns a dict: codes (N,G), out (N,G*dg) (the gathered rows, exact),
    marginal (G,V), perplexity (), and `surrogate` (N,G*dg): the straight-through expression whose autograd gradient is the
    definition's (None on the eval path).  logits and codevectors may require grad."""
    N, G, V = logits.shape
    cv = codevectors.to(dtype).view(G, V, -1)
    lg = logits.to(dtype)
    codes = codes_of(logits.detach(), None if noise is None else noise.detach())
    hard = torch.nn.functional.one_hot(codes, V).to(dtype)
    out = torch.stack([cv[g][codes[:, g]] for g in range(G)], dim=1).reshape(N, -1)
    if noise is None:
        perplexity, marginal = perplexity_of(hard, row_mask)
        surrogate = None
    else:
        y = torch.softmax((lg + noise.to(dtype)) / tau, dim=-1)
        probs = hard - y.detach() + y
        surrogate = torch.einsum("ngv,gvd->ngd", probs, cv).reshape(N, -1)
        perplexity, marginal = perplexity_of(torch.softmax(lg, dim=-1), row_mask)
    return dict(codes=codes, out=out, marginal=marginal, perplexity=perplexity, surrogate=surrogate)


def quantize_grads(logits, noise, codevectors, tau, row_mask, dout, dperplexity, dtype=F64):
    """(dlogits (N,G,V), dcodevectors (G*V,dg)) of sum(out * dout) + perplexity * dperplexity"""
    lg = logits.to(dtype).clone().requires_grad_(True)
    cv = codevectors.to(dtype).clone().requires_grad_(True)
    q = quantize(lg, noise, cv, tau, row_mask, dtype)
    loss = (q["surrogate"] * dout.to(dtype)).sum() + q["perplexity"] * float(dperplexity)
    return torch.autograd.grad(loss, (lg, cv))


def quantize_scales(logits, noise, codevectors, tau, row_mask, dout, dperplexity):
    """float64 term magnitudes: dict of dlogits (N,G,V), dcodevectors (G*V,dg), perplexity ()."""
    N, G, V = logits.shape
    lg, cv = logits.to(F64), codevectors.to(F64).view(G, V, -1)
    d = dout.to(F64).view(N, G, -1)
    y = torch.softmax((lg + noise.to(F64)) / tau, dim=-1)
    p = torch.softmax(lg, dim=-1)
    gabs = torch.einsum("ngd,gvd->ngv", d.abs(), cv.abs())
    total, count = marginal_of(p, row_mask)
    m = total / count
    eh = torch.exp(-(m * torch.log(m + 1e-7)).sum(-1))                                   # (G)
    coef = (eh[:, None] * (torch.log(m + 1e-7).abs() + m / (m + 1e-7)) / count)          # |c[g][v]|
    keep = torch.ones(N, dtype=F64) if row_mask is None else row_mask.to(F64)
    straight = y * (gabs + (y * gabs).sum(-1, keepdim=True)) / tau
    perp = abs(float(dperplexity)) * keep[:, None, None] * p * (coef[None] + (p * coef[None]).sum(-1, keepdim=True))
    codes = codes_of(logits, noise)
    dcv = torch.zeros(G, V, d.shape[-1], dtype=F64)
    for g in range(G):
        dcv[g].index_add_(0, codes[:, g], d[:, g].abs())
    perplexity = (eh[:, None] * m * (torch.log(m + 1e-7).abs() + 1)).sum()
    return dict(dlogits=straight + perp, dcodevectors=dcv.view(G * V, -1), perplexity=perplexity, marginal=total)


def _candidates(context, targets, negatives, ids, dtype):
    B, T, D = context.shape
    dev = context.device
    c, tg = context.to(dtype), targets.to(dtype)
    neg = negatives.long()
    absent = (neg < 0) | (neg >= T)
    idx = torch.cat([torch.arange(T, device=dev)[None, :, None].expand(B, T, 1), neg.clamp(0, T - 1)], dim=-1)    # (B,T,K+1)
    rows = torch.arange(B, device=dev)[:, None, None]
    cand = tg[rows, idx]                                                                                         # (B,T,K+1,D)
    excluded = torch.cat([torch.zeros(B, T, 1, dtype=torch.bool, device=dev), absent], dim=-1)
    if ids is not None:
        same = ids.long()[rows, idx] == ids.long()[:, :, None]
        same[:, :, 0] = False
        excluded = excluded | same
    return c, cand, excluded


def contrastive(context, targets, mask, negatives, ids=None, temperature=0.1, dtype=F64):
    """context, targets (B,T,D), mask (B,T) bool, negatives (B,T,K) int, ids (B,T) int or None.  Returns a dict: loss (),
    frame_loss (B,T), correct (B,T) bool, z (B,T,K+1).  context and targets may require grad."""
    c, cand, excluded = _candidates(context, targets, negatives, ids, dtype)
    dot = (c[:, :, None, :] * cand).sum(-1)
    den = (torch.linalg.vector_norm(c, dim=-1)[:, :, None] * torch.linalg.vector_norm(cand, dim=-1)).clamp_min(1e-8)
    z = (dot / den / temperature).masked_fill(excluded, -float("inf"))
    m = mask.bool()
    frame_loss = torch.where(m, torch.logsumexp(z, dim=-1) - z[..., 0], torch.zeros((), dtype=dtype, device=z.device))
    correct = (z[..., 0] >= z.max(dim=-1).values) & m
    return dict(loss=frame_loss.sum(), frame_loss=frame_loss, correct=correct, z=z)


def contrastive_grads(context, targets, mask, negatives, ids, temperature, gframe, dtype=F64):
    """(dcontext, dtargets) of sum(frame_loss * gframe)"""
    c = context.to(dtype).clone().requires_grad_(True)
    t = targets.to(dtype).clone().requires_grad_(True)
    r = contrastive(c, t, mask, negatives, ids, temperature, dtype)
    return torch.autograd.grad((r["frame_loss"] * gframe.to(dtype)).sum(), (c, t))


def contrastive_scales(context, targets, mask, negatives, ids, temperature, gframe):
    """float64 term magnitudes: dict of dcontext, dtargets (B,T,D): sum_k |w_k| (|other row| / den + |cos| |own row| / |own|^2)
    with |w_k| = |gframe| (p_k + [k = 0]) / temperature, over the terms each gradient row is a sum of."""
    B, T, D = context.shape
    c, cand, excluded = _candidates(context, targets, negatives, ids, F64)
    r = contrastive(context, targets, mask, negatives, ids, temperature)
    p = torch.softmax(r["z"], dim=-1)
    w = gframe.to(F64).abs()[:, :, None] * (p + torch.nn.functional.one_hot(torch.zeros(B, T, dtype=torch.long), p.shape[-1]))
    w = (w / temperature) * mask.to(F64)[:, :, None] * (~excluded).to(F64)                                       # (B,T,K+1)
    cn, kn = torch.linalg.vector_norm(c, dim=-1), torch.linalg.vector_norm(cand, dim=-1)
    prod = cn[:, :, None] * kn
    den = prod.clamp_min(1e-8)
    cos = (c[:, :, None, :] * cand).sum(-1).abs() / den * (prod > 1e-8)
    dctx = (w[..., None] * cand.abs() / den[..., None]).sum(2) + (w * cos).sum(2)[..., None] * c.abs() / \
        (cn * cn).clamp_min(1e-300)[..., None]
    # every (t, k) sends |w| (|context[t]| / den + |cos| |cand| / |cand|^2) to the frame it drew
    send = w[..., None] * (c.abs()[:, :, None, :] / den[..., None] + cos[..., None] * cand.abs() / (kn * kn).clamp_min(1e-300)[..., None])
    neg = negatives.long().clamp(0, T - 1)
    idx = torch.cat([torch.arange(T)[None, :, None].expand(B, T, 1), neg], dim=-1)
    dtg = torch.zeros(B, T, D, dtype=F64)
    for b in range(B):
        dtg[b].index_add_(0, idx[b].reshape(-1), send[b].reshape(-1, D))
    return dict(dcontext=dctx, dtargets=dtg)
