"""Float64 restatement, torch on the CPU, of the n-best CTC scores and of the MWER risk (INTEGRATION.md "MWER training and n-best
scores").  Per hypothesis the log-likelihood and its gradient come from oracle.ctc_lattice, ONE row at a time (B = 1, so the
oracle's own mean over the batch is the identity); `ll_ctc_loss` is the cross-check through F.ctc_loss in double.  The risk is
written with plain torch ops so that autograd gives its weights.  Nothing here is shared with the kernels."""
import math

import torch
import torch.nn.functional as F

from oracle import conformer_oracle as O


def row_ll_and_grad(logits_b, labels, Tb, blank):
    """(ll, d ll / d logits (T,V)) of one label list against the first Tb frames of logits_b (T,V); ll = -inf (and a zero
    gradient) without an alignment"""
    L = len(labels)
    tg = torch.tensor([list(labels) + [0] * (1 if L == 0 else 0)], dtype=torch.int64)
    _, nll, grad = O.ctc_lattice(logits_b[None].double(), tg, [Tb], [L], blank)
    ll = -float(nll[0])
    if not math.isfinite(ll):
        return -math.inf, torch.zeros_like(logits_b, dtype=torch.float64)
    return ll, -grad[0] * max(L, 1)


def scores(logits, hyps, hyp_len, in_len, blank):
    """ll (B,N) float64 and dll (B,N,T,V) float64: hyps a nested list [b][n] of label lists, hyp_len[b][n] < 0 = unused"""
    B, T, V = logits.shape
    N = len(hyps[0])
    ll = torch.full((B, N), -math.inf, dtype=torch.float64)
    dll = torch.zeros(B, N, T, V, dtype=torch.float64)
    for b in range(B):
        Tb = max(0, min(int(in_len[b]), T))
        for n in range(N):
            if hyp_len[b][n] < 0:
                continue
            ll[b, n], dll[b, n] = row_ll_and_grad(logits[b], list(hyps[b][n])[:hyp_len[b][n]], Tb, blank)
    return ll, dll


def ll_ctc_loss(logits, hyps, hyp_len, in_len, blank):
    """The same ll through F.ctc_loss(reduction="none") in double (inf -> -inf); unused rows -inf"""
    B, T, V = logits.shape
    N = len(hyps[0])
    lp = logits.double().log_softmax(-1)
    ll = torch.full((B, N), -math.inf, dtype=torch.float64)
    for b in range(B):
        Tb = max(0, min(int(in_len[b]), T))
        for n in range(N):
            L = hyp_len[b][n]
            if L < 0:
                continue
            if Tb == 0:
                ll[b, n] = 0.0 if L == 0 else -math.inf
                continue
            tg = torch.tensor([list(hyps[b][n])[:L]], dtype=torch.int64).reshape(1, L)
            nll = F.ctc_loss(lp[b, :Tb, None, :], tg, torch.tensor([Tb]), torch.tensor([L]), blank=blank, reduction="none")
            ll[b, n] = -nll[0]
    return ll


def risk(ll, errors, hyp_len):
    """(loss, risk (B)) of the lists, differentiable in ll: over the live rows (used, finite ll) P = softmax(ll), R = sum P W,
    risk = R - mean W; fewer than two live rows: 0.  loss = mean over the batch."""
    B, N = ll.shape
    out = []
    for b in range(B):
        live = [n for n in range(N) if hyp_len[b][n] >= 0 and math.isfinite(float(ll[b, n].detach()))]
        if len(live) < 2:
            out.append(ll.new_zeros(()))
            continue
        W = torch.tensor([float(errors[b][n]) for n in live], dtype=torch.float64)
        P = torch.softmax(ll[b, live], dim=0)
        out.append((P * W).sum() - W.mean())
    r = torch.stack(out)
    return r.mean(), r


def risk_weights(ll, errors, hyp_len):
    """(loss, d loss / d ll (B,N) by autograd, risk (B), max_n |W_n - R_b| over the live rows (B))"""
    x = ll.clone()
    finite = torch.isfinite(x)
    x = torch.where(finite, x, torch.zeros_like(x)).requires_grad_(True)
    lx = torch.where(finite, x, torch.full_like(x, -math.inf))
    loss, r = risk(lx, errors, hyp_len)
    (g,) = torch.autograd.grad(loss, x, allow_unused=True) if loss.requires_grad else (None,)
    g = torch.zeros_like(x) if g is None else torch.where(finite, g, torch.zeros_like(g))
    spread = []
    for b in range(ll.shape[0]):
        live = [n for n in range(ll.shape[1]) if hyp_len[b][n] >= 0 and bool(finite[b, n])]
        if len(live) < 2:
            spread.append(0.0)
            continue
        W = torch.tensor([float(errors[b][n]) for n in live], dtype=torch.float64)
        R = float((torch.softmax(ll[b, live], dim=0) * W).sum())
        spread.append(float((W - R).abs().max()))
    return loss.detach(), g.detach(), r.detach(), torch.tensor(spread, dtype=torch.float64)


def closed_form_weights(ll, errors, hyp_len):
    """P_n (W_n - R_b) / B, zeros for rows that are not live and utterances with fewer than two live rows"""
    B, N = ll.shape
    w = torch.zeros(B, N, dtype=torch.float64)
    for b in range(B):
        live = [n for n in range(N) if hyp_len[b][n] >= 0 and math.isfinite(float(ll[b, n]))]
        if len(live) < 2:
            continue
        W = torch.tensor([float(errors[b][n]) for n in live], dtype=torch.float64)
        P = torch.softmax(ll[b, live], dim=0)
        w[b, live] = P * (W - (P * W).sum()) / B
    return w


def posterior(ll, hyp_len):
    B, N = ll.shape
    p = torch.zeros(B, N, dtype=torch.float64)
    for b in range(B):
        live = [n for n in range(N) if hyp_len[b][n] >= 0 and math.isfinite(float(ll[b, n]))]
        if live:
            p[b, live] = torch.softmax(ll[b, live], dim=0)
    return p


def weighted_grad(dll, weight):
    """(sum_n w_n dll_n, sum_n |w_n| |dll_n|): the gradient and the size of the terms summed, both (B,T,V)"""
    w = weight.double()[:, :, None, None]
    return (w * dll).sum(1), (w.abs() * dll.abs()).sum(1)


# ---- the hand-built list of the GPU tests: B = 3, N = 4, in_len = [37, 20, 1], blank 0 ----------------------------------------
def hand_built(V):
    """(hyps [b][n], hyp_len [b][n], in_len): repeated labels, the empty hypothesis, an infeasible row (utterance 2: one frame,
    two labels), an unused row, two rows that differ in one label"""
    a = [2, 2, 2, 3]                                   # needs 4 + 2 frames
    b0 = [5, 7, 9, 11, 4, 6]
    b1 = [5, 7, 9, 12, 4, 6]                           # differs from b0 in one label
    top = V - 1
    hyps = [[a, b0, b1, []],
            [b0, [top, 1, top], a, [3]],
            [[4], [4, 5], [], [7]]]
    hyp_len = [[4, 6, 6, 0],
               [6, 3, 4, -1],                          # row 3 unused
               [1, 2, 0, 1]]                           # row 1 infeasible at one frame
    return hyps, hyp_len, [37, 20, 1]


def padded(hyps, hyp_len, width=None):
    """hyps as a (B,N,width) int64 tensor padded with -1, hyp_len as (B,N) int64"""
    width = width or max(1, max(len(h) for row in hyps for h in row))
    t = torch.full((len(hyps), len(hyps[0]), width), -1, dtype=torch.int64)
    for b, row in enumerate(hyps):
        for n, h in enumerate(row):
            t[b, n, :len(h)] = torch.tensor(h, dtype=torch.int64)
    return t, torch.tensor(hyp_len, dtype=torch.int64)
