"""A float64 restatement of the transducer (INTEGRATION.md "Transducer (RNN-T)") in plain loops: the lattice and its likelihood,
the closed-form gradient, the predictor (embedding + LSTM) and joiner, and the time-synchronous greedy loop.  A helper, not a test
module; it shares nothing with conformer_amd (torch is used for float64 tensors and, in `ll_autograd`, for autograd)."""
import math

import torch

NEG = -math.inf


def clamp(v, lo, hi):
    return max(lo, min(hi, int(v)))


def lae(a, b):
    if a == NEG:
        return b
    if b == NEG:
        return a
    m = max(a, b)
    return m + math.log1p(math.exp(-abs(a - b)))


def geometry(T, U1, V, targets_b, in_len_b, tg_len_b):
    Tb, Ub = clamp(in_len_b, 0, T), clamp(tg_len_b, 0, U1 - 1)
    y = [clamp(targets_b[u], 0, V - 1) for u in range(Ub)]
    return Tb, Ub, y


def lattice(lp, y, Tb, Ub, blank):
    """alpha, beta (lists [t][u]) and ll of one utterance from lp (T,U1,V) = log_softmax (nested lists or a tensor)"""
    alpha = [[NEG] * (Ub + 1) for _ in range(Tb)]
    beta = [[NEG] * (Ub + 1) for _ in range(Tb)]
    for t in range(Tb):
        for u in range(Ub + 1):
            if t == 0 and u == 0:
                alpha[t][u] = 0.0
                continue
            up = alpha[t - 1][u] + float(lp[t - 1][u][blank]) if t > 0 else NEG
            left = alpha[t][u - 1] + float(lp[t][u - 1][y[u - 1]]) if u > 0 else NEG
            alpha[t][u] = lae(up, left)
    for t in range(Tb - 1, -1, -1):
        for u in range(Ub, -1, -1):
            if t == Tb - 1 and u == Ub:
                beta[t][u] = float(lp[t][u][blank])
                continue
            down = beta[t + 1][u] + float(lp[t][u][blank]) if t + 1 < Tb else NEG
            right = beta[t][u + 1] + float(lp[t][u][y[u]]) if u < Ub else NEG
            beta[t][u] = lae(down, right)
    ll = alpha[Tb - 1][Ub] + float(lp[Tb - 1][Ub][blank])
    return alpha, beta, ll


def loss_and_grad(logits, targets, in_len, tg_len, blank):
    """logits (B,T,U1,V) float64.  Returns (nll (B) float64, +inf where in_len clamps to 0; grad (B,T,U1,V) = d nll_b / d logits,
    the closed form at unit weight; terms (B,T,U1,V) = gamma softmax + eb [v = blank] + el [v = y_u], the sizes of the terms
    the gradient sums)."""
    B, T, U1, V = logits.shape
    lp_all = torch.log_softmax(logits.double(), -1)
    nll = torch.zeros(B, dtype=torch.float64)
    grad = torch.zeros(B, T, U1, V, dtype=torch.float64)
    terms = torch.zeros(B, T, U1, V, dtype=torch.float64)
    for b in range(B):
        Tb, Ub, y = geometry(T, U1, V, [] if targets is None else targets[b].tolist(), in_len[b], tg_len[b])
        if Tb == 0:
            nll[b] = math.inf
            continue
        lp = lp_all[b].tolist()
        alpha, beta, ll = lattice(lp, y, Tb, Ub, blank)
        assert abs(ll - beta[0][0]) <= 1e-9 * max(1.0, abs(ll))
        nll[b] = -ll
        for t in range(Tb):
            for u in range(Ub + 1):
                gamma = math.exp(alpha[t][u] + beta[t][u] - ll)
                nxt = beta[t + 1][u] if t + 1 < Tb else (0.0 if u == Ub else NEG)
                eb = math.exp(alpha[t][u] + lp[t][u][blank] + nxt - ll) if nxt != NEG else 0.0
                el = math.exp(alpha[t][u] + lp[t][u][y[u]] + beta[t][u + 1] - ll) if u < Ub else 0.0
                sm = torch.exp(lp_all[b, t, u])
                grad[b, t, u] = gamma * sm
                terms[b, t, u] = gamma * sm
                grad[b, t, u, blank] -= eb
                terms[b, t, u, blank] += eb
                if u < Ub:
                    grad[b, t, u, y[u]] -= el
                    terms[b, t, u, y[u]] += el
    return nll, grad, terms


def ll_by_enumeration(lp, y, Tb, Ub, blank):
    """log of the sum over every path: Tb blanks and Ub labels in any order that ends with the blank at (Tb - 1, Ub)"""
    total = [NEG]

    def walk(t, u, acc):
        if t == Tb - 1 and u == Ub:
            total[0] = lae(total[0], acc + float(lp[t][u][blank]))
            return
        if t + 1 < Tb:
            walk(t + 1, u, acc + float(lp[t][u][blank]))
        if u < Ub:
            walk(t, u + 1, acc + float(lp[t][u][y[u]]))

    walk(0, 0, 0.0)
    return total[0]


def ll_autograd(logits_b, y, Tb, Ub, blank):
    """the alpha recursion of one utterance on float64 tensors, for torch.autograd"""
    lp = torch.log_softmax(logits_b, -1)
    alpha = {}
    for t in range(Tb):
        for u in range(Ub + 1):
            if t == 0 and u == 0:
                alpha[t, u] = lp.new_zeros(())
                continue
            parts = []
            if t > 0:
                parts.append(alpha[t - 1, u] + lp[t - 1, u, blank])
            if u > 0:
                parts.append(alpha[t, u - 1] + lp[t, u - 1, y[u - 1]])
            alpha[t, u] = torch.logsumexp(torch.stack(parts), 0)
    return alpha[Tb - 1, Ub] + lp[Tb - 1, Ub, blank]


# ---- the model heads ---------------------------------------------------------------------------------------------------------------

def _lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh):
    H = h.shape[0]
    g = w_ih @ x + b_ih + w_hh @ h + b_hh
    i, f, gg, o = torch.sigmoid(g[:H]), torch.sigmoid(g[H:2 * H]), torch.tanh(g[2 * H:3 * H]), torch.sigmoid(g[3 * H:])
    c = f * c + i * gg
    return o * torch.tanh(c), c


class Heads:
    """predictor.* and joiner.* parameters as float64 (a state_dict of those two modules, prefixes included)"""

    def __init__(self, sd, blank, as_given=False):
        """as_given: sd already holds float64 tensors to use as they are (leaves of an autograd graph)"""
        self.p = dict(sd) if as_given else {k: v.detach().double().cpu() for k, v in sd.items()}
        self.blank = blank
        self.n_layers = sum(1 for k in self.p if k.startswith("predictor.lstm.weight_ih_l"))
        self.H = self.p["predictor.lstm.weight_hh_l0"].shape[1]

    def zero_state(self):
        return [(torch.zeros(self.H, dtype=torch.float64), torch.zeros(self.H, dtype=torch.float64)) for _ in range(self.n_layers)]

    def step(self, token, state):
        """one predictor step: returns (top output, new state)"""
        x = self.p["predictor.embedding.weight"][token]
        new = []
        for k in range(self.n_layers):
            h, c = _lstm_cell(x, *state[k], *(self.p[f"predictor.lstm.{n}_l{k}"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")))
            new.append((h, c))
            x = h
        return x, new

    def predictor(self, targets_b, Ub):
        """(Ub + 1, H): the outputs over [blank, y_0 .. y_{Ub-1}]"""
        state, out = self.zero_state(), []
        for tok in [self.blank] + list(targets_b[:Ub]):
            y, state = self.step(int(tok), state)
            out.append(y)
        return torch.stack(out)

    def joint(self, enc_row, pred_row):
        e = self.p["joiner.enc_proj.weight"] @ enc_row + self.p["joiner.enc_proj.bias"]
        q = self.p["joiner.pred_proj.weight"] @ pred_row + self.p["joiner.pred_proj.bias"]
        return self.p["joiner.out.weight"] @ torch.tanh(e + q) + self.p["joiner.out.bias"]

    def logits(self, enc_b, pred_b):
        """(T, U, V) from enc_b (T, d) and pred_b (U, H)"""
        e = enc_b @ self.p["joiner.enc_proj.weight"].T + self.p["joiner.enc_proj.bias"]
        q = pred_b @ self.p["joiner.pred_proj.weight"].T + self.p["joiner.pred_proj.bias"]
        return torch.tanh(e[:, None, :] + q[None, :, :]) @ self.p["joiner.out.weight"].T + self.p["joiner.out.bias"]

    def greedy(self, enc_b, Tb, max_symbols):
        """(tokens, frames, margins, cuts): margins = top-1 minus top-2 logit at every decision visited, cuts = the decisions
        at which a non-blank argmax was not emitted because the frame already held max_symbols tokens"""
        tokens, frames, margins, cuts = [], [], [], 0
        out, state = self.step(self.blank, self.zero_state())
        t = n = 0
        while t < Tb:
            z = self.joint(enc_b[t], out)
            top = torch.topk(z, 2)
            margins.append(float(top.values[0] - top.values[1]))
            k = int(top.indices[0])
            if k != self.blank and n < max_symbols:
                tokens.append(k)
                frames.append(t)
                n += 1
                out, state = self.step(k, state)
            else:
                cuts += int(k != self.blank)
                t += 1
                n = 0
        return tokens, frames, margins, cuts


GREEDY_SEED = 4         # chosen on the CPU (tests/test_rnnt_cpu.py checks what it must give)
GREEDY_SHAPE = dict(B=3, T=23, V=29, d=16, H=16, J=20, n_layers=2, blank=0, max_symbols=2, in_len=(23, 15, 23))


def greedy_fixture(seed=GREEDY_SEED):
    """(state_dict of `predictor.*` / `joiner.*` fp32 tensors, enc (B,T,d) fp32) of the greedy-decode fixture: two loud
    utterances (the second shorter than T) and a silent one (all-zero frames) under an output bias that favours blank"""
    s = GREEDY_SHAPE
    g = torch.Generator().manual_seed(1000 + seed)

    def u(*shape, scale):
        return (torch.rand(*shape, generator=g) * 2 - 1) * scale

    sd = {"predictor.embedding.weight": u(s["V"], s["H"], scale=1.0)}
    for k in range(s["n_layers"]):
        sd[f"predictor.lstm.weight_ih_l{k}"] = u(4 * s["H"], s["H"], scale=0.3)
        sd[f"predictor.lstm.weight_hh_l{k}"] = u(4 * s["H"], s["H"], scale=0.3)
        sd[f"predictor.lstm.bias_ih_l{k}"] = u(4 * s["H"], scale=0.3)
        sd[f"predictor.lstm.bias_hh_l{k}"] = u(4 * s["H"], scale=0.3)
    sd["joiner.enc_proj.weight"] = u(s["J"], s["d"], scale=0.5)
    sd["joiner.enc_proj.bias"] = u(s["J"], scale=0.1)
    sd["joiner.pred_proj.weight"] = u(s["J"], s["H"], scale=0.5)
    sd["joiner.pred_proj.bias"] = u(s["J"], scale=0.1)
    sd["joiner.out.weight"] = u(s["V"], s["J"], scale=0.5)
    sd["joiner.out.bias"] = u(s["V"], scale=0.1)
    sd["joiner.out.bias"][s["blank"]] = 2.5
    enc = torch.randn(s["B"], s["T"], s["d"], generator=g) * 2.0
    enc[2] = 0.0
    return sd, enc


def greedy_reference(seed=GREEDY_SEED):
    """per utterance (tokens, frames, margins, cuts) of the fixture"""
    sd, enc = greedy_fixture(seed)
    s = GREEDY_SHAPE
    heads = Heads(sd, s["blank"])
    return [heads.greedy(enc[b].double(), clamp(s["in_len"][b], 0, s["T"]), s["max_symbols"]) for b in range(s["B"])]
