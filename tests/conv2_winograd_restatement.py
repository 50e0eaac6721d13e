"""Float64 restatement of the stem conv2 as polyphase Winograd F(2x2,2x2) (csrc/conv2_wino_f32.hip): the term / pattern
index map, the weight transform and the output transform.  h1 is channel-last (B, T1, F1, C); w2 is (C_out, C_in, 3, 3)
indexed [co][ci][kf][kt], as the stem stores it."""
import torch

# per dimension pattern a in {0, 1, 2}: list of terms (pixels [(d, sign)], taps [k])
DIM_TERMS = {
    0: [([(0, 1.0), (2, -1.0)], [0]), ([(1, 1.0)], [1])],
    1: [([(2, 1.0)], [0, 2])],
    2: [([(4, 1.0), (2, -1.0)], [2]), ([(3, 1.0)], [1])],
}


def pattern_terms(p):
    """Terms of pattern p = 3 a + b in walk order u = ut * nf + uf."""
    a, b = divmod(p, 3)
    return [(tt, tf) for tt in DIM_TERMS[a] for tf in DIM_TERMS[b]]


def term_weight(w2, tt, tf):
    """(C_out, C_in): the sum of w2[:, :, kf, kt] over the term's time and frequency taps."""
    return sum(w2[:, :, kf, kt] for kt in tt[1] for kf in tf[1])


def pack(w2):
    """The kernel's weight pack: pattern blocks in p order, each (C_out, nt * C) with column nt*32*(ci//32) + 32*u + ci%32."""
    C = w2.shape[0]
    out = []
    for p in range(9):
        terms = pattern_terms(p)
        nt = len(terms)
        blk = torch.empty(C, nt * C, dtype=w2.dtype)
        for u, (tt, tf) in enumerate(terms):
            wt = term_weight(w2, tt, tf)
            for c32 in range(C // 32):
                blk[:, nt * 32 * c32 + 32 * u: nt * 32 * c32 + 32 * u + 32] = wt[:, 32 * c32: 32 * c32 + 32]
        out.append(blk.reshape(-1))
    return torch.cat(out)


def planes(h1, w2):
    """The nine pattern planes (9, B, TI, TJ, C_out) of h1 (B, T1, F1, C), pixels outside T1 x F1 taken as zero."""
    B, T1, F1, C = h1.shape
    T2, F2 = (T1 - 1) // 2, (F1 - 1) // 2
    TI, TJ = (T2 + 1) // 2, (F2 + 1) // 2
    hp = torch.zeros(B, 4 * TI + 1, 4 * TJ + 1, C, dtype=h1.dtype)
    hp[:, :min(T1, 4 * TI + 1), :min(F1, 4 * TJ + 1)] = h1[:, :4 * TI + 1, :4 * TJ + 1]
    out = []
    for p in range(9):
        acc = torch.zeros(B, TI, TJ, w2.shape[0], dtype=h1.dtype)
        for tt, tf in pattern_terms(p):
            x = sum(st * sf * hp[:, dt:dt + 4 * TI:4, df:df + 4 * TJ:4] for dt, st in tt[0] for df, sf in tf[0])
            acc += x @ term_weight(w2, tt, tf).T
        out.append(acc)
    return torch.stack(out)


def combine(P, b2, T2, F2):
    """h2 (B, T2, F2, C) = relu(b2 + sum_{a in S(r), b in S(s)} P_ab), S(0) = {0, 1}, S(1) = {1, 2}."""
    _, B, TI, TJ, C = P.shape
    y = torch.empty(B, 2 * TI, 2 * TJ, C, dtype=P.dtype)
    for r in range(2):
        for s in range(2):
            y[:, r::2, s::2] = sum(P[3 * a + b] for a in (r, r + 1) for b in (s, s + 1))
    return torch.relu(y[:, :T2, :F2] + b2)


def conv2_winograd(h1, w2, b2):
    B, T1, F1, C = h1.shape
    return combine(planes(h1, w2), b2, (T1 - 1) // 2, (F1 - 1) // 2)


def conv2_direct(h1, w2, b2):
    """relu(conv2d(stride 2)) in the same channel-last layout: the conv's H is time, W frequency, so the kernel is w2^T."""
    x = h1.permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(x, w2.transpose(2, 3), b2, stride=2)
    return torch.relu(y).permute(0, 2, 3, 1)
