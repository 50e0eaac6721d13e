"""Ill-conditioned statistics: input classes, condition number, fp32 emulations and the error table `C` shared by
test_stats_conditioning_cpu.py and test_stats_conditioning_gpu.py.  Pure torch, no GPU.

Every kernel that computes or consumes a (mean, variance) pair is documented as free of the E[x^2] - mean^2 cancellation: the
two-pass LayerNorm, the (sum, M2 about the own mean) partials of the GEMM / ffn_fused / rowchain epilogues, the Chan merges of
the folded consumers and of the BatchNorm statistics.  With

    kappa = sqrt(1 + (mean * rstd)^2),      rstd = 1 / sqrt(var + eps)                (eps INSIDE rstd: flat rows are finite)

a correct fp32 algorithm is wrong by a few eps32 * kappa and a one-pass one by eps32 * kappa^2.  The bound of every test is

    C[family] * EPS32 * kappa_class         (kappa_class = the largest kappa of the class's rows)

and C[family] is FOUR times the largest err / (EPS32 * kappa_class) that the fp32 emulation below shows over all classes and the
widths of `EMU_WIDTHS` (the 4x: the device's summation order and its rcp / exp forms).  How the error is taken:

    outputs   per-class rel-L2 against float64
    mean      max over rows of |mean - mu| / max(|mu|, sqrt(var + eps))     (never above "absolute error over |mu|": at mu = 0
              that ratio is undefined, and a mean is known to eps32 times the size of the terms it sums, not to eps32 * |mu|)
    rstd      max over rows of the relative error
"""
import math

import torch

EPS32 = 2.0 ** -24
LN_EPS = 1e-5
SCALES = (1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3)


# ---- row classes ----------------------------------------------------------------------------------------------------------
def noise(*shape, seed=0):
    """Unit-variance noise that is the same bits on every host: twelve uniform integers summed exactly (Irwin-Hall), where
    torch.randn goes through the host's vector log / sin and differs in the last place from one CPU to another -- enough to move
    the largest error over 70 rows by a fifth."""
    g = torch.Generator().manual_seed(seed)
    acc = torch.zeros(*shape, dtype=torch.int64)
    for _ in range(12):
        acc += torch.randint(0, 1 << 20, tuple(shape), generator=g, dtype=torch.int64)
    return (acc.double() / (1 << 20) - 6.0).float()


def _offset(mu):
    return lambda rows, d, seed: noise(rows, d, seed=seed) + mu


def _flat(c):
    return lambda rows, d, seed: torch.full((rows, d), float(c))


def _near_flat(rows, d, seed):
    """73 +- 1e-2: the relative spread of 7.3 +- 1e-3, ten times up, so that the variance (1e-4) stands above eps = 1e-5.  Below
    eps, rstd hardly depends on the variance and a one-pass variance, wrong by 30 %, stayed within 40 x of the right one."""
    return 73.0 + 1e-2 * noise(rows, d, seed=seed)


def _common_sign(rows, d, seed):
    return 2 * noise(rows, d, seed=seed).abs() + 0.5


def _outlier(rows, d, seed):
    """z with one column at 200; the column moves to another 32-column group from row to row (where d has more than one)."""
    x = noise(rows, d, seed=seed)
    r = torch.arange(rows)
    col = ((r % max(1, d // 32)) * 32 + (7 * r) % 32) % d
    x[r, col] = 200.0
    return x


BASE = {
    "offset+30": _offset(30.0), "offset-30": _offset(-30.0), "offset+300": _offset(300.0), "offset-300": _offset(-300.0),
    "offset+3000": _offset(3000.0),
    "flat0": _flat(0.0), "flat1": _flat(1.0), "flat7.3": _flat(7.3), "flat-1000": _flat(-1000.0),
    "nearflat": _near_flat, "commonsign": _common_sign, "outlier": _outlier,
}
# The interleave leaves flat-1000 to its own class and does not scale the flat rows: a flat row has kappa = |c| / sqrt(eps), 3e5
# at c = 1000, and the class bound would be of order 0.1 -- no longer orders of magnitude below what a row index off by one
# costs.  With them kappa_mixed is about 7e3 (near-flat x 1e3) and the bound a few 1e-3 against an O(1) error.
MIXED = tuple(n for n in BASE if n != "flat-1000")


def _mixed(rows, d, seed):
    x = torch.empty(rows, d)
    for i, name in enumerate(MIXED):
        x[i::len(MIXED)] = BASE[name](rows, d, seed + 1 + i)[i::len(MIXED)]
    s = torch.tensor([1.0 if MIXED[r % len(MIXED)].startswith("flat") else SCALES[r % len(SCALES)] for r in range(rows)])
    return x * s[:, None]


CLASSES = dict(BASE, mixed=_mixed)
WELL = "well"                                      # z alone (kappa ~ 1): only where a test names it (the row-walk routes)
OFFSET_MAX = "offset+3000"                         # the offset class with the largest kappa
NEAR_FLAT = "nearflat"


def make(name, rows, d, seed=0):
    """(rows, d) fp32 input of class `name`."""
    if name == WELL:
        return noise(rows, d, seed=seed)
    return CLASSES[name](rows, d, seed).float().contiguous()


def kappa(x, eps=LN_EPS):
    """Per-row condition number of (mean, rstd) over the last axis, float64."""
    xd = x.double()
    mu = xd.mean(-1)
    var = ((xd - mu[..., None]) ** 2).mean(-1)
    return torch.sqrt(1 + mu * mu / (var + eps))


def stats64(x, eps=LN_EPS):
    """(mean, var, rstd) of every row in float64."""
    xd = x.double()
    mu = xd.mean(-1)
    var = ((xd - mu[..., None]) ** 2).mean(-1)
    return mu, var, 1 / torch.sqrt(var + eps)


# ---- error measures ---------------------------------------------------------------------------------------------------------
def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    den = float(b.norm())
    return float((a - b).norm()) / (den if den > 0 else 1.0)


def mean_err(mean, mu, var, eps=LN_EPS):
    den = torch.maximum(mu.abs(), torch.sqrt(var + eps))
    return float(((mean.detach().double().cpu() - mu).abs() / den).max())


def rstd_err(rstd, ref):
    return float(((rstd.detach().double().cpu() - ref).abs() / ref).max())


def stats_err(mean, rstd, x, eps=LN_EPS):
    """The larger of the mean and the rstd error of fp32 statistics against the float64 statistics of x's rows."""
    mu, var, rs = stats64(x, eps)
    return max(mean_err(mean, mu, var, eps), rstd_err(rstd, rs))


# ---- fp32 emulations of the arithmetic the kernels document ------------------------------------------------------------------
def ln_params(d, seed=100):
    return 1 + 0.3 * noise(d, seed=seed), 1 + 0.2 * noise(d, seed=seed + 1000)


def layernorm64(x, gamma, beta, eps=LN_EPS):
    mu, _, rs = stats64(x, eps)
    return (x.double() - mu[:, None]) * rs[:, None] * gamma.double() + beta.double()


def tsum(x):
    """Sum over the last axis in fp32 as a halving tree of element-wise additions (the order of the kernels' shuffle reductions;
    unlike a library reduction it is the same arithmetic on every host)."""
    n = 1 << max(0, (x.shape[-1] - 1).bit_length())
    if n != x.shape[-1]:
        x = torch.cat([x, x.new_zeros(*x.shape[:-1], n - x.shape[-1])], dim=-1)
    while n > 1:
        n //= 2
        x = x[..., :n] + x[..., n:]
    return x[..., 0]


def mm_seq(x, wt, step=4):
    """x @ wt in fp32 with the contraction accumulated `step` columns at a time, in order (the MFMA K-loop)."""
    acc = torch.zeros(x.shape[0], wt.shape[1])
    for k in range(0, x.shape[1], step):
        acc = acc + tsum(x[:, None, k:k + step] * wt.t()[None, :, k:k + step])
    return acc


def ln_two_pass(x, gamma, beta, eps=LN_EPS):
    """layernorm.hip: mean, then the centred variance.  Returns (y, mean, rstd), all fp32."""
    d = x.shape[-1]
    mean = tsum(x)[:, None] / d
    c = x - mean
    rstd = 1 / torch.sqrt(tsum(c * c)[:, None] / d + eps)
    return c * rstd * gamma + beta, mean[:, 0], rstd[:, 0]


def ln_one_pass(x, gamma, beta, eps=LN_EPS):
    """The variant the kernels must NOT be: var = E[x^2] - mean^2."""
    d = x.shape[-1]
    mean = tsum(x)[:, None] / d
    var = (tsum(x * x)[:, None] / d - mean * mean).clamp_min(0)
    rstd = 1 / torch.sqrt(var + eps)
    return (x - mean) * rstd * gamma + beta, mean[:, 0], rstd[:, 0]


def partials(x, width=32):
    """(rows, d / width, 2) fp32: (sum, M2 about the group's own mean) of every `width` columns (the producers' epilogues)."""
    g = x.reshape(x.shape[0], -1, width)
    s = tsum(g)
    c = g - (s / width)[..., None]
    return torch.stack([s, tsum(c * c)], dim=-1)


def partials_sumsq(x, width=32):
    """The one-pass variant: (sum, sum of squares)."""
    g = x.reshape(x.shape[0], -1, width)
    return torch.stack([tsum(g), tsum(g * g)], dim=-1)


def chan_merge_equal(st, d, eps=LN_EPS):
    """Equal-count Chan merge of the partials in a binary tree (gemm_f32.hip, LN == 1 prologue).  Returns (mean, rstd) fp32."""
    parts = st.shape[1]
    n = float(d // parts)
    mean, m2 = st[..., 0] / n, st[..., 1]
    while mean.shape[1] > 1:
        a, b = mean[:, 0::2], mean[:, 1::2]
        dl = b - a
        m2 = m2[:, 0::2] + m2[:, 1::2] + dl * dl * (0.5 * n)
        mean = 0.5 * (a + b)
        n *= 2
    return mean[:, 0], 1 / torch.sqrt(m2[:, 0] / d + eps)


def merge_sumsq(st, d, eps=LN_EPS):
    mean = tsum(st[..., 0]) / d
    var = (tsum(st[..., 1]) / d - mean * mean).clamp_min(0)
    return mean, 1 / torch.sqrt(var + eps)


def fold_params(n, d, seed=200):
    """(W, b, gamma, beta) of a LayerNorm + Linear pair and its folded form (Wf, bias_f, colsum) as ops.fold_layernorm builds it."""
    w, b = noise(n, d, seed=seed) / math.sqrt(d), noise(n, seed=seed + 1000)
    gamma, beta = ln_params(d, seed + 1)
    wf = (w * gamma[None, :]).contiguous()
    bf = (b.double() + w.double() @ beta.double()).float()
    cs = wf.double().sum(1).float()
    return (w, b, gamma, beta), (wf, bf, cs)


def fold_consumer(x, mean, rstd, wf, bf, cs):
    """rstd * (x . Wf^T - mean * colsum) + bias_f in fp32 (the epilogue of the folded GEMM)."""
    return rstd[:, None] * (mm_seq(x, wf.t()) - mean[:, None] * cs[None, :]) + bf


def fold64(x, w, b, gamma, beta, eps=LN_EPS):
    return layernorm64(x, gamma, beta, eps) @ w.double().t() + b.double()


def bn_chan(v, chunk=16):
    """Per-channel (mean, biased var) of v (N, C): (count, mean, M2) of every `chunk` rows, merged in order with Chan's update
    (backward_ew.hip: chan_merge).  fp32."""
    n = torch.zeros(())
    mean = torch.zeros(v.shape[1])
    m2 = torch.zeros(v.shape[1])
    for i in range(0, v.shape[0], chunk):
        blk = v[i:i + chunk]
        nb = torch.tensor(float(blk.shape[0]))
        mb = tsum(blk.t()) / nb
        qb = tsum(((blk - mb) ** 2).t())
        nn = n + nb
        dl, f = mb - mean, nb / nn
        mean = mean + dl * f
        m2 = m2 + qb + dl * dl * n * f
        n = nn
    return mean, m2 / n


def bn_one_pass(v):
    n = v.shape[0]
    mean = tsum(v.t()) / n
    return mean, (tsum((v * v).t()) / n - mean * mean).clamp_min(0)


def bn_columns(n, names, seed=300):
    """(n, len(names)) fp32: column j is a row of class names[j] (the channels play the classes)."""
    return torch.stack([make(nm, 1, n, seed + j)[0] for j, nm in enumerate(names)], dim=1).contiguous()


# ---- the emulation's own error, in units of EPS32 * kappa_class ---------------------------------------------------------------
EMU_ROWS = 70
EMU_WIDTHS = {"ln_out": (32, 512, 2052), "ln_stats": (32, 512, 2052), "merged": (32, 128, 512), "fold": (32, 128, 512), "bn": (400,)}
FOLD_N = 96
BN_EMU_CHANNELS = 16
BN_CLASSES = tuple(BASE)                                        # a channel is one row: the interleave has no meaning there


def emulation_ratio(family, name, d, one_pass=False, seed=0):
    """err / (EPS32 * kappa_class) of the family's fp32 emulation (or of its one-pass variant) on class `name` at width d."""
    if family == "bn":
        v = bn_columns(d, [name] * BN_EMU_CHANNELS, seed + 300)
        mean, var = (bn_one_pass if one_pass else bn_chan)(v)
        return stats_err(mean, 1 / torch.sqrt(var + LN_EPS), v.t()) / (EPS32 * float(kappa(v.t()).max()))
    x = make(name, EMU_ROWS, d, seed)
    unit = EPS32 * float(kappa(x).max())
    gamma, beta = ln_params(d)
    if family in ("ln_out", "ln_stats"):
        y, mean, rstd = (ln_one_pass if one_pass else ln_two_pass)(x, gamma, beta)
        if family == "ln_out":
            return rel_l2(y, layernorm64(x, gamma, beta)) / unit
        return stats_err(mean, rstd, x) / unit
    mean, rstd = merge_sumsq(partials_sumsq(x), d) if one_pass else chan_merge_equal(partials(x), d)
    if family == "merged":
        return stats_err(mean, rstd, x) / unit
    assert family == "fold"
    raw, (wf, bf, cs) = fold_params(FOLD_N, d)
    return rel_l2(fold_consumer(x, mean, rstd, wf, bf, cs), fold64(x, *raw)) / unit


def family_classes(family):
    return BN_CLASSES if family == "bn" else tuple(CLASSES)


# ---- the table --------------------------------------------------------------------------------------------------------------
# emu: the largest emulation_ratio over family_classes x EMU_WIDTHS (test_stats_conditioning_cpu.py holds it at <= C / 4);
# C: the constant of the bound, 4 x emu rounded up to a whole number; gpu: the largest ratio the gfx950 kernels of the family
# showed in test_stats_conditioning_gpu.py on an MI355X (recorded, not asserted: ln_out from layernorm on flat7.3 rows, d = 2052;
# ln_stats from layernorm_train on outlier rows, d = 1024; merged from linear_residual on outlier rows, d = 512; fold from the
# increment of ffn_fused on flat7.3 rows, d = 512; bn from swish_bn_eval on the flat7.3 columns).
TABLE = {
    "ln_out":   {"emu": 1.03, "C": 5.0, "gpu": 1.13},       # emu: outlier, d = 512
    "ln_stats": {"emu": 3.70, "C": 15.0, "gpu": 3.17},      # emu: outlier, d = 2052 (the mean)
    "merged":   {"emu": 3.20, "C": 13.0, "gpu": 2.16},      # emu: outlier, d = 512 (the mean)
    "fold":     {"emu": 2.57, "C": 11.0, "gpu": 8.10},      # emu: flat1, d = 512 (x . Wf^T - mean * colsum)
    "bn":       {"emu": 4.38, "C": 18.0, "gpu": 3.70},      # emu: outlier (the mean)
}
C = {k: v["C"] for k, v in TABLE.items()}

