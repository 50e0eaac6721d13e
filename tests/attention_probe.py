"""Per-element softmax-mass probes of the attention forward (helper, not a test file; tests/test_attention_probe_{cpu,gpu}.py).

A whole-tensor rel_l2 on random operands averages a local mistake away: one lost (query row, key) pair moves it by ~1e-3 in
bf16, under every 16-bit bar of the suite.  The probes choose inputs for which the ONLY inexact step left in the 16-bit kernel is
the one rounding of P, so the error bound is a statement per element:

  * operands that round to themselves: q, k and the projected positions are multiples of 0.25 in [-1, 1], the biases u, v
    multiples of 0.25 in [-0.5, 0.5]; q+u, q+v, k and pos are then exact in bf16 and fp16 (`operands` asserts it), every product is
    a multiple of 1/16 below 2 and every 64-term sum is exact in fp32: the scores are exact up to the one multiply by
    inv_sqrt_dh * log2 e;
  * V holds only 0 and 1 (exact in every type, so P.V adds rounded p's exactly in fp32): V[k,h,c] = 1 iff c == col(k,h); every
    output element is the softmax mass of the known key set {k : col(k,h) == c}.  Pattern A: col = (k + h) % dh; pattern B:
    col = (k + k // dh + h) % dh, which separates key k from key k + dh where A cannot (dh = 8 against a 32-key tile).

Bound, per element (ref = float64 mass from oracle.conformer_oracle.relpos_attention_core):

      |ctx - ref| <= (u_t + F) * ref + floor                 fp32 context
      |ctx - ref| <= (2 u_t + u_t^2 + F) * ref + floor       context stored in the 16-bit type

u_t is the unit roundoff of P's type under round-to-nearest (2^-8 bf16, 2^-11 fp16, 0 for the fp32 kernels): all p are >= 0 and
the row sum l is taken from the UNROUNDED p, so a sum of rounded p's over any key set is off by at most u_t relative -- derived,
not tuned.  floor: fp16 p's below the smallest subnormal flush to zero and subnormal ones carry an absolute error, at most 2^-24
per key (l >= 1): n_set * 2^-24 with n_set the largest key set; 1e-9 otherwise.  Where ref == 0 every key of the column is padded
or not yet visible: the output must be within floor of zero, so any leaked mass fails outright.  F, below, allows for the fp32
parts (v_exp_f32, the scale multiply, the order of the sums) and is alone the tolerance of the fp32 kernels.
"""
import functools
import math

import torch

from oracle import conformer_oracle as O

# F: measured on the REFERENCE, never on the kernels -- the worst per-element relative error of relpos_attention_core run in
# float32 on the CPU against the same call in float64, over every probe case and both patterns (full-utterance and chunked):
# `measure_F()`, recomputed and compared by tests/test_attention_probe_cpu.py.  Margin 8x: the kernels' exp is a hardware
# approximation of ~1 ulp in the log2 domain and their sums run in another order.  F stays far below u_fp16 / 8 = 6.1e-5.
# Worst observed fraction of the bound on the MI355X, per route (worst element over the table, both patterns), bf16 / fp16:
#   inference, fp32 or 16-bit q|k|v, fp32 context   0.958 / 0.928      the same with a 16-bit context   0.891 / 0.844
#   training forward: context 0.958 / 0.928, lse 0.059 / 0.059         streaming rows form              0.958 / 0.951
#   (the torch model of tests/test_attention_probe_cpu.py: 0.958 / 0.952 -- the kernels sit where their arithmetic says)
#   fp32 control (F alone): forward at 4 / 8 / 9 waves and train 0.138, lse 0.059, rows 0.138, 2 key slices 0.128, slots 0.111
F_MEASURED = 3.5e-7            # measure_F() gives 3.495e-7
F_MARGIN = 8
F = F_MARGIN * F_MEASURED

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}
DT16 = (torch.bfloat16, torch.float16)
PATTERNS = ("A", "B")

# seam -> (B, T, H, dh, lengths): the smallest shapes at which each seam of attention_mfma16.hip exists
CASES = {
    "single_row_single_key": (2, 1, 2, 8, (1, 1)),
    "first_tile_edge_one_key_utterance": (2, 33, 2, 8, (33, 1)),
    "dh16_zero_fill_mask_in_tile": (2, 97, 1, 16, (97, 64)),
    "ring_wrap_two_blocks_mask_past_edge": (2, 161, 2, 64, (161, 129)),
    "dh36_mask_mid_tile": (2, 249, 4, 36, (249, 131)),
    "three_blocks_last_partial": (2, 300, 2, 64, (300, 193)),
    "length_zero_uniform": (2, 40, 2, 8, (40, 0)),
    "no_lengths": (1, 130, 2, 32, None),
}
# streaming chunk ends: q_begin off every 32 / 128 boundary, and chunks that start exactly on one
CHUNK_ENDS = {1: [1], 33: [1, 32, 33], 40: [1, 33, 40], 97: [1, 33, 64, 97], 130: [1, 33, 64, 129, 130],
              161: [31, 32, 160, 161], 249: [1, 33, 64, 129, 190, 249], 300: [1, 33, 64, 129, 190, 257, 300],
              520: [505, 520]}
SPLIT_CASE = (2, 520, 2, 16)          # fp32 rows form with the default hint: ops._key_split gives 2 key slices


def lengths_tensor(lengths):
    return None if lengths is None else torch.tensor(lengths, dtype=torch.int64)


def visible_end_of(T, ends):
    ve = torch.empty(T, dtype=torch.long)
    start = 0
    for e in ends:
        ve[start:e] = e
        start = e
    assert start == T
    return ve


def key_columns(T, H, dh, pattern):
    """col[k, h]: the one output column of head h that key k feeds."""
    k = torch.arange(T)[:, None]
    h = torch.arange(H)[None, :]
    if pattern == "A":
        return (k + h) % dh
    assert pattern == "B"
    return (k + k // dh + h) % dh


def _quarters(shape, lim, g):
    n = int(round(4 * lim))
    return torch.randint(-n, n + 1, shape, generator=g).double() / 4.0


@functools.lru_cache(maxsize=None)
def operands(B, T, H, dh, pattern, seed=0):
    """dict q, k, v (B,T,H,dh), pos (2T-1,H,dh), u, vb (H,dh), col (T,H); float64, shared and never modified."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * T + dh + H)
    q, k = _quarters((B, T, H, dh), 1.0, g), _quarters((B, T, H, dh), 1.0, g)
    pos = _quarters((2 * T - 1, H, dh), 1.0, g)
    u, vb = _quarters((H, dh), 0.5, g), _quarters((H, dh), 0.5, g)
    col = key_columns(T, H, dh, pattern)
    v = torch.zeros(B, T, H, dh, dtype=torch.float64)
    v.scatter_(-1, col[None, :, :, None].expand(B, T, H, 1), 1.0)
    for dt in DT16:                                       # every operand of a product rounds to itself
        for t in (q + u, q + vb, q, k, pos, v):
            assert torch.equal(t.to(dt).double(), t)
    return dict(q=q, k=k, v=v, pos=pos, u=u, vb=vb, col=col, B=B, T=T, H=H, dh=dh, pattern=pattern)


def n_set(op):
    """Size of the largest key set (keys feeding one column of one head)."""
    T, H, dh = op["T"], op["H"], op["dh"]
    cnt = torch.zeros(H, dh, dtype=torch.long)
    cnt.scatter_add_(1, op["col"].t().contiguous(), torch.ones(H, T, dtype=torch.long))
    return int(cnt.max())


def device_inputs(op, dev, qkv_dtype=torch.float32):
    """qkv (B,T,3d) in qkv_dtype, pos (2T-1,d), u, v (H,dh) fp32, as the ops wrappers take them."""
    B, T, d = op["B"], op["T"], op["H"] * op["dh"]
    qkv = torch.cat([op[n].reshape(B, T, d) for n in ("q", "k", "v")], dim=-1).float().to(qkv_dtype).contiguous().to(dev)
    return qkv, op["pos"].reshape(2 * T - 1, d).float().contiguous().to(dev), op["u"].float().to(dev), op["vb"].float().to(dev)


def _core(op, lengths, visible_end, dtype):
    c = lambda t: t.to(dtype)
    return O.relpos_attention_core(c(op["q"]), c(op["k"]), c(op["v"]), c(op["pos"]), c(op["u"]), c(op["vb"]), lengths, visible_end)


@functools.lru_cache(maxsize=None)
def _reference(B, T, H, dh, pattern, lengths, ends):
    op = operands(B, T, H, dh, pattern)
    return _core(op, lengths_tensor(lengths), None if ends is None else visible_end_of(T, ends), torch.float64)


def reference(op, lengths=None, ends=None):
    """float64 softmax mass of every key set, (B,T,d): relpos_attention_core on the probe operands.  lengths: tuple or None (an
    entry 0 is the reference's uniform degenerate case: every key masked alike); ends: chunk ends (prefix rule) or None."""
    return _reference(op["B"], op["T"], op["H"], op["dh"], op["pattern"], None if lengths is None else tuple(lengths),
                      None if ends is None else tuple(ends))


def scores_log2(op, dtype=torch.float64):
    """The scaled scores in the log2 domain, (B,H,T,T), as the kernels form them: ((q+u).k + (q+v).p_{i-k}) * (inv_sqrt_dh * log2 e)."""
    B, T, H, dh = op["B"], op["T"], op["H"], op["dh"]
    c = lambda t: t.to(dtype)
    content = torch.einsum("bihc,bkhc->bhik", c(op["q"] + op["u"]), c(op["k"]))
    full = torch.einsum("bihc,jhc->bhij", c(op["q"] + op["vb"]), c(op["pos"]))
    i = torch.arange(T)[:, None]
    k = torch.arange(T)[None, :]
    s = content + full.gather(-1, ((T - 1) - (i - k)).expand(B, H, T, T))
    scale2 = torch.tensor(1.0 / math.sqrt(dh), dtype=dtype) * torch.tensor(1.4426950408889634, dtype=dtype)
    return s * scale2


def key_visible(op, lengths=None, ends=None):
    """(B,1,T,T) bool: key k takes part in row i's softmax.  lengths[b] == 0: every key (the uniform case, scores forced to 0)."""
    B, T = op["B"], op["T"]
    ok = torch.ones(B, 1, T, T, dtype=torch.bool)
    if lengths is not None:
        L = lengths_tensor(lengths)
        L = torch.where(L <= 0, torch.full_like(L, T), L)
        ok &= (torch.arange(T)[None, :] < L[:, None])[:, None, None, :]
    if ends is not None:
        ok &= (torch.arange(T)[None, :] < visible_end_of(T, ends)[:, None])[None, None]
    return ok


def reference_lse(op, lengths=None):
    """float64 natural log-sum-exp of the scaled, masked scores, (B,H,T); rows of an utterance of length 0: log T."""
    s = scores_log2(op) * math.log(2.0)
    if lengths is not None:
        uniform = lengths_tensor(lengths) <= 0
        s = torch.where(uniform[:, None, None, None], torch.zeros_like(s), s)
    s = s.masked_fill(~key_visible(op, lengths), -math.inf)
    return torch.logsumexp(s, dim=-1)


def measure_F():
    """Worst per-element relative error of the float32 reference against the float64 one over every probe case."""
    worst = 0.0
    for B, T, H, dh, lengths in list(CASES.values()) + [SPLIT_CASE + (None,)]:
        for pattern in PATTERNS:
            op = operands(B, T, H, dh, pattern)
            variants = [(lengths, None)]
            if lengths is None or min(lengths) > 0:
                variants.append((None, CHUNK_ENDS[T]))
            for L, ends in variants:
                ref = reference(op, L, ends)
                got = _core(op, lengths_tensor(L), None if ends is None else visible_end_of(T, ends), torch.float32).double()
                nz = ref > 0
                worst = max(worst, float(((got - ref).abs()[nz] / ref[nz]).max()))
    return worst


def bound(ref, dtype, ctx16, nset):
    """The per-element bound for a context computed with P in `dtype` (torch.float32: the fp32 kernels, F alone)."""
    u = U[dtype]
    rel = (2 * u + u * u + F) if ctx16 else (u + F)
    floor = nset * 2.0 ** -24 if dtype == torch.float16 else 1e-9
    return rel * ref + floor


def worst_fraction(got, ref, bnd):
    """max |got - ref| / bound and its flat index (NaN counts as infinite)."""
    frac = (got.double() - ref).abs() / bnd
    frac = torch.where(torch.isnan(frac), torch.full_like(frac, math.inf), frac)
    idx = int(frac.argmax())
    return float(frac.flatten()[idx]), idx


def check(got, ref, op, dtype, ctx16=False, rows=None, what=""):
    """Assert the bound on every element of got (B,T,d) (rows: only query rows [rows[0], rows[1])); returns the worst fraction of
    the bound.  The failure message names the worst element and the keys of its column: it should point at a tile."""
    B, T, H, dh = op["B"], op["T"], op["H"], op["dh"]
    got = got.detach().cpu().double().reshape(B, T, H * dh)
    lo, hi = (0, T) if rows is None else rows
    g, r = got[:, lo:hi], ref[:, lo:hi]
    bnd = bound(r, dtype, ctx16, n_set(op))
    frac, idx = worst_fraction(g, r, bnd)
    if not frac <= 1.0:
        b, rem = divmod(idx, (hi - lo) * H * dh)
        i, rem = divmod(rem, H * dh)
        h, c = divmod(rem, dh)
        keys = torch.nonzero(op["col"][:, h] == c).flatten().tolist()
        raise AssertionError(f"{what}: pattern {op['pattern']} batch {b} query row {lo + i} head {h} column {c} (keys {keys}): got "
                             f"{float(g[b, i, h * dh + c])!r}, reference {float(r[b, i, h * dh + c])!r}, bound "
                             f"{float(bnd[b, i, h * dh + c]):.3e} ({frac:.1f}x)")
    return frac


def check_lse(got, op, lengths, what=""):
    """|lse - ref| <= F * max(1, |lse|) per row (P's rounding does not enter the log-sum-exp); returns the worst fraction."""
    ref = reference_lse(op, lengths)
    frac, idx = worst_fraction(got.detach().cpu().double(), ref, F * ref.abs().clamp(min=1.0))
    if not frac <= 1.0:
        H, T = op["H"], op["T"]
        b, rem = divmod(idx, H * T)
        h, i = divmod(rem, T)
        raise AssertionError(f"{what}: lse batch {b} head {h} query row {i}: got {float(got[b, h, i])!r}, reference "
                             f"{float(ref[b, h, i])!r} ({frac:.1f}x)")
    return frac


# ---- torch model of the 16-bit kernel's arithmetic, with injectable structural faults (tests/test_attention_probe_cpu.py)

FAULTS = ("dropped_pair", "pos_off_by_one_in_tile", "mask_admits_key_L", "keys_exchanged")


def kernel_model(op, lengths, dtype, ctx16=False, fault=None, ends=None):
    """fp32 scores (exact for the probe operands), fp32 exp2 against the row maximum, the row sum taken from the unrounded
    probabilities, P rounded to `dtype` before P.V, one fp32 divide; optionally the context rounded to `dtype`; `ends`: the chunked (prefix-rule) evaluation.  Faults:
      dropped_pair            one (row, key) pair contributes nothing to P.V           (b 0, h 0, row T//2, key (T//2)//2)
      pos_off_by_one_in_tile  the positional term of one 32-key tile uses row j+1      (the last full tile, every row)
      mask_admits_key_L       the padding mask admits key lengths[b]                   (every b with 0 < lengths[b] < T)
      keys_exchanged          keys 5 and 13 change places in P.V                       (b 0, h 0, row T//2: one lane's registers)
    Returns (B,T,d) float64, or None where the fault does not exist at this shape."""
    B, T, H, dh = op["B"], op["T"], op["H"], op["dh"]
    s = scores_log2(op, torch.float32)
    if fault == "pos_off_by_one_in_tile":
        if T < 2:
            return None
        k0 = 32 * max(0, min(T, 10 ** 9 if lengths is None else max(lengths)) // 32 - 1)
        k1 = min(k0 + 32, T)
        q, pp, vb = op["q"].float(), op["pos"].float(), op["vb"].float()
        full = torch.einsum("bihc,jhc->bhij", q + vb, pp)
        i = torch.arange(T)[:, None]
        k = torch.arange(T)[None, :]
        j1 = ((T - 1) - (i - k) + 1).clamp(max=2 * T - 2)
        content = torch.einsum("bihc,bkhc->bhik", q + op["u"].float(), op["k"].float())
        scale2 = torch.tensor(1.0 / math.sqrt(dh)) * torch.tensor(1.4426950408889634)
        wrong = (content + full.gather(-1, j1.expand(B, H, T, T))) * scale2
        s = s.clone()
        s[..., k0:k1] = wrong[..., k0:k1]
    ok = key_visible(op, lengths, ends)
    if fault == "mask_admits_key_L":
        hit = [b for b in range(B) if lengths is not None and 0 < lengths[b] < T]
        if not hit:
            return None
        ok = ok.clone()
        for b in hit:
            ok[b, :, :, lengths[b]] = True
    if lengths is not None:
        uniform = lengths_tensor(lengths) <= 0
        s = torch.where(uniform[:, None, None, None], torch.zeros_like(s), s)
    s = s.masked_fill(~ok, -math.inf)
    p = torch.exp2(s - s.max(dim=-1, keepdim=True).values)
    l = p.sum(-1)
    p16 = p.to(dtype).float()
    if fault == "dropped_pair":
        p16[0, 0, T // 2, (T // 2) // 2] = 0.0
    if fault == "keys_exchanged":
        if T < 14:
            return None
        p16[0, 0, T // 2, [5, 13]] = p16[0, 0, T // 2, [13, 5]]
    o = torch.einsum("bhik,bkhc->bihc", p16, op["v"].float()) / l.permute(0, 2, 1)[..., None]
    if ctx16:
        o = o.to(dtype).float()
    return o.reshape(B, T, H * dh).double()
