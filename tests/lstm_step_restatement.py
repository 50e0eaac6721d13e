"""Float64, teacher-forced restatement of ONE step of the decoder LSTM (helper, not a test file; tests/test_lstm_step_{cpu,gpu}.py).

A free-running float64 LSTM drifts away from the 16-bit kernels: they round h_t (and dG_t) to 16 bits between steps, and only a
whole-tensor rel_l2 of 1e-2 survives T such steps.  The replay here never free-runs.  Step t takes the DEVICE's own previous
outputs as its state (y[:, t-1] and cells[:, t-1]; dG[:, t+1] in the backward), rounds them as the kernel rounds them, and
computes that one step in float64: every remaining difference is the fp32 arithmetic of one step, ~1e-6 per element, and the
bound is a statement per element of gates, cells, y, dG and the final dc.

  forward step t    pre = gx[:, t] + r(h_prev) @ r(W_hh).T       r = round trip through the 16-bit type (identity for fp32)
                    i|f|g|o = sigmoid, sigmoid, tanh, sigmoid;  c_t = f c_prev + i g;  h_t = o tanh(c_t)
                    a frame at or beyond lengths[b]: y = 0, gates = 0, cells[t] == c_prev EXACTLY
  backward step t   dh = dy[:, t] + r(dG_dev[:, t+1]) @ r(W_hh);  do = dh tanh(c_t) o(1-o);  dc = dh o (1 - tanh^2 c_t) + dc_next
                    di = dc g i(1-i);  df = dc c_{t-1} f(1-f);  dg = dc i (1-g^2);  dc_next = dc f
                    dc_next is carried by the replay itself in float64 (never rounded to 16 bits: it cannot drift)
                    a dead frame: dG = 0 and dc = 0 EXACTLY

Bound, per element:  |dev - ref| <= E_MARGIN * E_*_MEASURED * max(1, |ref|).  E is measured on the CPU, never on the kernels:
`emulate_fp32` is the same recurrence in torch float32 with the kernels' formulas (1/(1+exp2(-x log2 e)), 1 - 2/(exp2(2x log2 e)+1),
the argument product rounded to fp32) and -- backward -- the whole T-step fp32 dc chain, and `measure_E()` is its worst distance
from the replay over every case shape and dtype below.  Margin 8x (the convention of F_MARGIN in tests/attention_probe.py): the
kernels' v_exp_f32 and the MFMA summation order are only approximated by the CPU emulation.  gx is a standard normal clamped to
+-3 and the states are O(1), so no pre-activation leaves the range over which E is measured.  The emulation uses elementwise IEEE
operations only (`_dot32`, `_exp2_32`): with a BLAS product and a vectorised fp32 exp2 the forward figure was 9.1e-7 on one host
and 4.1e-7 on another, and a recorded constant could not hold on both.
"""
import functools
import math

import torch

E_FWD_MEASURED = 4.2e-7         # measure_E() gives 4.182e-7 (a gate of the carried fp16 case, H=656)
E_BWD_MEASURED = 2.4e-7         # measure_E() gives 2.324e-7
E_MARGIN = 8
E_FWD = E_MARGIN * E_FWD_MEASURED
E_BWD = E_MARGIN * E_BWD_MEASURED

LOG2E = 1.4426950408889634
DT16 = (torch.bfloat16, torch.float16)
GATES = "ifgo"

# route -> (hidden units, utterances) a workgroup owns and the threads of its gate stage per utterance (tid = row * n + unit)
ROUTES = {
    "fwd_row": (4, 16, 4), "fwd_frag": (4, 16, 4), "fwd_16": (8, 32, 8),
    "bwd_row": (16, 16, 16), "bwd_frag": (16, 16, 16), "bwd_16": (16, 16, 16),
}
# The smallest shapes at which each seam of a contraction loop exists: route -> (dtypes, H list, B list, T).  One pass of the
# waves covers H = 320 (fp32 forward: 4 waves x 5 chunks of 16), 640 (16-bit forward: 4 x 10), 160 (fp32 BPTT: 8 x 5 chunks over
# 4H), 320 (16-bit BPTT: 8 x 10); the largest H of each row runs a partial second pass (clamped loads, guarded tail).
FWD_CASES = {
    "fwd_row": ((torch.float32,), (20, 324), (1, 17), 3),
    "fwd_frag": ((torch.float32,), (16, 320, 336), (17, 33), 3),
    "fwd_16": (DT16, (16, 48, 640, 656), (1, 33), 3),
}
BWD_CASES = {
    "bwd_row": ((torch.float32,), (20, 164), (17,), 4),
    "bwd_frag": ((torch.float32,), (16, 160, 176), (17, 33), 4),
    "bwd_16": (DT16, (16, 320, 336), (17, 33), 4),
}
# carried forward: the H with the partial second pass, a partial last utterance block, chunks of 2 and 1 frames
CARRY_CASES = {"fwd_row": ((torch.float32,), 324, 17), "fwd_frag": ((torch.float32,), 336, 17), "fwd_16": (DT16, 656, 33)}
CARRY_CHUNKS = (2, 1)


def cases(table):
    """Every (route, dtype, H, B, T) of a case table."""
    return [(route, dt, H, B, T) for route, (dts, Hs, Bs, T) in table.items() for dt in dts for H in Hs for B in Bs]


def carry_cases():
    return [(route, dt, H, B) for route, (dts, H, B) in CARRY_CASES.items() for dt in dts]


def lengths_for(B, T):
    """Unsorted lengths with one equal to T, one equal to 1, and the utterance of the last (partial) block ending early."""
    if B == 1:
        return [T]
    L = [(5 * b + 2) % T + 1 for b in range(B)]
    L[1], L[2 % B], L[B - 1] = T, 1, max(1, T - 1)
    if B == 2:
        L = [1, T]
    return L


def carry_lengths(B, T):
    """Per-slot frame counts of one chunk: 0 (the slot keeps its state), partial and full, the last slot ending early."""
    L = [(T, 0, max(1, T - 1))[(b + T) % 3] for b in range(B)]
    L[B - 1] = T - 1
    return L


def make_case(H, B, T, seed=0, state=False, lengths=None):
    """Operands of one case (CPU fp32): gx ~ N(0,1) clamped to +-3, W_hh uniform in +-1/sqrt(H) (nn.LSTM's init), dy ~ N(0,1),
    and an O(1) (h, c) state whose values are not representable in 16 bits."""
    g = torch.Generator().manual_seed(1000 * H + 10 * B + T + seed)
    case = {"H": H, "B": B, "T": T,
            "gx": torch.randn(B, T, 4 * H, generator=g).clamp(-3, 3),
            "w_hh": (torch.rand(4 * H, H, generator=g) * 2 - 1) / math.sqrt(H),
            "dy": torch.randn(B, T, H, generator=g),
            "lengths": lengths_for(B, T) if lengths is None else list(lengths), "h0": None, "c0": None}
    if state:
        case["h0"] = (torch.rand(B, H, generator=g) * 2 - 1) * 0.8
        case["c0"] = torch.randn(B, H, generator=g)
        assert not torch.equal(case["h0"], case["h0"].bfloat16().float()) and not torch.equal(case["h0"], case["h0"].half().float())
    return case


def r(x, dtype):
    """x (fp32) as the kernel exchanges it: a round trip through the 16-bit type, the identity for fp32; float64 result."""
    x = x.float()
    return (x if dtype == torch.float32 else x.to(dtype).float()).double()


def live_mask(lengths, B, T):
    """(B, T) bool: frame t of utterance b is inside the utterance."""
    if lengths is None:
        return torch.ones(B, T, dtype=torch.bool)
    return torch.arange(T)[None, :] < torch.as_tensor(lengths, dtype=torch.int64).cpu()[:, None]


# ---- structural faults a kernel could have, applied to the replay ------------------------------------------------------------
FAULTS = ("tail_step_dropped", "k_columns_exchanged", "utterance_rows_exchanged", "gate_row_exchanged", "buffer_parity_wrong",
          "exchange_unrounded", "finished_state_not_frozen")


def fault_applies(fault, direction, dtype, B, lengths=None, T=None):
    """Whether `fault` changes anything at a case: an unrounded exchange needs a 16-bit mode, exchanged rows two utterances, an
    unfrozen state a finished utterance -- and the forward: the backward multiplies every term of a dead frame by one of its
    saved gates, which the forward stored as 0, so an unfrozen backward step computes the same zeros."""
    if fault == "exchange_unrounded":
        return dtype != torch.float32
    if fault == "utterance_rows_exchanged":
        return B >= 2
    if fault == "finished_state_not_frozen":
        return direction == "fwd" and lengths is not None and min(lengths) < T
    return True


def _exchange_rows(B, lengths):
    """The longest utterance and its neighbour in the same 16-row block."""
    b = 0 if lengths is None else max(range(B), key=lambda i: lengths[i])
    return [b, b ^ 1] if (b ^ 1) < B else [b, b - 1]


def _faulty_operand(x, w_cols, fault, B, lengths):
    """The exchanged operand x (B, K) and a mask over W's contraction index (K) under a contraction fault."""
    K = x.shape[1]
    if fault == "tail_step_dropped":
        w_cols = w_cols.clone()
        w_cols[16 * ((K - 1) // 16):] = 0.0
    elif fault == "k_columns_exchanged":
        x = x.clone()
        x[:, [0, 8]] = x[:, [8, 0]]
    elif fault == "utterance_rows_exchanged":
        x = x.clone()
        rows = _exchange_rows(B, lengths)
        x[rows] = x[rows[::-1]]
    return x, w_cols


def _gate_rows(w, fault):
    if fault == "gate_row_exchanged":
        H = w.shape[1]
        w = w.clone()
        w[[0, H]] = w[[H, 0]]
    return w


# ---- the replay ---------------------------------------------------------------------------------------------------------------
def replay_forward(case, dtype, y_dev=None, cells_dev=None, state=None, fault=None):
    """Expected (gates (B,T,4H), cells (B,T,H), y (B,T,H)) in float64, step t computed from the device's y[:, t-1] and
    cells[:, t-1] (step 0: from `state` = (h, c) before the call, or zeros).  With y_dev = cells_dev = None the replay is fed its
    own outputs instead (a free-running float64 LSTM: what the oracle computes when dtype is float32)."""
    gx, H, B, T, lengths = case["gx"].double(), case["H"], case["B"], case["T"], case["lengths"]
    w = _gate_rows(r(case["w_hh"], dtype), fault)
    live = live_mask(lengths, B, T)
    round_h = (lambda h: h.double()) if fault == "exchange_unrounded" else (lambda h: r(h, dtype))
    gates, cells, y = gx.new_zeros(B, T, 4 * H), gx.new_zeros(B, T, H), gx.new_zeros(B, T, H)
    h_init = gx.new_zeros(B, H) if state is None else state[0].detach().cpu().float()
    c_init = gx.new_zeros(B, H) if state is None else state[1].detach().cpu().double()
    self_fed = y_dev is None
    assert not self_fed or dtype == torch.float32        # (its own float64 h has no 16-bit exchange to model)
    if not self_fed:
        y_dev, cells_dev = y_dev.detach().cpu().float(), cells_dev.detach().cpu().float()
    h_own, c_own = h_init.double(), c_init
    for t in range(T):
        if self_fed:
            h_prev, c_prev, h_prev2 = h_own, c_own, None
        else:
            h_prev = round_h(y_dev[:, t - 1] if t > 0 else h_init)
            h_prev2 = round_h(y_dev[:, t - 2] if t > 1 else h_init)
            c_prev = (cells_dev[:, t - 1] if t > 0 else c_init).double()
        if fault == "buffer_parity_wrong":
            h_prev = h_prev2
        h_prev, kmask = _faulty_operand(h_prev, torch.ones(H, dtype=torch.float64), fault, B, lengths)
        pre = gx[:, t] + h_prev @ (w * kmask).t()
        i, f, g, o = pre[:, :H].sigmoid(), pre[:, H:2 * H].sigmoid(), pre[:, 2 * H:3 * H].tanh(), pre[:, 3 * H:].sigmoid()
        c = f * c_prev + i * g
        h = o * c.tanh()
        lv = live[:, t, None] if fault != "finished_state_not_frozen" else torch.ones(B, 1, dtype=torch.bool)
        gates[:, t] = torch.where(lv, torch.cat([i, f, g, o], 1), torch.zeros_like(pre))
        cells[:, t] = torch.where(lv, c, c_prev)
        y[:, t] = torch.where(lv, h, torch.zeros_like(h))
        h_own, c_own = torch.where(lv, h, h_own), cells[:, t]
    return gates, cells, y


def replay_backward(case, dtype, gates, cells, dG_dev=None, fault=None):
    """Expected (dG (B,T,4H), final dc (B,H)) in float64 from the forward's saved gates and cells, step t computed from the
    device's dG[:, t+1]; dc_next is the replay's own, in float64.  dG_dev = None: fed its own dG (float64 BPTT)."""
    H, B, T, lengths = case["H"], case["B"], case["T"], case["lengths"]
    dy = case["dy"].double()
    gates, cells = gates.detach().cpu().double(), cells.detach().cpu().double()
    w = _gate_rows(r(case["w_hh"], dtype), fault)
    live = live_mask(lengths, B, T)
    round_g = (lambda x: x.double()) if fault == "exchange_unrounded" else (lambda x: r(x, dtype))
    self_fed = dG_dev is None
    assert not self_fed or dtype == torch.float32
    if not self_fed:
        dG_dev = dG_dev.detach().cpu().float()
    dG = dy.new_zeros(B, T, 4 * H)
    dc_next = dy.new_zeros(B, H)
    zero = dy.new_zeros(B, 4 * H)
    for t in range(T - 1, -1, -1):
        ahead = t + 2 if fault == "buffer_parity_wrong" else t + 1
        if self_fed:
            g_next = dG[:, ahead] if ahead < T else zero
        else:
            g_next = round_g(dG_dev[:, ahead]) if ahead < T else zero
        g_next, kmask = _faulty_operand(g_next, torch.ones(4 * H, dtype=torch.float64), fault, B, lengths)
        dh = dy[:, t] + g_next @ (w * kmask[:, None])
        i, f, g, o = gates[:, t, :H], gates[:, t, H:2 * H], gates[:, t, 2 * H:3 * H], gates[:, t, 3 * H:]
        th = cells[:, t].tanh()
        c_prev = cells[:, t - 1] if t > 0 else torch.zeros_like(th)
        dc = dh * o * (1 - th * th) + dc_next
        step = torch.cat([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * th * o * (1 - o)], 1)
        lv = live[:, t, None] if fault != "finished_state_not_frozen" else torch.ones(B, 1, dtype=torch.bool)
        dG[:, t] = torch.where(lv, step, torch.zeros_like(step))
        dc_next = torch.where(lv, dc * f, torch.zeros_like(dc))
    return dG, dc_next


def faulty(direction, case, dtype, fault, **kw):
    """The replay of `direction` ("fwd" / "bwd") with one of FAULTS applied: what a kernel with that error would return for the
    same previous outputs."""
    assert fault in FAULTS
    return (replay_forward if direction == "fwd" else replay_backward)(case, dtype, fault=fault, **kw)


# ---- the yardstick: the same recurrence in fp32 with the kernels' formulas -----------------------------------------------------
def _exp2_32(x):
    """fp32 exp2 of an fp32 argument, rounded from the float64 value: the same bits on every machine (a vectorised fp32 exp2 may
    differ in the last place between instruction sets)."""
    return torch.exp2(x.double()).float()


def _sig32(x):
    return 1.0 / (1.0 + _exp2_32(-x * LOG2E))


def _tanh32(x):
    return 1.0 - 2.0 / (_exp2_32(2.0 * x * LOG2E) + 1.0)


def _dot32(x, w):
    """x (B,K) @ w (N,K).T with fp32 accumulation in a fixed order: one rounding per 4 products (a 16x16x4 MFMA step), k ascending.
    Only elementwise IEEE operations (the products of fp32 values are exact in float64), so every machine gives the same bits; a
    BLAS call sums in an order that depends on the machine and its thread count, and E would move with it."""
    xt, wt = x.double().t().contiguous(), w.double().t().contiguous()           # k-major: the slices below are contiguous
    acc = x.new_zeros(x.shape[0], w.shape[0])
    for k0 in range(0, xt.shape[0], 16):
        p = xt[k0:k0 + 16, :, None] * wt[k0:k0 + 16, None, :]
        for j in range(0, p.shape[0], 4):
            acc = (acc.double() + (((p[j] + p[j + 1]) + p[j + 2]) + p[j + 3])).float()
    return acc


def _r32(x, dtype):
    return x if dtype == torch.float32 else x.to(dtype).float()


def emulate_fp32(direction, case, dtype, state=None, gates=None, cells=None):
    """The recurrence in torch float32 on the CPU, exchanging h_t / dG_t through `dtype` as the kernels do.  "fwd": returns
    (gates, cells, y); "bwd" (from the saved gates and cells): (dG, dc) with the whole T-step fp32 dc chain.  The yardstick of
    the tolerance, not the code under test."""
    H, B, T, lengths = case["H"], case["B"], case["T"], case["lengths"]
    w = _r32(case["w_hh"], dtype)
    live = live_mask(lengths, B, T)
    if direction == "fwd":
        gx = case["gx"]
        out_g, out_c, y = gx.new_zeros(B, T, 4 * H), gx.new_zeros(B, T, H), gx.new_zeros(B, T, H)
        h_prev = gx.new_zeros(B, H) if state is None else state[0].float()
        c_prev = gx.new_zeros(B, H) if state is None else state[1].float()
        for t in range(T):
            pre = gx[:, t] + _dot32(_r32(h_prev, dtype), w)
            i, f, g, o = _sig32(pre[:, :H]), _sig32(pre[:, H:2 * H]), _tanh32(pre[:, 2 * H:3 * H]), _sig32(pre[:, 3 * H:])
            c = f * c_prev + i * g
            h = o * _tanh32(c)
            lv = live[:, t, None]
            out_g[:, t] = torch.where(lv, torch.cat([i, f, g, o], 1), torch.zeros_like(pre))
            out_c[:, t] = torch.where(lv, c, c_prev)
            y[:, t] = torch.where(lv, h, torch.zeros_like(h))
            h_prev, c_prev = torch.where(lv, h, h_prev), out_c[:, t]
        return out_g, out_c, y
    dy, wt = case["dy"], w.t().contiguous()
    dG, dc_next = dy.new_zeros(B, T, 4 * H), dy.new_zeros(B, H)
    for t in range(T - 1, -1, -1):
        dh = dy[:, t] + (_dot32(_r32(dG[:, t + 1], dtype), wt) if t + 1 < T else 0.0)
        i, f, g, o = gates[:, t, :H], gates[:, t, H:2 * H], gates[:, t, 2 * H:3 * H], gates[:, t, 3 * H:]
        th = _tanh32(cells[:, t])
        c_prev = cells[:, t - 1] if t > 0 else torch.zeros_like(th)
        dc = dh * o * (1.0 - th * th) + dc_next
        step = torch.cat([dc * g * i * (1.0 - i), dc * c_prev * f * (1.0 - f), dc * i * (1.0 - g * g), dh * th * o * (1.0 - o)], 1)
        lv = live[:, t, None]
        dG[:, t] = torch.where(lv, step, torch.zeros_like(step))
        dc_next = torch.where(lv, dc * f, torch.zeros_like(dc))
    return dG, dc_next


def _distance(got, ref):
    return float(((got.double() - ref).abs() / ref.abs().clamp(min=1.0)).max())


@functools.lru_cache(maxsize=None)
def emulated_runs():
    """direction -> [(label, case, dtype, replay kwargs, the emulation's outputs, the clean replay of them)] over every case shape
    and dtype, carried forward cases included: the emulation plays the device.  Computed once per process; read-only."""
    out = {"fwd": [], "bwd": []}
    for route, dt, H, B, T in cases(FWD_CASES):
        case = make_case(H, B, T)
        eg, ec, ey = emulate_fp32("fwd", case, dt)
        kw = dict(y_dev=ey, cells_dev=ec)
        out["fwd"].append((f"{route} H={H} B={B}", case, dt, kw, (eg, ec, ey), replay_forward(case, dt, **kw)))
    for route, dt, H, B in carry_cases():
        T = CARRY_CHUNKS[0]
        case = make_case(H, B, T, state=True, lengths=carry_lengths(B, T))
        st = (case["h0"], case["c0"])
        eg, ec, ey = emulate_fp32("fwd", case, dt, state=st)
        kw = dict(y_dev=ey, cells_dev=ec, state=st)
        out["fwd"].append((f"{route} carried H={H} B={B}", case, dt, kw, (eg, ec, ey), replay_forward(case, dt, **kw)))
    for route, dt, H, B, T in cases(BWD_CASES):
        case = make_case(H, B, T)
        eg, ec, _ = emulate_fp32("fwd", case, dt)
        dG, dc = emulate_fp32("bwd", case, dt, gates=eg, cells=ec)
        kw = dict(gates=eg, cells=ec, dG_dev=dG)
        out["bwd"].append((f"{route} H={H} B={B}", case, dt, kw, (dG, dc), replay_backward(case, dt, **kw)))
    return out


def measure_E():
    """(E_fwd, E_bwd): the largest |emulation - replay| / max(1, |replay|) over every case shape and dtype, forward quantities
    (gates, cells, y; carried cases included) and backward ones (dG, final dc)."""
    runs = emulated_runs()
    return tuple(max(_distance(a, b) for _, _, _, _, emu, clean in runs[d] for a, b in zip(emu, clean)) for d in ("fwd", "bwd"))


# ---- the check ----------------------------------------------------------------------------------------------------------------
def owner(route, b, unit):
    """((workgroup x, y), wave) of the gate-stage thread that writes element (utterance b, hidden unit) on `route`."""
    units, rows, per_row = ROUTES[route]
    return (unit // units, b // rows), ((b % rows) * per_row + unit % units) >> 6


def worst_fraction(got, ref, E, exact=None):
    """max |got - ref| / (E max(1, |ref|)) and its flat index; where `exact` any difference (and any NaN) counts as infinite."""
    diff = (got.double() - ref).abs()
    frac = diff / (E * ref.abs().clamp(min=1.0))
    if exact is not None:
        frac = torch.where(exact.expand_as(frac), torch.where(diff == 0, torch.zeros_like(frac), torch.full_like(frac, math.inf)), frac)
    frac = torch.where(torch.isnan(frac), torch.full_like(frac, math.inf), frac)
    idx = int(frac.argmax())
    return float(frac.flatten()[idx]), idx


def check(quantity, got, ref, E, route, exact=None, what=""):
    """Assert |got - ref| <= E max(1, |ref|) on every element of got (B,T,N) or (B,N), N = H or 4H (gate-major), and equality
    where `exact` (B,T,1); returns the worst fraction of the bound.  A failure names the element and the thread that owns it."""
    got = got.detach().cpu()
    if got.dim() == 2:
        got, ref = got[:, None], ref[:, None]
    assert got.shape == ref.shape, (quantity, tuple(got.shape), tuple(ref.shape))
    frac, idx = worst_fraction(got, ref, E, exact)
    if not frac <= 1.0:
        B, T, N = ref.shape
        H = N if quantity in ("cells", "y", "dc", "h_state", "c_state") else N // 4
        b, rem = divmod(idx, T * N)
        t, n = divmod(rem, N)
        gate, unit = divmod(n, H)
        (wx, wy), wave = owner(route, b, unit)
        raise AssertionError(f"{what}: {quantity} step {t} utterance {b} unit {unit}" + (f" gate {GATES[gate]}" if N != H else "") +
                             f" (workgroup ({wx}, {wy}) wave {wave} of {route}): got {float(got[b, t, n])!r}, expected "
                             f"{float(ref[b, t, n])!r}, bound {E * max(1.0, abs(float(ref[b, t, n]))):.3e} ({frac:.1f}x)")
    return frac


def check_forward(case, dtype, route, gates, cells, y, state=None, what=""):
    """Every step of a forward call against the replay fed with the call's own y and cells; the worst fraction of the bound."""
    rg, rc, ry = replay_forward(case, dtype, y, cells, state=state)
    dead = ~live_mask(case["lengths"], case["B"], case["T"])[:, :, None]
    return max(check("gates", gates, rg, E_FWD, route, dead, what), check("cells", cells, rc, E_FWD, route, dead, what),
               check("y", y, ry, E_FWD, route, dead, what))


def check_backward(case, dtype, route, gates, cells, dG, dc, what=""):
    """Every step of a BPTT call against the replay fed with the call's own dG; the worst fraction of the bound."""
    rG, rdc = replay_backward(case, dtype, gates, cells, dG)
    dead = ~live_mask(case["lengths"], case["B"], case["T"])[:, :, None]
    return max(check("dG", dG, rG, E_BWD, route, dead, what), check("dc", dc, rdc, E_BWD, route, None, what))
