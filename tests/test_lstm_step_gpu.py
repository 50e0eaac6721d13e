"""Every LSTM recurrence kernel, per element and one step at a time, against the float64 teacher-forced replay of
tests/lstm_step_restatement.py: gates, cells and y of every forward step, dG of every BPTT step and the final dc, at the smallest
shapes at which each seam of the contraction loops exists (idle waves, a ragged last chunk, exactly one pass of the waves, a
partial second pass with its clamped loads and guarded tail) with a partial last utterance block and unsorted ragged lengths.
The bound is E_MARGIN x the fp32 error measured on the CPU emulation (tests/test_lstm_step_cpu.py), ~1e-6 per element; the
free-run rel_l2 < 1e-2 of the other LSTM tests stays the end-to-end check.

Worst fraction of the bound on the MI355X, per route (worst element over the route's shapes; bf16 / fp16 where 16-bit):
  forward   row-major 0.065, fragment 0.079, 16-bit 0.071 / 0.069      carried   row-major 0.071, fragment 0.075, 16-bit 0.066 / 0.071
  BPTT      row-major 0.116, fragment 0.143, 16-bit 0.215 / 0.193
(the CPU emulation the bound is measured on sits at 0.125 by construction).  Before its 16-bit dG copy was made to round the stored
fp32 value, the fp16 BPTT kernel was at 1.2 at H=320 B=33: the compiler folded the last multiply of each dG into the conversion."""
import pytest
import torch

from tests import lstm_step_restatement as R
from tests.util import Calls

pytestmark = pytest.mark.gpu

NAME = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
ENTRY = {"fwd_row": "cfm_lstm_fwd_f32", "fwd_frag": "cfm_lstm_fwd_frag_f32", "fwd_16": "cfm_lstm_fwd_mfma16_f32",
         "bwd_row": "cfm_lstm_bwd_f32", "bwd_frag": "cfm_lstm_bwd_frag_f32", "bwd_16": "cfm_lstm_bwd_mfma16_f32"}
CARRY_ENTRY = {"fwd_row": "cfm_lstm_fwd_carry_f32", "fwd_frag": "cfm_lstm_fwd_frag_carry_f32", "fwd_16": "cfm_lstm_fwd_mfma16_carry_f32"}
ENTRIES = tuple(ENTRY.values()) + tuple(CARRY_ENTRY.values())


def _id(case):
    return f"{case[0]}-{NAME[case[1]]}-" + "-".join(str(v) for v in case[2:])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _prec(dtype):
    from conformer_amd import ops
    return ops.precision({torch.float32: ops.PREC_F32, torch.bfloat16: ops.PREC_BF16, torch.float16: ops.PREC_FP16}[dtype])


def _forward(dev, case, dtype, entry, w_hh=None, state=None):
    """(y, gates, cells) of ops.lstm_recurrence on the device under `dtype`'s precision mode; asserts the entry that ran."""
    from conformer_amd import ops
    w_hh = case["w_hh"].to(dev) if w_hh is None else w_hh
    L = torch.tensor(case["lengths"], dtype=torch.int64, device=dev)
    with Calls(*ENTRIES) as seen, _prec(dtype):
        y, gates, cells = ops.lstm_recurrence(case["gx"].to(dev), w_hh, L, save=True, state=state)
    assert seen == {entry}, seen
    return y, gates, cells


@pytest.mark.parametrize("route,dtype,H,B,T", R.cases(R.FWD_CASES), ids=[_id(c) for c in R.cases(R.FWD_CASES)])
def test_forward_every_step_per_element(dev, route, dtype, H, B, T):
    case = R.make_case(H, B, T)
    L = case["lengths"]
    assert B == 1 or (max(L) == T and min(L) == 1 and L[B - 1] < T and L != sorted(L, reverse=True) and (B - 1) % 16 == 0)
    y, gates, cells = _forward(dev, case, dtype, ENTRY[route])
    frac = R.check_forward(case, dtype, route, gates, cells, y, what=f"{route} {NAME[dtype]} H={H} B={B}")
    print(f"{route} {NAME[dtype]} H={H} B={B}: worst fraction of the bound {frac:.3f}")


@pytest.mark.parametrize("route,dtype,H,B,T", R.cases(R.BWD_CASES), ids=[_id(c) for c in R.cases(R.BWD_CASES)])
def test_bptt_every_step_per_element(dev, route, dtype, H, B, T):
    from conformer_amd import ops
    case = R.make_case(H, B, T)
    L = case["lengths"]
    assert max(L) == T and min(L) == 1 and L[B - 1] < T and L != sorted(L, reverse=True) and (B - 1) % 16 == 0
    w_hh = case["w_hh"].to(dev)
    _, gates, cells = _forward(dev, case, dtype, ENTRY["fwd" + route[3:]], w_hh=w_hh)        # the matching forward's activations
    with Calls(*ENTRIES) as seen, _prec(dtype):
        dG, dc = ops.lstm_bptt(w_hh, gates, cells, case["dy"].to(dev), torch.tensor(L, dtype=torch.int64, device=dev))
    assert seen == {ENTRY[route]}, seen
    frac = R.check_backward(case, dtype, route, gates, cells, dG, dc, what=f"{route} {NAME[dtype]} H={H} B={B}")
    assert (dG.cpu()[~R.live_mask(L, B, T)] == 0).all()                                       # dead frames carry no gradient, exactly
    print(f"{route} {NAME[dtype]} H={H} B={B}: worst fraction of the bound {frac:.3f}")


@pytest.mark.parametrize("route,dtype,H,B", R.carry_cases(), ids=[_id(c) for c in R.carry_cases()])
def test_carried_forward_every_step_per_element(dev, route, dtype, H, B):
    """Chunks of 2 and 1 frames from a random fp32 state that no 16-bit type represents: step 0 is replayed from r(h_state), a slot
    with 0 frames gets its state back bit for bit, and the returned state is y / cells at each slot's last live frame."""
    full = R.make_case(H, B, sum(R.CARRY_CHUNKS), state=True)
    w_hh = full["w_hh"].to(dev)
    h, c = full["h0"].to(dev).clone(), full["c0"].to(dev).clone()
    t0, worst = 0, 0.0
    for T in R.CARRY_CHUNKS:
        L = R.carry_lengths(B, T)
        assert 0 in L and (T == 1 or T in L) and L[B - 1] < T and (B - 1) % 16 == 0
        chunk = dict(full, T=T, gx=full["gx"][:, t0:t0 + T].contiguous(), lengths=L)
        before = (h.clone(), c.clone())
        y, gates, cells = _forward(dev, chunk, dtype, CARRY_ENTRY[route], w_hh=w_hh, state=(h, c))
        worst = max(worst, R.check_forward(chunk, dtype, route, gates, cells, y, state=before,
                                           what=f"{route} carried {NAME[dtype]} H={H} B={B} frames {t0}..{t0 + T - 1}"))
        n = torch.tensor(L, device=dev)
        rows, last = torch.arange(B, device=dev), (n - 1).clamp(min=0)
        assert torch.equal(h, torch.where((n > 0)[:, None], y[rows, last], before[0]))
        assert torch.equal(c, torch.where((n > 0)[:, None], cells[rows, last], before[1]))
        t0 += T
    print(f"{route} carried {NAME[dtype]} H={H} B={B}: worst fraction of the bound {worst:.3f}")
