"""The per-element bound of tests/lstm_step_restatement.py discriminates, and its replay is the LSTM: fed its own outputs the
float64 replay reproduces oracle.lstm_layer (forward, and dG through autograd, ragged lengths included); the fp32 emulation of
the kernels' arithmetic stays inside the bound at every case shape and dtype; every structural fault of FAULTS leaves it; and E,
the allowance for one step of fp32 arithmetic, is its measurement on the emulation.  No GPU."""
import pytest
import torch

from oracle import conformer_oracle as O
from tests import lstm_step_restatement as R

NAME = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}


@pytest.fixture(scope="module")
def runs():
    """direction -> [(label, case, dtype, replay kwargs, the emulation's outputs, the clean replay of them)] over every case
    shape and dtype: the emulation plays the device.  Computed once, never modified."""
    return R.emulated_runs()


@pytest.mark.parametrize("H,B,T,lengths", [(20, 5, 6, [6, 2, 5, 1, 3]), (16, 3, 4, None), (48, 17, 5, "table")])
def test_replay_fed_its_own_outputs_is_the_oracle_lstm(H, B, T, lengths):
    """Forward y and, through autograd of sum(y * dy), the gradient of the pre-activations: to float64 rounding."""
    case = R.make_case(H, B, T, lengths=R.lengths_for(B, T) if lengths == "table" else lengths)
    if lengths is None:
        case["lengths"] = None
    L = None if case["lengths"] is None else torch.tensor(case["lengths"])
    gx = case["gx"].double().requires_grad_(True)
    zero = torch.zeros(4 * H, dtype=torch.float64)
    ref = O.lstm_layer(gx, L, torch.eye(4 * H, dtype=torch.float64), case["w_hh"].double(), zero, zero)
    (ref * case["dy"].double()).sum().backward()
    gates, cells, y = R.replay_forward(case, torch.float32)
    assert (y - ref.detach()).abs().max() < 1e-14
    dG, dc = R.replay_backward(case, torch.float32, gates, cells)
    assert (dG - gx.grad).abs().max() < 1e-13
    live = R.live_mask(case["lengths"], B, T)
    assert (dG[~live] == 0).all() and (y[~live] == 0).all() and torch.isfinite(dc).all()


def test_measured_E_is_within_the_recorded_constants():
    e_fwd, e_bwd = R.measure_E()            # 4.182e-7 and 2.324e-7: elementwise IEEE operations only, the same on every machine
    print(f"E forward: measured {e_fwd:.3e}, recorded {R.E_FWD_MEASURED:.3e}; backward: measured {e_bwd:.3e}, recorded "
          f"{R.E_BWD_MEASURED:.3e}")
    assert R.E_MARGIN == 8 and R.E_FWD == 8 * R.E_FWD_MEASURED and R.E_BWD == 8 * R.E_BWD_MEASURED
    assert e_fwd <= R.E_FWD_MEASURED and e_bwd <= R.E_BWD_MEASURED          # no larger than the recorded constants
    assert R.E_FWD_MEASURED <= 2 * e_fwd and R.E_BWD_MEASURED <= 2 * e_bwd  # which are this measurement, not a looser number


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_clean_emulation_is_inside_the_bound_everywhere(runs, direction):
    worst = 0.0
    for label, case, dt, kw, emu, _ in runs[direction]:
        route, what = label.split()[0], f"{label} {NAME[dt]}"
        if direction == "fwd":
            worst = max(worst, R.check_forward(case, dt, route, *emu, state=kw.get("state"), what=what))
        else:
            worst = max(worst, R.check_backward(case, dt, route, kw["gates"], kw["cells"], *emu, what=what))
    print(f"{direction}: the emulation's worst fraction of the bound {worst:.3f}")
    assert worst <= 1.0 / R.E_MARGIN + 1e-9


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("fault", R.FAULTS)
@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_every_fault_leaves_the_bound_at_least_tenfold(runs, direction, fault, dtype):
    """At every case shape to which the fault applies, some element is at least 10x outside the bound.

    Measured, the weakest case shape of each fault, forward / backward: the unrounded exchange 14.4x / 18.9x under fp16 (H=16, the
    fewest elements) and 106x / 153x under bf16; every other fault 3.4e3x or more."""
    E = R.E_FWD if direction == "fwd" else R.E_BWD
    seen, weakest = 0, None
    for label, case, dt, kw, _, clean in runs[direction]:
        if dt != dtype or not R.fault_applies(fault, direction, dt, case["B"], case["lengths"], case["T"]):
            continue
        bad = R.faulty(direction, case, dt, fault, **kw)
        frac = max(R.worst_fraction(b.float(), c, E)[0] for b, c in zip(bad, clean))
        seen += 1
        if weakest is None or frac < weakest[0]:
            weakest = (frac, label)
    if not seen:
        assert not R.fault_applies(fault, direction, dtype, 33, R.lengths_for(33, 3), 3)
        return
    print(f"{direction} {fault} {NAME[dtype]}: weakest over {seen} cases {weakest[0]:.1f}x at {weakest[1]}")
    assert weakest[0] >= 10.0, weakest


def test_check_names_the_element_and_its_owner():
    case = R.make_case(48, 33, 3)
    eg, ec, ey = R.emulate_fp32("fwd", case, torch.bfloat16)
    assert R.check_forward(case, torch.bfloat16, "fwd_16", eg, ec, ey) <= 1.0 / R.E_MARGIN
    bad = eg.clone()
    bad[9, 1, 2 * 48 + 21] += 1e-4                         # utterance 9 is live at step 1
    assert case["lengths"][9] >= 2
    with pytest.raises(AssertionError, match=r"gates step 1 utterance 9 unit 21 gate g \(workgroup \(2, 0\) wave 1 of fwd_16\)"):
        R.check_forward(case, torch.bfloat16, "fwd_16", bad, ec, ey, what="case")
    dead = [b for b in range(33) if case["lengths"][b] < 3][0]
    bad = ec.clone()
    bad[dead, 2, 0] = torch.nextafter(bad[dead, 2, 0], torch.tensor(9.0))      # a frozen cell must be EQUAL, not merely close
    with pytest.raises(AssertionError, match=rf"cells step 2 utterance {dead} unit 0 "):
        R.check_forward(case, torch.bfloat16, "fwd_16", eg, bad, ey)
    assert R.owner("bwd_16", 21, 37) == ((2, 1), 1) and R.owner("fwd_row", 16, 323) == ((80, 1), 0)
