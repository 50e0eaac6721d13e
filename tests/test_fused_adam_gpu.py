"""conformer_amd.optim.FusedAdam on the device against torch.optim.Adam in float64 on the CPU, from the same fp32 values:
every parameter AND exp_avg, exp_avg_sq to rel-L2 < 2e-6, every parameter's state['step'] exactly.  The scenarios
(tests/fused_adam_cases.py; the same ones run against the restated entry on the host in tests/test_fused_adam_host_cpu.py)
are the ones where a step count per GROUP, which FusedAdam used to keep, departs from the stock optimizer's count per
PARAMETER -- a parameter that joins late, one that sits a step out, a loaded state with unequal counts -- and the layouts
the kernel meets in training: two groups, a changing lr, 120 parameters, gradients that are views of one flat bucket."""
import pytest
import torch

from tests import fused_adam_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.__name__)
def test_scenario(dev, case):
    from conformer_amd.optim import FusedAdam
    case(FusedAdam, dev)


def test_loaded_device_step_tensors_are_converted_once(dev):
    """A state whose `step` tensors live on the device (a capturable stock optimizer saves such) is read in load_state_dict;
    step() then reads nothing back: it runs under a stream capture guard that forbids synchronisation."""
    from conformer_amd.optim import FusedAdam
    tw = cases.Twin(FusedAdam, dev, cases.SHAPES, lr=1e-2)
    for k in range(2):
        tw.grads([i for i in range(len(cases.SHAPES)) if k or i != 1])
        tw.step()
    sd = tw.fused.state_dict()
    for st in sd["state"].values():
        st["step"] = st["step"].to(dev)
    tw.fused.load_state_dict(sd)
    assert all(st["step"].device.type == "cpu" for st in tw.fused.state.values())
    tw.grads()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        tw.fused.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    tw.ref.step()
    tw.check()
    assert [int(tw.fused.state[p]["step"]) for p in tw.ps] == [3, 2, 3, 3, 3]


def test_equal_counts_are_one_entry_call_per_group(dev):
    """The ordinary step stays one call of the entry per group (ceil(n / 48) launches inside it), as bench.py times it."""
    from conformer_amd.optim import FusedAdam
    from tests.util import Calls
    tw = cases.Twin(FusedAdam, dev, [(5,)] * 100 + [(3,)] * 7, [(list(range(100)), dict(lr=1e-2)), (list(range(100, 107)), dict(lr=1e-3))])
    from conformer_amd import _lib
    lib = _lib.load()
    real, calls = lib.cfm3_adam_step_f32, []

    def spy(*args):
        calls.append(args[1])
        return real(*args)
    lib.cfm3_adam_step_f32 = spy
    try:
        for k in range(3):
            tw.grads()
            del calls[:]
            tw.step()
            assert calls == [100, 7]
        with Calls("cfm_adam_step_f32") as seen:                 # (the float entry is no longer FusedAdam's)
            tw.grads()
            tw.step()
        assert not seen
    finally:
        lib.cfm3_adam_step_f32 = real
    tw.check()


@pytest.mark.parametrize("how", ["weight_decay", "amsgrad", "maximize", "non_contiguous", "fp16", "cpu"])
def test_a_refused_step_changes_nothing_in_any_group(dev, how):
    """The offender is in the SECOND group; the first must not have stepped (it used to)."""
    from conformer_amd import _lib
    from conformer_amd.optim import FusedAdam
    tw = cases.Twin(FusedAdam, dev, [(6, 4), (9,), (4, 6)], [([0, 1], dict(lr=1e-2)), ([2], dict(lr=1e-2))])
    tw.grads()
    tw.fused.step()
    tw.grads()
    bad = tw.ps[2]
    if how in ("weight_decay", "amsgrad", "maximize"):
        tw.fused.param_groups[1][how] = 0.1 if how == "weight_decay" else True
    else:
        bad.grad = None
        if how == "non_contiguous":
            bad.data = bad.data.t()
        elif how == "fp16":
            bad.data = bad.data.half()
        else:
            bad.data = bad.data.cpu()
        bad.grad = torch.ones_like(bad.data).contiguous()

    def snap():
        tensors = [t.detach().clone() for p in tw.ps for t in (p, tw.fused.state[p]["exp_avg"], tw.fused.state[p]["exp_avg_sq"])]
        return tensors, dict(tw.fused._counts)
    before = snap()
    with pytest.raises(_lib.ConformerHipError):
        tw.fused.step()
    after = snap()
    assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(before[0], after[0]))
    assert before[1] == after[1] and sorted(after[1].values()) == [1, 1, 1]
    tw.fused.state_dict()
    assert [int(tw.fused.state[p]["step"]) for p in tw.ps] == [1, 1, 1]
