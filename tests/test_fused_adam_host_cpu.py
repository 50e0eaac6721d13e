"""The host half of conformer_amd.optim.FusedAdam without a GPU: the scenarios of tests/fused_adam_cases.py with the entry
cfm_adam_step_f32 replaced by the fp32 restatement (tests/adam_restatement.py::adam_step_f32) working on host memory.  What
this holds is everything step() decides on the host: the per-parameter counts and bias corrections, which parameters go out
in which call, the descriptor tables and their cache, state_dict / load_state_dict, the refusals.  The kernel itself is held
on the device by tests/test_adam_kernel_gpu.py, and the same scenarios run there in tests/test_fused_adam_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import fused_adam_cases as cases
from tests.adam_restatement import adam_step_f32


@pytest.fixture
def entry(monkeypatch):
    """FusedAdam on CPU tensors: the entry swapped on the library object (which is what _lib.call runs), every call recorded
    as (n_tensors, numels, bias_c1, sqrt_bias_c2)."""
    from conformer_amd import _lib, ops, optim
    lib = _lib.load()
    log = []

    def view(ptr, n):
        return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_float)), shape=(n,))

    def fake(tensors, n_tensors, lr, b1, b2, eps, c1, sc2, stream):
        arr = ctypes.cast(tensors, ctypes.POINTER(optim._AdamTensor))
        f = np.float32
        for i in range(n_tensors):
            t = arr[i]
            assert t.param and t.grad and t.exp_avg and t.exp_avg_sq and t.numel > 0
            p, g, m, v = (view(a, t.numel) for a in (t.param, t.grad, t.exp_avg, t.exp_avg_sq))
            m_new = m + (g - m) * f(1.0 - b1)
            v_new = f(b2) * v + f(1.0 - b2) * g * g
            p[:] = p - (f(lr) / f(c1)) * m_new / (np.sqrt(v_new) / f(sc2) + f(eps))
            m[:], v[:] = m_new, v_new
        log.append((n_tensors, [arr[i].numel for i in range(n_tensors)], c1, sc2))
        return 0

    monkeypatch.setattr(lib, "cfm3_adam_step_f32", fake, raising=True)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(optim, "_fits", lambda t: t.dtype == torch.float32 and t.is_contiguous())
    return log


def test_the_fake_entry_is_the_restated_step(entry):
    from conformer_amd import _lib, optim
    rng = np.random.default_rng(0)
    p, g, m = (rng.standard_normal(37).astype(np.float32) for _ in range(3))
    v = rng.random(37).astype(np.float32)
    want = adam_step_f32(p, g, m, v, 1e-2, 0.9, 0.999, 1e-8, 3, scalars="double")
    arr = (optim._AdamTensor * 1)(optim._AdamTensor(p.ctypes.data, g.ctypes.data, m.ctypes.data, v.ctypes.data, 37))
    _lib.call("cfm3_adam_step_f32", ctypes.addressof(arr), 1, 1e-2, 0.9, 0.999, 1e-8, 1 - 0.9 ** 3, (1 - 0.999 ** 3) ** 0.5, None)
    assert all(np.array_equal(a, b) for a, b in zip((p, m, v), want))


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.__name__)
def test_scenario_on_the_host(entry, case):
    from conformer_amd.optim import FusedAdam
    case(FusedAdam, torch.device("cpu"))


def test_equal_counts_are_one_call_per_group(entry):
    """The ordinary step (every parameter of a group at the same count) is exactly one call of the entry per group, whatever
    the number of parameters; unequal counts are one call per distinct count, and the calls merge again when the counts do."""
    from conformer_amd.optim import FusedAdam
    tw = cases.Twin(FusedAdam, torch.device("cpu"), [(3,)] * 100 + [(5,)] * 30, [(list(range(100)), dict(lr=1e-2)),
                                                                                 (list(range(100, 130)), dict(lr=1e-3))])
    for k in range(3):
        tw.grads()
        del entry[:]
        tw.step()
        assert [n for n, *_ in entry] == [100, 30]
    tw.grads([i for i in range(130) if i not in (7, 8, 110)])     # three parameters sit a step out
    del entry[:]
    tw.step()
    assert [n for n, *_ in entry] == [98, 29]
    tw.grads()
    del entry[:]
    tw.step()
    assert sorted(n for n, *_ in entry) == [1, 2, 29, 98]         # (counts 5 and 4 in both groups)
    c1 = {n: c for n, _, c, _ in entry}
    assert c1[98] == 1 - 0.9 ** 5 and c1[2] == 1 - 0.9 ** 4
    tw.check()


def test_table_cache_follows_the_membership_of_a_call(entry):
    """The same call slot of a group holds other parameters from one step to the next: the cached table is rebuilt, and every
    parameter is stepped with its own moments (a stale table would step a parameter against another one's state)."""
    from conformer_amd.optim import FusedAdam
    tw = cases.Twin(FusedAdam, torch.device("cpu"), [(4,), (4,), (4,), (4,)], lr=1e-2)
    for live in ([0, 1], [2, 3], [0, 1, 2, 3], [1, 2], [0, 3], [0, 1, 2, 3], [3, 2, 1, 0]):
        tw.grads(live)
        tw.step()
        tw.check(f"after {live}:")


def test_step_reads_nothing_back_and_load_converts_once(entry):
    """The counts live on the host: step() never touches state[p]['step'], and load_state_dict leaves host tensors there."""
    from conformer_amd.optim import FusedAdam
    tw = cases.Twin(FusedAdam, torch.device("cpu"), cases.SHAPES, lr=1e-2)
    tw.grads()
    tw.step()

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"step() read state['step'].{name}")
    for p in tw.ps:
        tw.fused.state[p]["step"] = Untouchable()
    tw.grads()
    tw.step()
    for p in tw.ps:
        tw.fused.state[p]["step"] = torch.tensor(0.0)            # (what state_dict() overwrites with the host count)
    sd = tw.fused.state_dict()
    assert [float(s["step"]) for s in sd["state"].values()] == [2.0] * len(tw.ps)
    again = FusedAdam([torch.nn.Parameter(p.detach().clone()) for p in tw.ps], lr=1e-2)
    again.load_state_dict(sd)
    assert all(st["step"].device.type == "cpu" for st in again.state.values())
    assert sorted(again._counts.values()) == [2] * len(tw.ps)


@pytest.mark.parametrize("how", ["weight_decay", "amsgrad", "maximize", "non_contiguous", "non_contiguous_grad", "fp16"])
def test_a_refused_step_changes_nothing_in_any_group(entry, how):
    """The refusal is in the SECOND group: the first must not have stepped."""
    from conformer_amd import _lib
    from conformer_amd.optim import FusedAdam
    opts = {how: 0.1 if how == "weight_decay" else True} if how in ("weight_decay", "amsgrad", "maximize") else {}
    tw = cases.Twin(FusedAdam, torch.device("cpu"), [(6, 4), (9,), (4, 6)], [([0, 1], dict(lr=1e-2)), ([2], dict(lr=1e-2))])
    tw.grads()
    tw.fused.step()
    tw.grads()
    bad = tw.ps[2]
    if opts:
        tw.fused.param_groups[1].update(opts)
    elif how == "non_contiguous":
        bad.grad = None
        bad.data = bad.data.t()
        bad.grad = torch.ones(6, 4)
    elif how == "non_contiguous_grad":
        bad.grad = torch.ones(6, 4).t()
    else:
        bad.grad = None
        bad.data = bad.data.half()
        bad.grad = torch.ones(4, 6, dtype=torch.float16)
    snap = lambda: ([p.detach().clone() for p in tw.ps],
                    [t.clone() for p in tw.ps for t in (tw.fused.state[p]["exp_avg"], tw.fused.state[p]["exp_avg_sq"])],
                    dict(tw.fused._counts))
    before = snap()
    del entry[:]
    with pytest.raises(_lib.ConformerHipError):
        tw.fused.step()
    after = snap()
    assert not entry
    assert all(torch.equal(a, b) for a, b in zip(before[0], after[0]))
    assert all(torch.equal(a, b) for a, b in zip(before[1], after[1]))
    assert before[2] == after[2] == {p: 1 for p in tw.ps}
