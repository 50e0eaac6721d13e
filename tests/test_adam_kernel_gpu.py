"""The fused Adam kernel (csrc/train_aux.hip::adam_kernel) through its two entries, called directly with a ctypes table as
optim.py does: cfm_adam_step_f32 (float scalars) and cfm3_adam_step_f32 (double scalars, what FusedAdam calls).  Every output
element is held against the float64 restatement of ONE step (tests/adam_restatement.py) within the forward-error bounds of a
correct fp32 evaluation -- m' and v' from the inputs, p' from the device's own m' and v' --, on designed inputs (g = 0 with
v = 0, near-cancelling m', |g| over 24 decades in one tensor), over the step counts, betas, eps and lr of the sweep; at every
chunk and tail size next to sentinels; at every split of the table into launches, where a tensor's result must not depend on
its place in the table; and on the scalar path of pointers that are not 16-byte aligned.  The refusals need no GPU:
tests/test_abi.py::test_adam_step_refusals_without_gpu.  tests/test_adam_restatement_cpu.py shows that the bounds hold for
a correct fp32 evaluation of these inputs and are left tenfold by five wrong formulas.

Largest observed error / bound on the MI355X over the whole sweep of (a) (a ratio above 1 would be a kernel or restatement
bug, not a bound to widen; test_one_step_per_element_over_the_sweep prints the figures per class under `pytest -s`):
    cfm3_adam_step_f32   p' 0.496   m' 0.310   v' 0.273
    cfm_adam_step_f32    p' 0.497   m' 0.310   v' 0.292
(numpy's fp32 evaluation of the same expressions, one rounding per operation: p' 0.497, m' 0.324, v' 0.292.)  On the
g = 0, v = 0 class v' is exactly 0 and, where m = 0 as well, p does not move."""
import ctypes

import numpy as np
import pytest
import torch

from tests import adam_restatement as R

pytestmark = pytest.mark.gpu

GUARD = 64                             # elements before and after every guarded slice (256 bytes: the slice keeps its offset mod 16 bytes)
SENTINEL = 0x7FC0DEAD                  # a NaN with a payload: any arithmetic on it, or any store over it, shows
ENTRIES = sorted(R.ENTRIES)
DEFAULT = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, step=3)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def adam_call(entry, rows, lr, beta1, beta2, eps, step):
    """One call of `entry` over rows = [(p, g, m, v) device tensors]; the scalars as optim.py forms them."""
    from conformer_amd import _lib, ops
    from conformer_amd.optim import _AdamTensor
    arr = (_AdamTensor * len(rows))()
    for i, (p, g, m, v) in enumerate(rows):
        assert all(t.is_contiguous() and t.dtype == torch.float32 and t.numel() == p.numel() for t in (p, g, m, v))
        arr[i] = _AdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel())
    _lib.call(entry, ctypes.addressof(arr), len(rows), *R.kernel_scalars(lr, beta1, beta2, eps, step), ops._stream())


def guarded(values, offset, dev):
    """(buffer, slice): `values` at element `offset` behind GUARD sentinels of a sentinel-filled allocation, GUARD more behind"""
    n = len(values)
    buf = torch.full((GUARD + offset + n + GUARD,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    sl = buf[GUARD + offset:GUARD + offset + n]
    sl.copy_(torch.from_numpy(np.ascontiguousarray(values)))
    assert sl.data_ptr() % 16 == 4 * (offset % 4)
    return buf, sl


def guards_intact(buf, offset, n):
    bits = buf.view(torch.int32)
    return bool((bits[:GUARD + offset] == SENTINEL).all()) and bool((bits[GUARD + offset + n:] == SENTINEL).all())


def worst_ratios(got, x, hyper, scalars):
    """(p', m', v') largest error / bound of device outputs `got` (tensors) for inputs x (numpy)"""
    out = [t.detach().cpu().numpy() for t in got]
    return [float(r.max()) for r in R.check_step(out, *x, hyper["lr"], hyper["beta1"], hyper["beta2"], hyper["eps"], hyper["step"],
                                                  scalars)]


def assert_within(ratios, what):
    for name, r in zip(("p'", "m'", "v'"), ratios):
        assert r <= 1.0, f"{what}: {name} leaves its bound, error / bound = {r:.3g}"


# ---- a. one step, per element, op by op ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("b1,b2", R.BETAS)
def test_one_step_per_element_over_the_sweep(dev, entry, b1, b2):
    scalars = R.ENTRIES[entry]
    inputs = {name: R.case_inputs(name, b1) for name in R.CASE_CLASSES}
    pristine = {name: [torch.from_numpy(a).to(dev) for a in x] for name, x in inputs.items()}
    worst = {name: [0.0, 0.0, 0.0] for name in R.CASE_CLASSES}
    for t, eps, lr in R.configs()[(b1, b2)]:
        hyper = dict(lr=lr, beta1=b1, beta2=b2, eps=eps, step=t)
        rows = {name: [a.clone() for a in x] for name, x in pristine.items()}
        adam_call(entry, [tuple(rows[name]) for name in R.CASE_CLASSES], **hyper)     # the four classes in one table
        for name in R.CASE_CLASSES:
            p, g, m, v = rows[name]
            assert torch.equal(g, pristine[name][1])
            ratios = worst_ratios((p, m, v), inputs[name], hyper, scalars)
            worst[name] = [max(a, b) for a, b in zip(worst[name], ratios)]
            assert_within(ratios, f"{entry} {name} t={t} betas=({b1}, {b2}) eps={eps} lr={lr}")
            if name == "zero":                                   # m = 0, g = 0, v = 0: 0 / eps, the parameter does not move
                still = inputs[name][2] == 0
                assert np.array_equal(p.cpu().numpy()[still], inputs[name][0][still])
    for name, (rp, rm, rv) in worst.items():
        print(f"adam ratios {entry} betas=({b1}, {b2}) {name}: p' {rp:.3f} m' {rm:.3f} v' {rv:.3f}")


# ---- b. chunk and tail ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1023, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 12289])
def test_chunk_and_tail_next_to_sentinels(dev, entry, n):
    x = R.case_inputs("generic", DEFAULT["beta1"], n=n, seed=n)
    (bp, p), (bg, g), (bm, m), (bv, v) = (guarded(a, 0, dev) for a in x)
    g_before = bg.clone()
    adam_call(entry, [(p, g, m, v)], **DEFAULT)
    assert_within(worst_ratios((p, m, v), x, DEFAULT, R.ENTRIES[entry]), f"{entry} n={n}")
    for name, buf in (("param", bp), ("exp_avg", bm), ("exp_avg_sq", bv)):
        assert guards_intact(buf, 0, n), f"{entry} n={n}: a write outside {name}"
    assert torch.equal(bg.view(torch.int32), g_before.view(torch.int32)), f"{entry} n={n}: grad was written"


# ---- c. launch split ------------------------------------------------------------------------------------------------------------
SPLIT_SIZES = (1, 5, 4096, 4097, 17)


@pytest.fixture(scope="module")
def split_inputs(dev):
    """145 tensors of distinct values, sizes cycling through SPLIT_SIZES (runs of one-block tensors next to two-block ones in
    the first-block prefix), uploaded once: (numpy inputs, device tensors)."""
    xs = [R.case_inputs("generic", DEFAULT["beta1"], n=SPLIT_SIZES[i % len(SPLIT_SIZES)], seed=1000 + i) for i in range(145)]
    return xs, [[torch.from_numpy(a).to(dev) for a in x] for x in xs]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n_tensors", [1, 47, 48, 49, 96, 97, 145])
def test_launch_split_and_place_in_the_table(dev, split_inputs, entry, n_tensors):
    xs, pristine = split_inputs
    rows = [[a.clone() for a in x] for x in pristine[:n_tensors]]
    adam_call(entry, [tuple(r) for r in rows], **DEFAULT)
    same = []
    for i, (x, row) in enumerate(zip(xs, rows)):
        p, g, m, v = row
        assert_within(worst_ratios((p, m, v), x, DEFAULT, R.ENTRIES[entry]), f"{entry} tensor {i} of {n_tensors} (n={p.numel()})")
        alone = [a.clone() for a in pristine[i]]
        assert all(a.data_ptr() % 16 == b.data_ptr() % 16 for a, b in zip(alone, row))
        adam_call(entry, [tuple(alone)], **DEFAULT)
        same.append(all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                        for a, b in zip((alone[0], alone[2], alone[3]), (p, m, v))))
        assert torch.equal(g, pristine[i][1])
    differ = [i for i, ok in enumerate(same) if not ok]
    assert not differ, f"{entry}: tensors {differ} of {n_tensors} differ from the same tensor stepped alone"


# ---- d. alignment: the scalar path ---------------------------------------------------------------------------------------------
OFFSETS = ([tuple(o if k == which else 0 for k in range(4)) for which in range(4) for o in (1, 2, 3)]
           + [(1, 1, 1, 1), (0, 1, 2, 3)])                      # element offsets of (param, grad, exp_avg, exp_avg_sq)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n", [5, 4099])
def test_unaligned_pointers_take_the_scalar_path(dev, entry, n):
    x = R.case_inputs("generic", DEFAULT["beta1"], n=n, seed=7 + n)
    aligned = [torch.from_numpy(a).to(dev) for a in x]
    adam_call(entry, [tuple(aligned)], **DEFAULT)
    for offsets in OFFSETS:
        bufs, rows = zip(*(guarded(a, o, dev) for a, o in zip(x, offsets)))
        g_before = bufs[1].clone()
        adam_call(entry, [tuple(rows)], **DEFAULT)
        p, g, m, v = rows
        equal = all(torch.equal(a, b) for a, b in zip((p, m, v), (aligned[0], aligned[2], aligned[3])))
        what = f"{entry} n={n} offsets={offsets} (bit-equal to the aligned run: {equal})"
        assert_within(worst_ratios((p, m, v), x, DEFAULT, R.ENTRIES[entry]), what)
        for name, k in (("param", 0), ("exp_avg", 2), ("exp_avg_sq", 3)):
            assert guards_intact(bufs[k], offsets[k], n), f"{what}: a write outside {name}"
        assert torch.equal(bufs[1].view(torch.int32), g_before.view(torch.int32)), f"{what}: grad was written"


def test_the_two_entries_differ_by_one_minus_beta_only(dev):
    """cfm3_adam_step_f32 is the same kernel fed 1 - beta from the double: at betas whose fp32 complement is exact either way
    (0.5, 0.75) the two entries agree bit for bit; at beta2 = 0.999 the float entry's exp_avg_sq is the one 1.3e-5 away from
    the float64 optimizer's."""
    x = R.case_inputs("generic", 0.5, n=1025, seed=3)
    out = {}
    for b2 in (0.75, 0.999):
        for entry in ENTRIES:
            row = [torch.from_numpy(a).to(dev) for a in x]
            row[3].zero_()                                       # v = 0: v' = (1 - beta2) g^2
            adam_call(entry, [tuple(row)], lr=1e-2, beta1=0.5, beta2=b2, eps=1e-8, step=1)
            out[b2, entry] = row
    assert all(torch.equal(a, b) for a, b in zip(out[0.75, ENTRIES[0]], out[0.75, ENTRIES[1]]))
    exact = (1 - 0.999) * x[1].astype(np.float64) ** 2
    off = {e: float(np.abs(out[0.999, e][3].cpu().numpy() / exact - 1).max()) for e in ENTRIES}
    assert off["cfm3_adam_step_f32"] < 4 * R.U * R.MARGIN and 1.2e-5 < off["cfm_adam_step_f32"] < 1.4e-5, off
