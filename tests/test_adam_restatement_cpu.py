"""tests/adam_restatement.py on the CPU: the restatement is torch.optim.Adam, its bounds hold for a correct fp32 evaluation
of the designed inputs, and they do not hold for five wrong formulas -- so the device test (tests/test_adam_kernel_gpu.py)
measures the kernel and discriminates."""
import math

import numpy as np
import pytest
import torch

from oracle import conformer_oracle as O
from tests import adam_restatement as R


def test_restatement_is_torch_adam_with_per_parameter_counts():
    """Float64 scalars, five steps, the second parameter without a gradient on steps 1, 2 and 4: every parameter follows its
    OWN count, as in torch.optim.Adam (parameters and both moments compared)."""
    g = torch.Generator().manual_seed(0)
    shapes = [(7, 5), (13,), (1,)]
    init = [torch.randn(*s, generator=g, dtype=torch.float64) for s in shapes]
    ps = [torch.nn.Parameter(t.clone()) for t in init]
    hyper = dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6)
    opt = torch.optim.Adam(ps, **hyper)
    mine = [(t.numpy().copy(), np.zeros(t.shape), np.zeros(t.shape), 0) for t in init]
    for k in range(5):
        for i, p in enumerate(ps):
            p.grad = None if i == 1 and k in (0, 1, 3) else torch.randn(p.shape, generator=g, dtype=torch.float64)
        opt.step()
        for i, p in enumerate(ps):
            if p.grad is None:
                continue
            x, m, v, t = mine[i]
            x, m, v = R.adam_step_ref(x, p.grad.numpy(), m, v, hyper["lr"], *hyper["betas"], hyper["eps"], t + 1, scalars="exact")
            mine[i] = (x, m, v, t + 1)
    assert [t for *_, t in mine] == [5, 2, 5] == [int(opt.state[p]["step"]) for p in ps]
    for (x, m, v, _), p in zip(mine, ps):
        np.testing.assert_allclose(x, p.detach().numpy(), rtol=1e-13, atol=0)
        np.testing.assert_allclose(m, opt.state[p]["exp_avg"].numpy(), rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(v, opt.state[p]["exp_avg_sq"].numpy(), rtol=1e-13, atol=1e-300)


def test_restatement_with_float64_scalars_is_the_oracles_adam_reference():
    g = torch.Generator().manual_seed(1)
    shapes = [(9, 4), (17,), (1,)]
    params = [torch.randn(*s, generator=g) for s in shapes]
    grads = [[torch.randn(*s, generator=g) * (0.1 + k) for s in shapes] for k in range(4)]
    ref = O.adam_reference(params, grads, lr=1e-2)
    for i, p in enumerate(params):
        x, m, v = p.double().numpy(), np.zeros(p.shape), np.zeros(p.shape)
        for k in range(4):
            x, m, v = R.adam_step_ref(x, grads[k][i].numpy(), m, v, 1e-2, 0.9, 0.999, 1e-8, k + 1, scalars="exact")
        np.testing.assert_allclose(x, ref[i].numpy(), rtol=1e-13, atol=0)


def test_fp32_scalars_are_the_kernels():
    """With the default fp32 scalars the restatement differs from the float64 one by the scalars' rounding only: 1e-7
    relative, not 1e-16 -- and `1 - beta` is formed from the fp32 beta."""
    lr, b2, eps, omb1, omb2, c1, sc2 = R._scalars(1e-2, 0.9, 0.999, 1e-8, 3, "float")
    f = np.float32
    assert omb1 == float(f(1) - f(0.9)) != 1 - 0.9 and omb2 == float(f(1) - f(0.999))
    assert abs(omb2 / (1 - 0.999) - 1) > 1e-5                    # what the fp32 beta costs the second moment
    double = R._scalars(1e-2, 0.9, 0.999, 1e-8, 3, "double")
    assert double[3:5] == (float(f(1 - 0.9)), float(f(1 - 0.999))) and abs(double[4] / (1 - 0.999) - 1) < 2.0 ** -24
    assert double[:3] + double[5:] == (lr, b2, eps, c1, sc2)
    assert set(R.ENTRIES.values()) == {"float", "double"}
    assert (lr, b2, eps) == (float(f(1e-2)), float(f(0.999)), float(f(1e-8)))
    assert c1 == float(f(1 - 0.9 ** 3)) and sc2 == float(f(math.sqrt(1 - 0.999 ** 3)))
    assert R.kernel_scalars(1e-2, 0.9, 0.999, 1e-8, 3) == (1e-2, 0.9, 0.999, 1e-8, 1 - 0.9 ** 3, math.sqrt(1 - 0.999 ** 3))


@pytest.mark.parametrize("name", R.CASE_CLASSES)
@pytest.mark.parametrize("beta1", [b for b, _ in R.BETAS])
def test_designed_inputs_are_what_they_claim(name, beta1):
    p, g, m, v = R.case_inputs(name, beta1)
    f = np.float32
    assert all(a.dtype == f and a.shape == (R.CASE_N,) and np.isfinite(a).all() for a in (p, g, m, v))
    tiny = np.finfo(f).tiny
    for a in (p, g, m, v):
        assert ((a == 0) | (np.abs(a) >= tiny)).all()                          # no denormal input
    assert (((g == 0) | ((np.abs(g) >= f(1e-12)) & (np.abs(g) <= f(1e12))))).all()
    assert (((v == 0) | ((v >= f(1e-24)) & (v <= f(1e24))))).all()
    if name == "zero":
        assert not g.any() and not v.any() and (m == 0).any() and (m != 0).any()
    if name == "cancel":
        omb = float(f(1) - f(beta1))
        terms = np.abs(m.astype(np.float64)) + np.abs(g.astype(np.float64) - m) * omb
        m_new = R.adam_step_ref(p, g, m, v, 1e-2, beta1, 0.999, 1e-8, 2)[1]
        assert (np.sign(g) == -np.sign(m)).all() and (np.abs(m_new) < 2e-3 * terms).all()
    if name == "range":
        a = np.abs(g[g != 0])
        assert a.min() <= 2e-12 and a.max() >= 5e11 and (g == 0).any() and (v == 0).any()


def _sweep():
    for (b1, b2), rest in R.configs().items():
        for t, eps, lr in rest:
            yield lr, b1, b2, eps, t


@pytest.mark.parametrize("scalars", sorted(R.ENTRIES.values()))
def test_the_fp32_evaluation_stays_inside_the_bounds_and_in_range(scalars):
    """numpy float32, one rounding per operation, no fma: every element of every class at every point of the sweep lies
    inside the bounds (the inputs do not leave them through the reference alone), no result overflows or is denormal."""
    worst = np.zeros(3)
    tiny = np.finfo(np.float32).tiny
    for lr, b1, b2, eps, t in _sweep():
        for name in R.CASE_CLASSES:
            x = R.case_inputs(name, b1)
            with np.errstate(all="raise", under="ignore"):
                got = R.adam_step_f32(*x, lr, b1, b2, eps, t, scalars)
            for a in got:
                assert np.isfinite(a).all() and ((a == 0) | (np.abs(a) >= tiny)).all(), (name, lr, b1, b2, eps, t)
            ratios = R.check_step(got, *x, lr, b1, b2, eps, t, scalars)
            for k, r in enumerate(ratios):
                assert r.max() <= 1.0, (name, "p' m' v'".split()[k], float(r.max()), lr, b1, b2, eps, t)
                worst[k] = max(worst[k], r.max())
    print(f"fp32 numpy evaluation, largest error / bound: p' {worst[0]:.3f}, m' {worst[1]:.3f}, v' {worst[2]:.3f}")
    assert (worst > 0.05).all()                                   # ... and the bounds are not loose by orders of magnitude


def _mutant(kind, p, g, m, v, lr, beta1, beta2, eps, step):
    """A subtly wrong Adam step in float64 from the kernel's fp32 scalars: (p', m', v')."""
    p, g, m, v = R._f64(p, g, m, v)
    if kind == "step_minus_one":
        step -= 1
    lr, b2, eps, omb1, omb2, c1, sc2 = R._scalars(lr, beta1, beta2, eps, step, "float")
    m_new = m + (g - m) * (omb2 if kind == "beta2_for_first_moment" else omb1)
    v_new = b2 * v + omb2 * (np.abs(g) if kind == "g_for_g_squared" else g * g)
    if kind == "eps_inside_sqrt":
        den = np.sqrt(v_new / (sc2 * sc2) + eps)
    elif kind == "c2_not_applied":
        den = np.sqrt(v_new) + eps
    else:
        den = np.sqrt(v_new) / sc2 + eps
    return p - (lr / c1) * m_new / den, m_new, v_new


MUTANTS = ("eps_inside_sqrt", "c2_not_applied", "beta2_for_first_moment", "g_for_g_squared", "step_minus_one")
# where a mutant IS the correct formula, and so cannot be told apart (asserted below to be equal there, not assumed):
#   g = 0 and v = 0 give v' = 0 whatever is done to g, and a denominator of eps whatever sqrt(v') is divided by
SAME_MATHS = {("g_for_g_squared", "zero"), ("c2_not_applied", "zero")}


@pytest.mark.parametrize("name", R.CASE_CLASSES)
@pytest.mark.parametrize("kind", MUTANTS)
def test_bounds_discriminate(kind, name):
    """On the inputs the device test uses (step 2, the default betas, eps 1e-8, lr 1e-2), checked as the device is: each
    wrong formula leaves a bound by at least 10x on at least one element of every class."""
    lr, b1, b2, eps, t = 1e-2, 0.9, 0.999, 1e-8, 2
    x = R.case_inputs(name, b1)
    got = _mutant(kind, *x, lr, b1, b2, eps, t)
    if (kind, name) in SAME_MATHS:
        assert all(np.array_equal(a, b) for a, b in zip(got, R.adam_step_ref(*x, lr, b1, b2, eps, t)))
        return
    worst = max(float(r.max()) for r in R.check_step(got, *x, lr, b1, b2, eps, t))
    assert worst >= 10.0, (kind, name, worst)


@pytest.mark.parametrize("b1,b2", R.BETAS)
def test_bounds_discriminate_at_every_pair_of_betas(b1, b2):
    """... and over the four classes together at the other betas too (where the mutant differs from the formula at all)."""
    lr, eps, t = 1e-2, 1e-8, 2
    for kind in MUTANTS:
        worst = 0.0
        for name in R.CASE_CLASSES:
            x = R.case_inputs(name, b1)
            got = _mutant(kind, *x, lr, b1, b2, eps, t)
            worst = max(worst, max(float(r.max()) for r in R.check_step(got, *x, lr, b1, b2, eps, t)))
        assert worst >= 10.0, (kind, b1, b2, worst)
