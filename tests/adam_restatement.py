"""Float64 restatement of ONE step of the fused Adam kernel (csrc/train_aux.hip::adam_kernel), element by element, with the
forward-error bounds of its fp32 evaluation, and the designed inputs the CPU and GPU tests share.

The kernel computes, per element, in fp32:

    m' = m + (g - m) * (1 - beta1)                                   (the lerp form of torch's foreach / fused Adam)
    v' = beta2 * v + (1 - beta2) * g * g                             (evaluated ((1 - beta2) * g) * g)
    p' = p - (lr / c1) * m' / (sqrt(v') / sqrt_c2 + eps)             (evaluated ((lr / c1) * m') / (...))

from the six scalars lr, beta1, beta2, eps, c1 = 1 - beta1^t and sqrt_c2 = sqrt(1 - beta2^t), which the host forms in
double.  `adam_step_ref` evaluates the same expressions in float64 FROM THE SCALARS AS THE KERNEL RECEIVES THEM, so a
comparison with the device measures the roundings of the kernel's own arithmetic and nothing else:
  scalars="float"   the entry cfm_adam_step_f32: the C ABI rounds the six to fp32 and 1 - beta is the fp32 difference from the
                    fp32 beta (exact for that beta -- and 1.3e-5 off 1 - 0.999, which is why FusedAdam calls the next one);
  scalars="double"  the entry cfm3_adam_step_f32: the six cross as doubles, 1 - beta is formed in double, all are rounded once;
  scalars="exact"   nothing is rounded: that is torch.optim.Adam in float64.

All arrays are numpy float64 (float32 inputs are widened exactly)."""
import math

import numpy as np

U = 2.0 ** -24            # unit roundoff of fp32: one correctly rounded operation is off by at most U relative
MARGIN = 2.0              # the one margin of every bound: covers an fma contracted or not and a division or square root one ulp off


def kernel_scalars(lr, beta1, beta2, eps, step):
    """(lr, beta1, beta2, eps, bias_c1, sqrt_bias_c2) as optim.py hands them to cfm_adam_step_f32: Python doubles."""
    return (float(lr), float(beta1), float(beta2), float(eps), 1.0 - beta1 ** step, math.sqrt(1.0 - beta2 ** step))


ENTRIES = {"cfm_adam_step_f32": "float", "cfm3_adam_step_f32": "double"}      # entry -> how its scalars cross the C boundary


def _scalars(lr, beta1, beta2, eps, step, scalars):
    """(lr, beta2, eps, 1 - beta1, 1 - beta2, c1, sqrt_c2) as float64 values of what the kernel computes with.  scalars:
      "float"   cfm_adam_step_f32: six floats; `1.0f - beta` is an fp32 subtraction from the fp32 beta
      "double"  cfm3_adam_step_f32: six doubles; 1 - beta is formed in double and rounded to fp32 like the others
      "exact"   nothing is rounded: torch.optim.Adam in float64"""
    lr, b1, b2, eps, c1, sc2 = kernel_scalars(lr, beta1, beta2, eps, step)
    if scalars == "exact":
        return lr, b2, eps, 1.0 - b1, 1.0 - b2, c1, sc2
    f = np.float32
    omb1, omb2 = (f(1.0) - f(b1), f(1.0) - f(b2)) if scalars == "float" else (f(1.0 - b1), f(1.0 - b2))
    assert scalars in ("float", "double")
    return tuple(float(x) for x in (f(lr), f(b2), f(eps), omb1, omb2, f(c1), f(sc2)))


def _f64(*arrays):
    return tuple(np.asarray(a, dtype=np.float64) for a in arrays)


def adam_step_ref(p, g, m, v, lr, beta1, beta2, eps, step, moments=None, scalars="float"):
    """One Adam step in float64: (p', m', v').  `moments=(m', v')`: p' is formed from THESE moments (the device's own, in the
    GPU test, so that the error of m' and v' does not compound into the check of p'); the returned m', v' are still the
    restated ones."""
    p, g, m, v = _f64(p, g, m, v)
    lr, b2, eps, omb1, omb2, c1, sc2 = _scalars(lr, beta1, beta2, eps, step, scalars)
    m_new = m + (g - m) * omb1
    v_new = b2 * v + omb2 * g * g
    mm, vv = (m_new, v_new) if moments is None else _f64(*moments)
    p_new = p - (lr / c1) * mm / (np.sqrt(vv) / sc2 + eps)
    return p_new, m_new, v_new


def adam_bounds(p, g, m, v, lr, beta1, beta2, eps, step, moments=None, scalars="float"):
    """Per-element bounds (bp, bm, bv) on |device - adam_step_ref| for a correct fp32 evaluation.  Each bound is
    MARGIN * (number of fp32 roundings) * U times the magnitude of the TERMS the roundings act on (not of the result, which
    cancellation can make arbitrarily smaller).  `moments`: as adam_step_ref, the (m', v') that p' is formed from."""
    p, g, m, v = _f64(p, g, m, v)
    omb1 = _scalars(lr, beta1, beta2, eps, step, scalars)[3]
    p_new, m_new, v_new = adam_step_ref(p, g, m, v, lr, beta1, beta2, eps, step, moments, scalars)
    # m' = m + (g - m) * (1 - beta1): 3 roundings (the subtraction, the product, the sum), each relative to a quantity of
    # magnitude at most |m| + |g - m| (1 - beta1)
    bm = MARGIN * 3 * U * (np.abs(m) + np.abs(g - m) * omb1)
    # v' = beta2 * v + ((1 - beta2) * g) * g: 4 roundings (three products, the sum); every term is non-negative, so each is
    # relative to at most v' itself
    bv = MARGIN * 4 * U * v_new
    # delta = ((lr / c1) * m') / (sqrt(v') / sqrt_c2 + eps): 6 roundings relative to |delta| (lr / c1, its product with m',
    # the square root, its quotient by sqrt_c2, the sum with eps -- both terms non-negative --, the division);
    # p' = p - delta: 1 rounding relative to |p'|
    delta = p - p_new
    bp = MARGIN * (6 * U * np.abs(delta) + 1 * U * np.abs(p_new))
    return bp, bm, bv


def adam_step_f32(p, g, m, v, lr, beta1, beta2, eps, step, scalars="float"):
    """The kernel's expressions in numpy float32 arithmetic, one rounding per operation (no fma): (p', m', v') float32."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    lr, b2, eps, omb1, omb2, c1, sc2 = (f(x) for x in _scalars(lr, beta1, beta2, eps, step, scalars))
    m_new = m + (g - m) * omb1
    v_new = b2 * v + omb2 * g * g
    p_new = p - (lr / c1) * m_new / (np.sqrt(v_new) / sc2 + eps)
    assert m_new.dtype == f and v_new.dtype == f and p_new.dtype == f
    return p_new, m_new, v_new


def check_step(got, p, g, m, v, lr, beta1, beta2, eps, step, scalars="float"):
    """The comparison both the CPU and the GPU test make: got = (p', m', v') of some evaluation.  m' and v' against the
    restatement from the inputs, p' against the restatement formed from got's OWN m', v'.  Returns the per-element
    error / bound ratios (rp, rm, rv); a correct fp32 evaluation keeps every ratio <= 1.  (A zero bound -- v' = 0, or
    m = g = 0 -- demands equality: ratio 0 when equal, inf when not.)"""
    gp, gm, gv = _f64(*got)
    rp_, rm_, rv_ = adam_step_ref(p, g, m, v, lr, beta1, beta2, eps, step, (gm, gv), scalars)
    bp, bm, bv = adam_bounds(p, g, m, v, lr, beta1, beta2, eps, step, (gm, gv), scalars)

    def ratio(x, r, b):
        e = np.abs(x - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(e == 0, 0.0, np.where(b > 0, e / b, np.inf))
    return ratio(gp, rp_, bp), ratio(gm, rm_, bm), ratio(gv, rv_, bv)


# ---- the sweeps of tests/test_adam_kernel_gpu.py (and of the discrimination tests on the CPU) --------------------------------
STEPS = (1, 2, 10, 1000, 100000)
BETAS = ((0.9, 0.999), (0.5, 0.9), (0.0, 0.999))
EPSS = (1e-8, 1e-3)
LRS = (1e-2, 2e-5)
CASE_CLASSES = ("generic", "zero", "cancel", "range")
CASE_N = 601              # not a multiple of 4: every class ends in the kernel's scalar tail


def _log_uniform(rng, n, lo, hi):
    return np.exp(rng.uniform(math.log(lo), math.log(hi), n))


def _signs(rng, n):
    return np.where(rng.random(n) < 0.5, -1.0, 1.0)


def case_inputs(name, beta1, n=CASE_N, seed=0):
    """fp32 (p, g, m, v) of one designed class.  No fp32 overflow and no denormals in inputs or results: |g| is 0 or in
    [1e-12, 1e12], v is 0 or in [1e-24, 1e24].
      generic  log-uniform magnitudes, random signs
      zero     g = 0 with v = 0 (the 0 / eps denominator); m is 0 on a third of the elements (p must not move at all)
      cancel   m and g of opposite sign with m + (g - m)(1 - beta1) cancelling to 1e-6 .. 1e-3 of its terms
      range    |g| log-spaced over the whole of [1e-12, 1e12] inside the one tensor, v over [1e-24, 1e24], a few of each 0"""
    rng = np.random.default_rng([seed, CASE_CLASSES.index(name)])
    p = _signs(rng, n) * _log_uniform(rng, n, 1e-8, 10.0)
    if name == "generic":
        g = _signs(rng, n) * _log_uniform(rng, n, 1e-6, 1e2)
        m = _signs(rng, n) * _log_uniform(rng, n, 1e-6, 1e2)
        v = _log_uniform(rng, n, 1e-12, 1e4)
    elif name == "zero":
        g, v = np.zeros(n), np.zeros(n)
        m = _signs(rng, n) * _log_uniform(rng, n, 1e-6, 1.0)
        m[::3] = 0.0
    elif name == "cancel":
        m = _signs(rng, n) * _log_uniform(rng, n, 1e-8, 1e2)
        rel = _signs(rng, n) * _log_uniform(rng, n, 1e-6, 1e-3)
        if beta1 == 0.0:
            rel = -np.abs(rel)                                   # (m' = g here: the cancellation is m + (g - m), g tiny and opposite)
        g = m * (rel - beta1 / (1.0 - beta1))                    # m' = m * rel * (1 - beta1)
        v = _log_uniform(rng, n, 1e-24, 1e-2)
    elif name == "range":
        g = _signs(rng, n) * np.exp(np.linspace(math.log(1e-12), math.log(1e12), n))
        rng.shuffle(g)
        m = _signs(rng, n) * _log_uniform(rng, n, 1e-12, 1e12)
        v = np.exp(np.linspace(math.log(1e-24), math.log(1e24), n))
        rng.shuffle(v)
        g[5::97] = 0.0
        v[11::89] = 0.0
    else:
        raise KeyError(name)
    f = np.float32
    p, g, m, v = (a.astype(f) for a in (p, g, m, v))
    g = np.where((g != 0) & (np.abs(g) < f(1e-12)), f(1e-12) * np.sign(g), g).astype(f)      # the fp32 rounding of an end point
    g = np.clip(g, -f(1e12), f(1e12))
    v = np.where((v != 0) & (v < f(1e-24)), f(1e-24), np.minimum(v, f(1e24))).astype(f)
    return p, g, m, v


def configs():
    """Every (beta1, beta2, step, eps, lr) of the sweep, grouped by the pair of betas (the cancel class depends on beta1)."""
    return {(b1, b2): [(t, eps, lr) for t in STEPS for eps in EPSS for lr in LRS] for b1, b2 in BETAS}
