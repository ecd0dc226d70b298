"""Adam references for the per-element tests of k_adam (csrc/elem.hip); a helper, not a test.

`adam_fp64` is torch.optim.Adam with its defaults (betas 0.9 / 0.999, eps 1e-8, no weight decay, no amsgrad; stage1_neural_atlas.py:132-134) in numpy
fp64; `adam_torch32` is the reference project's own optimizer, one `.step()` of torch.optim.Adam on the CPU in fp32, from a given state; `adam_bounds`
is the round-off an fp32 evaluation of that update may show against the fp64 one, per element, COUNTED from the roundings of the formulation — not
measured on anything (tests/test_adam_ref_host.py holds torch's fp32 step inside it without a GPU).

The roundings counted (u = 2^-24, one fp32 rounding):
  m' = m + (g - m) c1 (torch's lerp, k_adam's form) or 0.9 m + 0.1 g: the constant, two products / one difference, one sum   -> bm = 3u (|m| + |g|)
  v' = 0.999 v + (0.001 g) g: two constants, three products, one sum                                                         -> bv = 4u (v + g^2)
  den = sqrt(v') / sqrt(1 - 0.999^t) + eps: the propagated bv through the square root, then a 1-ulp square root, the divide, the add and the two
        fp32 constants (bias correction, eps)                                                                                -> 6u den
  q = m' / den: the propagated bm and dden, the divide and one spare                                                         -> 2u q
  p' = p - step_size q: the fp32 step size and the product (2u q), the final subtraction (u |p'|: half an ulp of the result, 2^-24 relative).
The absolute floors 2^-126 (bm) and 1e-37 (bv) are there because the device may flush subnormal moments to zero."""
import numpy as np

B1, B2, EPS = 0.9, 0.999, 1e-8
U = 2.0 ** -24


def _f64(*a):
    return [np.asarray(x, dtype=np.float64) for x in a]


def adam_fp64(p, m, v, g, step_after, lr=1e-4):
    """(p', m', v') after the step that makes the optimizer's counter `step_after`, everything in fp64."""
    p, m, v, g = _f64(p, m, v, g)
    t = float(step_after)
    m1 = B1 * m + (1.0 - B1) * g
    v1 = B2 * v + (1.0 - B2) * g * g
    bc1, bc2 = 1.0 - B1 ** t, 1.0 - B2 ** t
    p1 = p - lr / bc1 * m1 / (np.sqrt(v1) / np.sqrt(bc2) + EPS)
    return p1, m1, v1


def adam_torch32(p, m, v, g, step_after, lr=1e-4):
    """The same step by torch.optim.Adam(lr) on the CPU in fp32: state (step_after - 1, exp_avg = m, exp_avg_sq = v), .grad = g, one .step().
    Returns float32 arrays (p', m', v')."""
    return _adam_torch(p, m, v, g, step_after, lr, np.float32)


def adam_torch64(p, m, v, g, step_after, lr=1e-4):
    """torch.optim.Adam run in fp64 (what adam_fp64 restates)."""
    return _adam_torch(p, m, v, g, step_after, lr, np.float64)


def _adam_torch(p, m, v, g, step_after, lr, dtype):
    import torch
    t = lambda a: torch.from_numpy(np.array(a, dtype=dtype, copy=True).reshape(-1))     # noqa: E731
    par = torch.nn.Parameter(t(p))
    opt = torch.optim.Adam([par], lr=lr)
    # the counter is held in fp64: torch's own fp32 counter cannot hold 2^31 + 5, and the bias corrections are Python floats either way
    opt.state[par] = {"step": torch.tensor(float(step_after - 1), dtype=torch.float64), "exp_avg": t(m), "exp_avg_sq": t(v)}
    par.grad = t(g)
    opt.step()
    st = opt.state[par]
    assert float(st["step"]) == float(step_after)
    shp = np.shape(p)
    return tuple(x.detach().numpy().reshape(shp).copy() for x in (par, st["exp_avg"], st["exp_avg_sq"]))


def adam_bounds(p, m, v, g, step_after, lr=1e-4):
    """(bp, bm, bv): per-element bounds on |fp32 step - adam_fp64| for p', m', v' (fp64 arrays); the module docstring counts the roundings."""
    p, m, v, g = _f64(p, m, v, g)
    t = float(step_after)
    p1, m1, v1 = adam_fp64(p, m, v, g, step_after, lr)
    bm = 3 * U * (np.abs(m) + np.abs(g)) + 2.0 ** -126
    bv = 4 * U * (v + g * g) + 1e-37
    bs = np.sqrt(1.0 - B2 ** t)
    step_size = lr / (1.0 - B1 ** t)
    den = np.sqrt(v1) / bs + EPS
    dden = (np.sqrt(v1 + bv) - np.sqrt(np.maximum(v1 - bv, 0.0))) / bs + 6 * U * den
    q = np.abs(m1) / den
    bq = bm / den + q * dden / den + 2 * U * q
    bp = U * np.abs(p1) + step_size * (bq + 2 * U * q)
    return bp, bm, bv


def synthetic_moments(rng, n):
    """Moments as the tests draw them: s = 10^U(-12, -1), v = s^2, m = s U(-1, 1) — |m| <= sqrt(v), so one update moves a weight by at most
    ~lr / (1 - 0.9^t) sqrt(1 - 0.999^t) (a larger |m| / sqrt(v) would throw it past the |w| >= 8 range flag of the f16x3 images)."""
    s = 10.0 ** rng.uniform(-12.0, -1.0, n)
    m = (s * rng.uniform(-1.0, 1.0, n)).astype(np.float32)
    v = (s * s).astype(np.float32)
    v = np.maximum(v, (m.astype(np.float64) ** 2).astype(np.float32))        # keep |m| <= sqrt(v) after the fp32 roundings too
    v = np.where(v.astype(np.float64) < m.astype(np.float64) ** 2, np.nextafter(v, np.float32(np.inf)), v).astype(np.float32)
    return m, v
