"""tests/adam_ref.py checked without the kernel: adam_fp64 restates torch.optim.Adam (run in fp64) to 1e-12, and torch.optim.Adam's own fp32 step —
the reference project's optimizer — lies inside adam_bounds at every element of p, m and v, at early and late steps, with zero and with non-zero
moments, on gradients spanning twelve decades and on exact zeros.  tests/test_gpu_adam.py holds k_adam to the same bounds.

Measured on the CPU (torch 2.x, this file's draws): torch's worst error / bound ratio is ~1.0 for p (the half-ulp term of the final subtraction
dominates whenever the update is below an ulp of p), ~0.33 for m and ~0.53 for v; no rounding count had to be raised."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref as R  # noqa: E402

N = 66000
STEPS = (1, 2, 4, 100000, 2 ** 31 + 6)


def _draw(seed, zero_moments):
    rng = np.random.default_rng(seed)
    p = (0.06 * rng.standard_normal(N)).astype(np.float32)
    g = (rng.standard_normal(N) * 10.0 ** rng.uniform(-12.0, 0.0, N)).astype(np.float32)
    g[1000:3000] = 0.0                                           # a block of exact zeros (a dead unit's gradients)
    if zero_moments:
        m = np.zeros(N, np.float32); v = np.zeros(N, np.float32)
    else:
        m, v = R.synthetic_moments(rng, N)
    return p, m, v, g


@pytest.mark.parametrize("zero_moments", [True, False])
@pytest.mark.parametrize("step_after", STEPS)
def test_fp64_restatement_and_fp32_bound(step_after, zero_moments):
    p, m, v, g = _draw(step_after % 1000 + 7 * zero_moments, zero_moments)
    assert np.all(np.abs(m.astype(np.float64)) <= np.sqrt(v.astype(np.float64)))
    ref = R.adam_fp64(p, m, v, g, step_after)
    t64 = R.adam_torch64(p, m, v, g, step_after)
    for name, a, b in zip("pmv", ref, t64):
        scale = np.maximum(np.abs(b), 1e-300)
        assert np.all(np.abs(a - b) <= 1e-12 * scale), (name, step_after, float((np.abs(a - b) / scale).max()))
    t32 = R.adam_torch32(p, m, v, g, step_after)
    bounds = R.adam_bounds(p, m, v, g, step_after)
    ratios = {}
    for name, a, r, b in zip("pmv", t32, ref, bounds):
        assert a.dtype == np.float32
        err = np.abs(a.astype(np.float64) - r)
        ratios[name] = float((err / b).max())
        bad = np.flatnonzero(err > b)
        assert bad.size == 0, (name, step_after, zero_moments, bad[:5], err[bad[:5]], b[bad[:5]])
    print("step %d, %s moments: torch fp32 worst error / bound: p %.3f m %.3f v %.3f"
          % (step_after, "zero" if zero_moments else "drawn", ratios["p"], ratios["m"], ratios["v"]))
    # where g == 0 and the moments are zero nothing moves, bit for bit (torch does not skip such parameters: the update is 0 / eps)
    if zero_moments:
        z = g == 0
        assert z.sum() >= 2000
        for a, b in zip(t32, (p, m, v)):
            assert np.array_equal(a[z].view(np.uint32), b[z].view(np.uint32))


def test_bound_is_tight_enough_to_see_a_wrong_formula():
    """What the bound is for: an eps on the wrong side of the square root, a bias correction frozen at step 1, or moments that do not decay where
    g == 0 each leave it at a large share of the elements."""
    p, m, v, g = _draw(3, False)
    t = 100000
    bp, bm, bv = R.adam_bounds(p, m, v, g, t)
    p1, m1, v1 = R.adam_fp64(p, m, v, g, t)
    bc1, bc2 = 1 - 0.9 ** t, 1 - 0.999 ** t
    wrong_eps = p - 1e-4 / bc1 * m1 / np.sqrt(v1 / bc2 + 1e-8)
    assert (np.abs(wrong_eps - p1) > bp).mean() > 0.3
    frozen = p - 1e-4 / (1 - 0.9) * m1 / (np.sqrt(v1) / np.sqrt(1 - 0.999) + 1e-8)
    assert (np.abs(frozen - p1) > bp).mean() > 0.3
    z = g == 0
    assert (np.abs(m[z].astype(np.float64) - m1[z]) > bm[z]).mean() > 0.99
    assert (np.abs(v[z].astype(np.float64) - v1[z]) > bv[z]).mean() > 0.99
