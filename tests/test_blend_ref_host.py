"""tests/blend_ref.py on the CPU: the exact float32 fma, and that the compose check of the GPU tests can fail."""
import numpy as np

import blend_ref as B


def test_fma32_rounds_once():
    """a * b + c just below the midpoint of two float32: float64 rounds the sum onto the midpoint and the tie then goes to even, one step
    too high; the exact restatement stays below."""
    one, e = np.float32(1), np.float32(2.0 ** -23)
    a, b, c = np.float32((1 + 2.0 ** -23) * 2.0 ** -24), one - e, one + e
    assert np.float32(float(a) * float(b) + float(c)) == one + 2 * e
    assert B.fma32(a, b, c) == one + e
    assert B.fma32(np.float32(3), np.float32(5), np.float32(-15)) == 0 and B.fma32(a, np.float32(0), c) == c


def test_the_compose_check_can_fail():
    rng = np.random.default_rng(3)
    alpha = rng.uniform(0.001, 0.991, (24, 40)).astype(np.float32)
    rgb1, rgb2 = rng.uniform(0, 1, (2, 24, 40, 3)).astype(np.float32)
    flat = (alpha.reshape(-1), rgb1.reshape(-1, 3), rgb2.reshape(-1, 3))
    good = B.blend(*flat).reshape(24, 40, 3)
    assert (B.composes(good, alpha, rgb1, rgb2) == 0).all()
    up = np.nextafter(alpha, np.float32(1))       # the alpha one step away, as the finish kernel's can be
    steps = B.composes(B.blend(up.reshape(-1), *flat[1:]).reshape(24, 40, 3), alpha, rgb1, rgb2)
    assert (np.abs(steps) <= 1).all() and (steps == 1).any()       # some pixels give the same bits with several alphas
    L = {"alpha": alpha, "rgb1": rgb1, "rgb2": rgb2}
    assert B.check_composes(good, L, "written-out blend") == 0
    swapped = B.blend_swapped(*flat).reshape(24, 40, 3)      # channel 1 fused, channels 0 and 2 not
    none = int((B.composes(swapped, alpha, rgb1, rgb2) == B.NO_ALPHA).sum())
    assert none > alpha.size // 4, none
    try:
        B.check_composes(swapped, L, "swapped forms")
    except AssertionError:
        return
    raise AssertionError("the swapped forms passed the compose check")
