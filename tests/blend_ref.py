"""Test helper (not a test module): k_frame_finish_at's fg/bg blend restated exactly on float32 arrays, and the check that a rendered
frame is that blend of render_layers' values.

The kernel writes every rounding out (elem.hip, fp contract off): w2 = fl(1 - alpha), bg = fl(rgb2 * w2), channel 1 = fl(fl(rgb1 * alpha)
+ bg), channels 0 and 2 = fma(alpha, rgb1, bg) with one rounding.  The fma is restated with exact rational arithmetic: a float64
product-and-add rounds twice on the way to float32.

The alpha is not quite render_layers': k_layer_finish (contraction on) computes alpha = fl(h * 0.99 + 0.001) in one fma, the finish kernel
fl(fl(h * 0.99) + 0.001).  h * 0.99 is smaller than the sum, so rounding it moves the sum by at most half an ulp of alpha, and the two
final roundings land within two float32 steps of each other (one, away from a power of two).  So a pixel composes if one alpha within
two steps of render_layers' gives all three of its channels bit for bit."""
from fractions import Fraction

import numpy as np

NO_ALPHA = 99       # composes(): no alpha within reach gives the pixel
REACH = 2


def fma32(a, b, c):
    """The correctly rounded float32 a * b + c of float32 arrays, element by element.  The float64 sum of the exact float64 product
    lies within a float32 step of it; the exact rational value picks among that float32 and its two neighbours, ties to even."""
    a, b, c = (np.asarray(x, np.float32) for x in np.broadcast_arrays(a, b, c))
    out = np.empty(a.shape, np.float32)
    for i in np.ndindex(a.shape):
        fa, fb, fc = float(a[i]), float(b[i]), float(c[i])
        x = Fraction(fa) * Fraction(fb) + Fraction(fc)
        r = np.float32(fa * fb + fc)
        cands = (np.nextafter(r, np.float32(-np.inf)), r, np.nextafter(r, np.float32(np.inf)))
        out[i] = min(cands, key=lambda q: (abs(Fraction(float(q)) - x), int(q.view(np.uint32)) & 1))
    return out


def blend(alpha, rgb1, rgb2):
    """(n, 3) float32: the kernel's blend of alpha (n,), rgb1, rgb2 (n, 3)."""
    a = alpha[:, None]
    bg = (rgb2 * (np.float32(1) - a).astype(np.float32)).astype(np.float32)
    out = np.empty_like(bg)
    out[:, 1] = ((rgb1[:, 1] * alpha).astype(np.float32) + bg[:, 1]).astype(np.float32)
    out[:, ::2] = fma32(a, rgb1[:, ::2], bg[:, ::2])
    return out


def blend_swapped(alpha, rgb1, rgb2):
    """blend with the forms of channel 1 and of channels 0 / 2 exchanged: what composes() must not accept."""
    a = alpha[:, None]
    bg = (rgb2 * (np.float32(1) - a).astype(np.float32)).astype(np.float32)
    out = ((rgb1 * a).astype(np.float32) + bg).astype(np.float32)
    out[:, 1] = fma32(alpha, rgb1[:, 1], bg[:, 1])
    return out


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def composes(rgb, alpha, rgb1, rgb2, blend=blend):
    """Per pixel of rgb (h, w, 3), the number of float32 steps (0, +-1, +-2; the nearest first) from alpha (h, w) to an alpha with which
    blend(alpha', rgb1, rgb2) is the pixel bit for bit in all three channels: (h, w) ints, NO_ALPHA where no alpha within REACH does."""
    rgb, rgb1, rgb2, alpha = rgb.reshape(-1, 3), rgb1.reshape(-1, 3), rgb2.reshape(-1, 3), alpha.reshape(-1)
    steps = np.full(alpha.shape, NO_ALPHA)
    for k in sorted(range(-REACH, REACH + 1), key=abs):
        todo = np.flatnonzero(steps == NO_ALPHA)
        if todo.size == 0:
            break
        a = alpha[todo]
        for _ in range(abs(k)):
            a = np.nextafter(a, np.float32(np.inf if k > 0 else -np.inf))
        ok = (_bits(blend(a, rgb1[todo], rgb2[todo])) == _bits(rgb[todo])).all(axis=1)
        steps[todo[ok]] = k
    return steps


def two_ulp_rule(rgb, alpha, rgb1, rgb2):
    """The looser rule the compose tests held before the blend was written out, per element (h, w, 3) bool: rgb equals the unfused or one
    of the two fused float32 results on `alpha`, or lies within two ulps of the unfused one."""
    a = alpha[:, :, None]
    w2 = (np.float32(1) - a).astype(np.float32)
    p1, p2 = (rgb1 * a).astype(np.float32), (rgb2 * w2).astype(np.float32)
    plain = (p1 + p2).astype(np.float32)
    fused = (rgb1.astype(np.float64) * a.astype(np.float64) + p2.astype(np.float64)).astype(np.float32)
    fused2 = (rgb2.astype(np.float64) * w2.astype(np.float64) + p1.astype(np.float64)).astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(plain), np.abs(rgb)))
    return (rgb == plain) | (rgb == fused) | (rgb == fused2) | (np.abs(rgb - plain) <= 2 * ulp)


def check_composes(rgb, layers, what):
    """Assert that rgb is the kernel's blend of layers' alpha, rgb1, rgb2: every pixel composes exactly with render_layers' alpha or with
    one within REACH steps of it, and the pixels that need another alpha also pass the two-ulp rule on render_layers' alpha.  Returns
    the number of pixels that needed another alpha."""
    steps = composes(rgb, layers["alpha"], layers["rgb1"], layers["rgb2"]).reshape(layers["alpha"].shape)
    other = steps != 0
    loose = two_ulp_rule(rgb, layers["alpha"], layers["rgb1"], layers["rgb2"]).all(axis=2)
    print("%s: %d of %d pixels compose exactly with render_layers' alpha, %d with an alpha one or two steps away, %d with none"
          % (what, int((steps == 0).sum()), steps.size, int((other & (steps != NO_ALPHA)).sum()), int((steps == NO_ALPHA).sum())))
    assert (steps != NO_ALPHA).all(), (what, int((steps == NO_ALPHA).sum()))
    assert loose[other].all(), (what, int((~loose[other]).sum()))
    return int(other.sum())
