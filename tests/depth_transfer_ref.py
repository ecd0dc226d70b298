"""numpy restatement of the deep apply (csrc/guided.hip k_guided_apply16, include/atlasfit.h af_guided_apply16) and of the depth transfer
built on it (guided.py depth_transfer), with an fp64 twin.  Does not import the product.

The coefficient planes are those of the 8-bit pair: tests/guided_transfer_ref.py's coeffs / coeffs64 and its bilinear sampling, imported.
Only the last step is restated here, operation by operation in fp32: f = (float)min(F, M), s = (float)(M / 255.0), p = abar * f,
q = bbar * s, t = p + q, out = clamp(rint(f + t), 0, M), rounding half to even."""
import numpy as np

import guided_transfer_ref as G

F32 = np.float32


def maxv(bits):
    return (1 << bits) - 1


def scale(bits):
    return F32(np.float64(maxv(bits)) / np.float64(255.0))      # exactly 1 at 8 bits, 257 at 16


def apply16(full16, bits, abar, bbar):
    assert full16.dtype == np.uint16
    H, W = full16.shape[:2]
    m = maxv(bits)
    f = np.minimum(full16, m).astype(F32)
    a, b = G._bilinear(abar, H, W), G._bilinear(bbar, H, W)
    assert a.dtype == F32 and b.dtype == F32
    p = (a * f).astype(F32)
    q = (b * scale(bits)).astype(F32)
    t = (p + q).astype(F32)
    v = np.rint((f + t).astype(F32))
    v = np.where(v > 0, np.where(v < F32(m), v, F32(m)), F32(0))      # the kernel's comparisons: a NaN becomes 0
    return v.astype(np.uint16)


def transfer16(full16, bits, proxy_in, proxy_out, r, eps):
    abar, bbar = G.coeffs(proxy_in, proxy_out, r, eps)
    return apply16(full16, bits, abar, bbar)


def transfer16_64(full16, bits, proxy_in, proxy_out, r, eps, unrounded=False):
    """The fp64 twin: exact box means, fp64 throughout, M / 255 in fp64; with `unrounded` the real-valued result before rounding."""
    abar, bbar = G.coeffs64(proxy_in, proxy_out, r, eps)
    H, W = full16.shape[:2]
    m = maxv(bits)
    f = np.minimum(full16, m).astype(np.float64)
    v = f + (G._bilinear(abar, H, W, np.float64) * f + G._bilinear(bbar, H, W, np.float64) * (np.float64(m) / 255.0))
    return v if unrounded else np.clip(np.rint(v), 0, m).astype(np.uint16)


def reduce_depth(v, bits):
    m = maxv(bits)
    x = np.minimum(np.asarray(v), m).astype(np.int64)
    return ((510 * x + m) // (2 * m)).astype(np.uint8)


def deepen(frame8, bits, seed):
    """A deep frame whose 8-bit reduction is close to frame8: 2^(bits - 8) * frame + seeded noise below that factor."""
    up = 1 << (bits - 8)
    rng = np.random.default_rng(seed)
    return (frame8.astype(np.uint16) * up + rng.integers(0, up, frame8.shape).astype(np.uint16)).astype(np.uint16)
