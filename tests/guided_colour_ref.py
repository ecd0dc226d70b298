"""numpy restatement of the guided transfer with a colour guide (csrc/guided.hip, include/atlasfit.h af_guided_coeffs_colour /
af_guided_apply_colour / af_guided_apply_colour16) and its fp64 twin.  Does not import the product.

The restatement performs the kernels' operations one by one: exact integer sums, then the header's LDL^T sequence with every fp64
operation a separate numpy operation (numpy fuses nothing), one rounding of x and b to fp32, the fp32 box means of
tests/guided_transfer_ref.py and the apply's fp32 steps in the kernel's order, so a GPU result may be compared bit for bit.  The twin
computes the same definition with numpy.linalg.solve and exact box means, fp64 throughout."""
import numpy as np

import guided_transfer_ref as G

F32, F64 = np.float32, np.float64
EPS_FLOOR = 2.0 ** -20
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # the order of S_cc'


def window_n(h, w, r):
    return (G._window_counts(h, r)[:, None] * G._window_counts(w, r)[None, :]).astype(np.int64)


def sums(proxy_in, proxy_out, r):
    """(n, S_c (h, w, 3), S_dk (h, w, 3), S_cc' (h, w, 6), S_c,dk (h, w, 3 [k], 3 [c])): exact, int64; each fits the kernel's int32."""
    i = proxy_in.astype(np.int64)
    d = proxy_out.astype(np.int64) - i
    h, w = i.shape[:2]
    s_c, s_d = G._box_int(i, r), G._box_int(d, r)
    s_cc = G._box_int(np.stack([i[..., u] * i[..., v] for u, v in PAIRS], -1), r)
    s_cd = G._box_int(d[..., :, None] * i[..., None, :], r)
    assert max(np.abs(s).max() for s in (s_c, s_d, s_cc, s_cd)) < 2 ** 31
    return window_n(h, w, r), s_c, s_d, s_cc, s_cd


def raw_coeffs(proxy_in, proxy_out, r, eps, pivots=False):
    """The unsmoothed (A (h, w, 9), b (h, w, 3)) float32; with `pivots` also (d0, d1, d2, e) in fp64."""
    n, s_c, s_d, s_cc, s_cd = sums(proxy_in, proxy_out, r)
    sig = [n * s_cc[..., q] - s_c[..., u] * s_c[..., v] for q, (u, v) in enumerate(PAIRS)]
    assert max(np.abs(s).max() for s in sig) < 2 ** 53
    nd = n.astype(F64)
    e = F64(F32(eps)) * (n * n).astype(F64)
    m00, m01, m02, m11, m12, m22 = (s.astype(F64) for s in sig)
    m00, m11, m22 = m00 + e, m11 + e, m22 + e
    d0 = m00
    l10 = m01 / d0
    l20 = m02 / d0
    d1 = m11 - l10 * m01
    t21 = m12 - l20 * m01
    l21 = t21 / d1
    d2 = (m22 - l20 * m02) - l21 * t21
    h, w = n.shape
    A, b = np.zeros((h, w, 9), F32), np.zeros((h, w, 3), F32)
    s0, s1, s2 = (s_c[..., c].astype(F64) for c in range(3))
    for k in range(3):
        kap = [n * s_cd[..., k, c] - s_c[..., c] * s_d[..., k] for c in range(3)]
        assert max(np.abs(v).max() for v in kap) < 2 ** 53
        z0 = kap[0].astype(F64)
        z1 = kap[1].astype(F64) - l10 * z0
        z2 = (kap[2].astype(F64) - l20 * z0) - l21 * z1
        x2 = z2 / d2
        x1 = z1 / d1 - l21 * x2
        x0 = (z0 / d0 - l10 * x1) - l20 * x2
        bk = (s_d[..., k].astype(F64) - ((x0 * s0 + x1 * s1) + x2 * s2)) / nd
        A[..., 3 * k], A[..., 3 * k + 1], A[..., 3 * k + 2] = x0.astype(F32), x1.astype(F32), x2.astype(F32)
        b[..., k] = bk.astype(F32)
    return (A, b, (d0, d1, d2, e)) if pivots else (A, b)


def coeffs(proxy_in, proxy_out, r, eps):
    """The smoothed planes (A (h, w, 9), b (h, w, 3)) float32: what af_guided_coeffs_colour returns."""
    A, b = raw_coeffs(proxy_in, proxy_out, r, eps)
    nf = window_n(*proxy_in.shape[:2], r)[:, :, None].astype(F32)
    return (G._box_f32(A, r) / nf).astype(F32), (G._box_f32(b, r) / nf).astype(F32)


def _steps(f, A, b, offset_scale=None):
    """t = A_k0 f_0; t = t + A_k1 f_1; t = t + A_k2 f_2; t = t + b_k [s]; f_k + t, each one fp32 operation; (H, W, 3) before rint."""
    out = np.zeros(f.shape, F32)
    for k in range(3):
        t = (A[..., 3 * k] * f[..., 0]).astype(F32)
        t = (t + (A[..., 3 * k + 1] * f[..., 1]).astype(F32)).astype(F32)
        t = (t + (A[..., 3 * k + 2] * f[..., 2]).astype(F32)).astype(F32)
        off = b[..., k] if offset_scale is None else (b[..., k] * offset_scale).astype(F32)
        t = (t + off).astype(F32)
        out[..., k] = (f[..., k] + t).astype(F32)
    return out


def _clamp(v, m):
    return np.where(v > 0, np.where(v < F32(m), v, F32(m)), F32(0))      # the kernel's comparisons: a NaN becomes 0


def apply(full, A, b):
    """af_guided_apply_colour."""
    H, W = full.shape[:2]
    As, bs = G._bilinear(A, H, W), G._bilinear(b, H, W)
    assert As.dtype == F32 and bs.dtype == F32
    return _clamp(np.rint(_steps(full.astype(F32), As, bs)), 255).astype(np.uint8)


def apply16(full16, bits, A, b):
    """af_guided_apply_colour16."""
    assert full16.dtype == np.uint16
    H, W = full16.shape[:2]
    m = (1 << bits) - 1
    s = F32(F64(m) / F64(255.0))
    As, bs = G._bilinear(A, H, W), G._bilinear(b, H, W)
    return _clamp(np.rint(_steps(np.minimum(full16, m).astype(F32), As, bs, s)), m).astype(np.uint16)


def transfer(full, proxy_in, proxy_out, r, eps):
    return apply(full, *coeffs(proxy_in, proxy_out, r, eps))


def transfer16(full16, bits, proxy_in, proxy_out, r, eps):
    return apply16(full16, bits, *coeffs(proxy_in, proxy_out, r, eps))


def unrounded(full, A, b):
    """The restatement's value before rint and the clamp, as fp64 of its fp32 steps."""
    H, W = full.shape[:2]
    return _steps(full.astype(F32), G._bilinear(A, H, W), G._bilinear(b, H, W)).astype(F64)


# ---- the fp64 twin: numpy.linalg.solve, exact box means, fp64 throughout ------------------------------------------------------------
def coeffs64(proxy_in, proxy_out, r, eps):
    n, s_c, s_d, s_cc, s_cd = sums(proxy_in, proxy_out, r)
    h, w = n.shape
    nd = n.astype(F64)
    sig = np.zeros((h, w, 3, 3))
    for q, (u, v) in enumerate(PAIRS):
        sig[..., u, v] = sig[..., v, u] = (n * s_cc[..., q] - s_c[..., u] * s_c[..., v]).astype(F64)
    sig = sig + (F64(F32(eps)) * nd * nd)[..., None, None] * np.eye(3)
    kap = (n[..., None, None] * s_cd - s_d[..., :, None] * s_c[..., None, :]).astype(F64)      # [k][c]
    x = np.linalg.solve(sig, np.swapaxes(kap, -1, -2))                                           # [c][k]
    A = np.swapaxes(x, -1, -2).reshape(h, w, 9)                                                  # 3k + c
    b = (s_d.astype(F64) - np.einsum("hwkc,hwc->hwk", A.reshape(h, w, 3, 3), s_c.astype(F64))) / nd[..., None]

    def mean(v):
        pad = np.zeros((h + 2 * r, w + 2 * r, v.shape[2]))
        pad[r:r + h, r:r + w] = v
        return sum(pad[r + dy:r + dy + h, r + dx:r + dx + w] for dy in range(-r, r + 1) for dx in range(-r, r + 1)) / nd[..., None]
    return mean(A), mean(b)


def transfer64(full, proxy_in, proxy_out, r, eps, unrounded=False):
    """The twin's output; with `unrounded` the real-valued F + (A F + b) before rounding and clamping."""
    A, b = coeffs64(proxy_in, proxy_out, r, eps)
    H, W = full.shape[:2]
    f = full.astype(F64)
    As, bs = G._bilinear(A, H, W, F64).reshape(H, W, 3, 3), G._bilinear(b, H, W, F64)
    v = f + (np.einsum("hwkc,hwc->hwk", As, f) + bs)
    return v if unrounded else np.clip(np.rint(v), 0, 255).astype(np.uint8)


# ---- the cases the colour tests add to guided_transfer_ref.CASES -------------------------------------------------------------------
MATRIX = np.array([[1.04, 0.05, -0.03], [-0.04, 0.98, 0.06], [0.03, -0.05, 1.05]])      # P_k = sum_c I_c MATRIX[c][k] + OFFSET[k]
OFFSET = np.array([4.0, -3.0, 2.0])


def make_grey():
    """(full, proxy_in, proxy_out): a 48 x 64 guide with three equal channels under a 96 x 128 frame; the worst-conditioned solve."""
    rng = np.random.RandomState(sum(map(ord, "grey")))
    y, x = np.mgrid[0:96, 0:128]
    g = np.clip(128 + 90 * np.sin(x / 11.0) * np.cos(y / 8.0) + rng.randint(-15, 16, (96, 128)), 0, 255).astype(np.uint8)
    full = np.repeat(g[:, :, None], 3, 2)
    i = G.area_shrink(full, 48, 64)
    gain = 1.0 + 0.1 * np.sin(np.mgrid[0:48, 0:64][1] / 19.0)
    p = np.clip(np.rint(i * gain[:, :, None] + np.array([6.0, -4.0, 9.0]) + rng.randint(-2, 3, i.shape)), 0, 255).astype(np.uint8)
    return full, i, p


def make_matrix():
    """(full, proxy_in, proxy_out, exact): a 96 x 128 picture in 40..215 (nothing clips under MATRIX and OFFSET), its 2 x 2 area shrink as
    the proxy, P = rint(I MATRIX + OFFSET), and the exact full-size answer F MATRIX + OFFSET in fp64."""
    rng = np.random.RandomState(sum(map(ord, "matrix")))
    y, x = np.mgrid[0:96, 0:128]
    base = np.stack([128 + 70 * np.sin(x / (9.0 + 2 * c) + c) * np.cos(y / (7.0 + c) - 2 * c) for c in range(3)], -1)
    full = np.clip(np.rint(base + rng.randint(-15, 16, base.shape)), 40, 215).astype(np.uint8)
    i = np.rint(full.astype(F64).reshape(48, 2, 64, 2, 3).mean((1, 3))).astype(np.uint8)
    pv = i.astype(F64) @ MATRIX + OFFSET
    assert pv.min() >= 0 and pv.max() <= 255
    exact = full.astype(F64) @ MATRIX + OFFSET
    assert exact.min() >= 0 and exact.max() <= 255
    return full, i, np.rint(pv).astype(np.uint8), exact
