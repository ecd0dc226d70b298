"""numpy restatement of the residual guided transfer (csrc/guided.hip, include/atlasfit.h af_guided_coeffs / af_guided_apply) and its fp64
twin.  Does not import the product.

The restatement performs the kernels' operations one by one, each a single correctly rounded fp32 (or exact integer) operation in the
kernels' order, so a GPU result may be compared bit for bit.  The twin computes the same definition in fp64 with exact box means."""
import numpy as np

F32 = np.float32


def _window_counts(size, r):
    p = np.arange(size)
    return np.minimum(p + r, size - 1) - np.maximum(p - r, 0) + 1


def _box_int(v, r):
    """Exact sums over the (2r + 1)^2 window clipped to the frame, int64 (zeros outside add nothing)."""
    h, w = v.shape[:2]
    pad = np.zeros((h + 2 * r, w + 2 * r) + v.shape[2:], np.int64)
    pad[r:r + h, r:r + w] = v
    c = np.cumsum(np.cumsum(pad, 0), 1)
    c = np.pad(c, [(1, 0), (1, 0)] + [(0, 0)] * (v.ndim - 2))
    k = 2 * r + 1
    return c[k:k + h, k:k + w] - c[:h, k:k + w] - c[k:k + h, :w] + c[:h, :w]


def _box_f32(v, r):
    """The kernel's fp32 box sum: along each row left to right from 0 over the clipped window, then down the rows top to bottom from 0."""
    h, w = v.shape[:2]
    tail = (1,) * (v.ndim - 2)
    x = np.arange(w).reshape((1, w) + tail)
    rows = np.zeros(v.shape, F32)
    for k in range(-r, r + 1):
        src = np.clip(np.arange(w) + k, 0, w - 1)
        ok = (x + k >= 0) & (x + k <= w - 1)
        rows = np.where(ok, rows + v[:, src], rows).astype(F32)
    y = np.arange(h).reshape((h, 1) + tail)
    out = np.zeros(v.shape, F32)
    for k in range(-r, r + 1):
        src = np.clip(np.arange(h) + k, 0, h - 1)
        ok = (y + k >= 0) & (y + k <= h - 1)
        out = np.where(ok, out + rows[src], out).astype(F32)
    return out


def raw_coeffs(proxy_in, proxy_out, r, eps):
    """(a, b, n): the unsmoothed coefficients (h, w, 3) float32 and the window counts (h, w, 1) int64."""
    i = proxy_in.astype(np.int64)
    d = proxy_out.astype(np.int64) - i
    h, w = i.shape[:2]
    n = (_window_counts(h, r)[:, None] * _window_counts(w, r)[None, :])[:, :, None].astype(np.int64)
    s_i, s_d, s_ii, s_id = _box_int(i, r), _box_int(d, r), _box_int(i * i, r), _box_int(i * d, r)
    assert max(np.abs(s).max() for s in (s_i, s_d, s_ii, s_id)) < 2 ** 31      # the kernel holds them in int32
    num = n * s_id - s_i * s_d
    den = n * s_ii - s_i * s_i
    nn = (n * n).astype(F32)
    a = num.astype(F32) / (den.astype(F32) + F32(eps) * nn)
    b = (s_d.astype(F32) - a * s_i.astype(F32)) / n.astype(F32)
    return a.astype(F32), b.astype(F32), n


def coeffs(proxy_in, proxy_out, r, eps):
    """The smoothed planes (abar, bbar), (h, w, 3) float32: what af_guided_coeffs returns."""
    a, b, n = raw_coeffs(proxy_in, proxy_out, r, eps)
    nf = n.astype(F32)
    return (_box_f32(a, r) / nf).astype(F32), (_box_f32(b, r) / nf).astype(F32)


def axis_taps(dst, src):
    """(i0, i1, f) of the dst pixel centres on an axis of src samples: s = (X + 0.5) * (src / dst) - 0.5 in fp64, clamped to [0, src - 1]."""
    scale = np.float64(src) / np.float64(dst)
    s = (np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5
    s = np.minimum(np.maximum(s, 0.0), np.float64(src - 1))
    i0 = s.astype(np.int64)
    return i0, np.minimum(i0 + 1, src - 1), (s - i0.astype(np.float64)).astype(F32)


def _bilinear(v, H, W, dtype=F32):
    h, w = v.shape[:2]
    y0, y1, ay = axis_taps(H, h)
    x0, x1, ax = axis_taps(W, w)
    ax, ay = ax.astype(dtype)[None, :, None], ay.astype(dtype)[:, None, None]
    v = v.astype(dtype)
    v00, v01, v10, v11 = v[y0][:, x0], v[y0][:, x1], v[y1][:, x0], v[y1][:, x1]
    top = v00 + ax * (v01 - v00)
    bot = v10 + ax * (v11 - v10)
    return top + ay * (bot - top)


def apply(full, abar, bbar):
    """af_guided_apply: clamp(rint(F + (abar F + bbar)), 0, 255) with the planes sampled bilinearly, every step one fp32 operation."""
    H, W = full.shape[:2]
    f = full.astype(F32)
    a, b = _bilinear(abar, H, W), _bilinear(bbar, H, W)
    assert a.dtype == F32 and b.dtype == F32
    v = np.rint(f + (a * f + b))
    return np.clip(v, 0, 255).astype(np.uint8)


def transfer(full, proxy_in, proxy_out, r, eps):
    abar, bbar = coeffs(proxy_in, proxy_out, r, eps)
    return apply(full, abar, bbar)


# ---- the fp64 twin: the same definition, exact box means, fp64 throughout --------------------------------------------------------
def coeffs64(proxy_in, proxy_out, r, eps):
    i = proxy_in.astype(np.int64)
    d = proxy_out.astype(np.int64) - i
    h, w = i.shape[:2]
    n = (_window_counts(h, r)[:, None] * _window_counts(w, r)[None, :])[:, :, None].astype(np.float64)
    s_i, s_d, s_ii, s_id = (_box_int(v, r).astype(np.float64) for v in (i, d, i * i, i * d))
    a = (n * s_id - s_i * s_d) / ((n * s_ii - s_i * s_i) + np.float64(F32(eps)) * n * n)
    b = (s_d - a * s_i) / n

    def mean(v):
        pad = np.zeros((h + 2 * r, w + 2 * r, 3))
        pad[r:r + h, r:r + w] = v
        return sum(pad[r + dy:r + dy + h, r + dx:r + dx + w] for dy in range(-r, r + 1) for dx in range(-r, r + 1)) / n
    return mean(a), mean(b)


def transfer64(full, proxy_in, proxy_out, r, eps, unrounded=False):
    """The twin's output; with `unrounded` the real-valued F + (abar F + bbar) before rounding and clamping."""
    abar, bbar = coeffs64(proxy_in, proxy_out, r, eps)
    H, W = full.shape[:2]
    f = full.astype(np.float64)
    v = f + (_bilinear(abar, H, W, np.float64) * f + _bilinear(bbar, H, W, np.float64))
    return v if unrounded else np.clip(np.rint(v), 0, 255).astype(np.uint8)


# ---- the GPU tests' inputs, shared with the host tests ---------------------------------------------------------------------------
def area_shrink(full, h, w):
    """A stand-in for the proxy input where the exact area shrink does not matter: the nearest source pixel of every proxy pixel."""
    H, W = full.shape[:2]
    ys = (np.arange(h) * H) // h
    xs = (np.arange(w) * W) // w
    return full[ys][:, xs].copy()


def make_case(name):
    """(full, proxy_in, proxy_out, r) of a named case; eps is the caller's."""
    rng = np.random.RandomState(sum(map(ord, name)))

    def rnd(h, w):
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)

    def smooth(h, w):      # a picture with structure: low-frequency colour plus noise
        y, x = np.mgrid[0:h, 0:w]
        base = np.stack([128 + 100 * np.sin(x / 9.0 + c) * np.cos(y / 7.0 - c) for c in range(3)], -1)
        return np.clip(base + rng.randint(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)

    def flicker(i):        # a proxy output: the input under a gain and offset that drift across the frame, plus noise
        h, w = i.shape[:2]
        y, x = np.mgrid[0:h, 0:w]
        g = 1.0 + 0.15 * np.sin(x / 23.0)[:, :, None]
        o = 12.0 * np.cos(y / 17.0)[:, :, None]
        return np.clip(np.rint(i * g + o + rng.randint(-3, 4, i.shape)), 0, 255).astype(np.uint8)

    if name == "ratio":            # a non-integer ratio
        full = smooth(149, 211)
        i = area_shrink(full, 37, 53)
        return full, i, flicker(i), 8
    if name == "same":             # ratio 1: the taps coincide
        full = smooth(41, 67)
        return full, full.copy(), flicker(full), 8
    if name == "r1":
        full = smooth(90, 77)
        i = area_shrink(full, 45, 39)
        return full, i, flicker(i), 1
    if name == "r32":              # a 37-row proxy: the window is clipped on both sides
        full = smooth(74, 200)
        i = area_shrink(full, 37, 100)
        return full, i, flicker(i), 32
    if name == "tiles":            # crosses tile boundaries in both directions, width no multiple of 64
        full = smooth(140, 262)
        i = area_shrink(full, 70, 131)
        return full, i, flicker(i), 5
    if name == "one":              # a 1x1 proxy under a 2x3 frame
        return rnd(2, 3), rnd(1, 1), rnd(1, 1), 8
    if name == "extreme":          # the largest sums: pins the int32 claim
        return rnd(140, 141), np.full((70, 70, 3), 255, np.uint8), np.zeros((70, 70, 3), np.uint8), 32
    if name == "identity":
        full = smooth(101, 99)
        i = area_shrink(full, 50, 49)
        return full, i, i.copy(), 8
    if name == "random":
        return rnd(67, 130), rnd(33, 64), rnd(33, 64), 8
    if name == "wide":             # W a multiple of 4 (the 12-byte path) with a row count that is none, two workgroups across
        full = smooth(35, 516)
        i = area_shrink(full, 17, 129)
        return full, i, flicker(i), 3
    if name in ("w8", "w8_one", "w7", "w7_one"):      # H = 5 with W = 8 (one 12-byte group pair) and W = 7 (the tail of a group of four), over 3x2 and 1x1 proxies
        h, w = (1, 1) if name.endswith("_one") else (3, 2)
        return rnd(5, 8 if name.startswith("w8") else 7), rnd(h, w), rnd(h, w), 8
    raise KeyError(name)


CASES = ("ratio", "same", "r1", "r32", "tiles", "one", "extreme", "identity", "random", "wide", "w8", "w8_one", "w7", "w7_one")
EPS = 64.0
