"""A numpy restatement of the mask propagation kernels (csrc/maskprop.hip, include/atlasfit.h af_mask_step / af_mask_blend, DESIGN.md
§2.15): every operation is one np.float32 operation in the order the kernel performs it, so the GPU tests demand equality bit for bit.
`step64` / `blend64` evaluate the same formulas in fp64 at the same fp32 look-up position q: the restatement's own error bound."""
import numpy as np

F = np.float32


def _taps(f_ts, h, w):
    """q = (x, y) + f_ts as fp32 adds, the inside test (false for a NaN), the four tap indices and the fractions; taps are clamped into
    the frame everywhere so that the arrays can be indexed, and only the inside pixels are used."""
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        qx = xs.astype(F) + f_ts[..., 0]
        qy = ys.astype(F) + f_ts[..., 1]
        inside = (qx >= F(0)) & (qx <= F(w - 1)) & (qy >= F(0)) & (qy <= F(h - 1))
    sx, sy = np.where(inside, qx, F(0)), np.where(inside, qy, F(0))
    x0, y0 = sx.astype(np.int64), sy.astype(np.int64)      # truncation: q >= 0 here
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = sx - x0.astype(F), sy - y0.astype(F)
    return inside, (x0, x1, y0, y1), ax, ay


def _bil(v, taps, ax, ay, one):
    """top = v00 (1 - ax) + v01 ax, bot alike, top (1 - ay) + bot ay: each product and sum rounded in v's precision."""
    x0, x1, y0, y1 = taps
    bx, by = one - ax, one - ay
    top = v[y0, x0] * bx + v[y0, x1] * ax
    bot = v[y1, x0] * bx + v[y1, x1] * ax
    return top * by + bot * ay


def step(m_s, c_s, f_ts, f_st, thresh=1.0):
    """af_mask_step in fp32 -> (m_t, c_t)."""
    h, w = m_s.shape
    assert m_s.dtype == c_s.dtype == f_ts.dtype == f_st.dtype == F
    inside, taps, ax, ay = _taps(f_ts, h, w)
    thresh2 = F(F(thresh) * F(thresh))
    with np.errstate(invalid="ignore", over="ignore"):
        dx = f_ts[..., 0] + _bil(f_st[..., 0], taps, ax, ay, F(1))
        dy = f_ts[..., 1] + _bil(f_st[..., 1], taps, ax, ay, F(1))
        ok = inside & (dx * dx + dy * dy < thresh2)
        m_t = np.where(ok, _bil(m_s, taps, ax, ay, F(1)), m_s)
        c_t = np.where(ok, _bil(c_s, taps, ax, ay, F(1)), F(0))
    assert m_t.dtype == c_t.dtype == F
    return m_t, c_t


def step64(m_s, c_s, f_ts, f_st, thresh=1.0):
    """The same formulas with every product and sum in fp64, at the fp32 q (and so the fp32 fractions, which are exact differences)
    -> (m_t, c_t, ok, margin): margin = | round-trip norm^2 - thresh^2 | in fp64, how far a pixel is from the other branch."""
    h, w = m_s.shape
    inside, taps, ax, ay = _taps(f_ts, h, w)
    ax, ay = ax.astype(np.float64), ay.astype(np.float64)
    d = lambda v: v.astype(np.float64)      # noqa: E731
    with np.errstate(invalid="ignore", over="ignore"):
        dx = d(f_ts[..., 0]) + _bil(d(f_st[..., 0]), taps, ax, ay, 1.0)
        dy = d(f_ts[..., 1]) + _bil(d(f_st[..., 1]), taps, ax, ay, 1.0)
        n2 = dx * dx + dy * dy
        ok = inside & (n2 < float(F(F(thresh) * F(thresh))))
        m_t = np.where(ok, _bil(d(m_s), taps, ax, ay, 1.0), d(m_s))
        c_t = np.where(ok, _bil(d(c_s), taps, ax, ay, 1.0), 0.0)
    return m_t, c_t, ok, np.abs(n2 - float(thresh) ** 2)


def _clamp(v, zero, one):
    """v < 0 ? 0 : (v > 1 ? 1 : v): by comparisons, a NaN stays one."""
    with np.errstate(invalid="ignore"):
        return np.where(v < zero, zero, np.where(v > one, one, v))


def blend(m_f, c_f, m_b, c_b, a, t, b):
    """af_mask_blend in fp32."""
    assert a < t < b and m_f.dtype == c_f.dtype == m_b.dtype == c_b.dtype == F
    to_b, from_a, span = F(b - t), F(t - a), F(b - a)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        wf, wb = to_b * c_f, from_a * c_b
        s = wf + wb
        weighted = (wf * m_f + wb * m_b) / s
        plain = (to_b * m_f + from_a * m_b) / span
        out = _clamp(np.where(s > F(0), weighted, plain), F(0), F(1))
    assert out.dtype == F
    return out


def blend64(m_f, c_f, m_b, c_b, a, t, b):
    d = lambda v: v.astype(np.float64)      # noqa: E731
    m_f, c_f, m_b, c_b = d(m_f), d(c_f), d(m_b), d(c_b)
    with np.errstate(invalid="ignore", divide="ignore"):
        wf, wb = (b - t) * c_f, (t - a) * c_b
        s = wf + wb
        return _clamp(np.where(s > 0, (wf * m_f + wb * m_b) / s, ((b - t) * m_f + (t - a) * m_b) / (b - a)), 0.0, 1.0)


def propagate(keys, flows12, flows21, thresh=1.0):
    """The masks of one shot of n = len(flows12) + 1 frames from its key masks, written frame by frame and not through the planner:
    frame t between keys a < t < b is the blend of the chain walked forward from a and the chain walked backward from b, a frame before
    the first key hangs on the backward chain from it, a frame behind the last key on the forward chain from it.  -> (n, h, w)."""
    n, ks = len(flows12) + 1, sorted(keys)
    fwd = lambda m, c, i: step(m, c, flows21[i], flows12[i], thresh)        # noqa: E731  frame i -> i + 1
    bwd = lambda m, c, i: step(m, c, flows12[i], flows21[i], thresh)        # noqa: E731  frame i + 1 -> i
    out = [None] * n
    for k in ks:
        out[k] = keys[k]
    m, c = keys[ks[0]], np.ones_like(keys[ks[0]])
    for t in range(ks[0] - 1, -1, -1):
        m, c = bwd(m, c, t)
        out[t] = m
    m, c = keys[ks[-1]], np.ones_like(keys[ks[-1]])
    for t in range(ks[-1] + 1, n):
        m, c = fwd(m, c, t - 1)
        out[t] = m
    for a, b in zip(ks[:-1], ks[1:]):
        f, r = {a: (keys[a], np.ones_like(keys[a]))}, {b: (keys[b], np.ones_like(keys[b]))}
        for t in range(a + 1, b):
            f[t] = fwd(f[t - 1][0], f[t - 1][1], t - 1)
        for t in range(b - 1, a, -1):
            r[t] = bwd(r[t + 1][0], r[t + 1][1], t)
        for t in range(a + 1, b):
            out[t] = blend(f[t][0], f[t][1], r[t][0], r[t][1], a, t, b)
    return np.stack(out)
