"""YCbCr <-> RGB of a YUV4MPEG2 frame payload of D = 8..16 bits per sample, restated from the text of DESIGN.md §2.18 in whole-array numpy
int64, its fp64 "exact" twin at depth D, and the depth reduction.  Does not import the package: the kernels (csrc/yuv16.hip) are held
against this file bit for bit, this file at D = 8 against tests/y4m_ref.py bit for bit, and at every depth against the exact twin within
the bound read_bound / write_bound derive from the coefficient tables.

The planes, sitings, interpolation weights and filter taps are y4m_ref's (imported, not restated: they do not depend on the depth).
Payload: uint16 samples, the Y plane h x w, then Cb, then Cr, each ch x cw.  Image: (h, w, 3) uint16 RGB.  M = 2^D - 1; a stored sample
above M reads as M."""
from fractions import Fraction

import numpy as np

import y4m_ref as R8

LAYOUTS, MATRICES, AXES, K = R8.LAYOUTS, R8.MATRICES, R8.AXES, R8.K
DEPTHS = (8, 9, 10, 12, 14, 16)
plane_size, frame_samples = R8.plane_size, R8.frame_bytes      # counts of samples


def qbits(bits):
    return bits + 6                                       # fraction bits of the coefficients: 14 at D = 8


def maxv(bits):
    return (1 << bits) - 1


def scales(full_range, bits):
    """(y0, sy, sc, C): Y = sy Y' + y0, Cx = sc C' + C for Y' in [0, M], C' in [-M / 2, M / 2]."""
    c = 1 << (bits - 1)
    if full_range:
        return 0, Fraction(1), Fraction(1), c
    up = 1 << (bits - 8)
    return 16 * up, Fraction(219 * up, maxv(bits)), Fraction(224 * up, maxv(bits)), c


def real_matrices(matrix, full_range, bits):
    """Exact rationals: (forward 3 x 3 rows Y, Cb, Cr over R, G, B; inverse coefficients cy, crv, cgu, cgv, cbu)."""
    kr, kb = K[matrix]
    kg = 1 - kr - kb
    _, sy, sc, _ = scales(full_range, bits)
    fwd = [[kr * sy, kg * sy, kb * sy],
           [-kr / (2 * (1 - kb)) * sc, -kg / (2 * (1 - kb)) * sc, Fraction(1, 2) * sc],
           [Fraction(1, 2) * sc, -kg / (2 * (1 - kr)) * sc, -kb / (2 * (1 - kr)) * sc]]
    inv = (1 / sy, 2 * (1 - kr) / sc, -2 * (1 - kb) * kb / kg / sc, -2 * (1 - kr) * kr / kg / sc, 2 * (1 - kb) / sc)
    return fwd, inv


def int_matrices(matrix, full_range, bits):
    """The integer tables at Q = D + 6 fraction bits: rows rounded, then the largest entry of each forward row adjusted so that the luma
    row sums exactly to round(sy 2^Q) and each chroma row to 0."""
    q = qbits(bits)
    rnd = lambda v: int(round(v * (1 << q)))              # noqa: E731  Fraction: the exact value rounded (no tie occurs)
    fwd, inv = real_matrices(matrix, full_range, bits)
    sy = scales(full_range, bits)[1]
    rows = []
    for row, target in zip(fwd, (rnd(sy), 0, 0)):
        r = [rnd(v) for v in row]
        big = max(range(3), key=lambda k: abs(r[k]))
        r[big] += target - sum(r)
        rows.append(r)
    return rows, tuple(rnd(v) for v in inv)


def split(payload, h, w, layout, bits):
    p = np.asarray(payload)
    assert p.dtype == np.uint16 and p.size == frame_samples(h, w, layout), (p.dtype, p.size, frame_samples(h, w, layout))
    p = np.minimum(p.reshape(-1), maxv(bits)).astype(np.int64)
    ch, cw = plane_size(h, w, layout)
    y = p[:h * w].reshape(h, w)
    if layout == "mono":
        return y, None, None
    return y, p[h * w:h * w + ch * cw].reshape(ch, cw), p[h * w + ch * cw:].reshape(ch, cw)


# ---- reading ---------------------------------------------------------------------------------------------------------------------
def yuv_to_rgb(payload, h, w, layout, matrix, full_range, bits):
    y, cb, cr = split(payload, h, w, layout, bits)
    _, (cy, crv, cgu, cgv, cbu) = int_matrices(matrix, full_range, bits)
    y0, _, _, c = scales(full_range, bits)
    q = qbits(bits)
    lum = cy * 16 * (y - y0) + (1 << (q + 3))
    if layout == "mono":
        u = v = np.zeros((h, w), np.int64)
    else:
        u, v = R8.chroma16(cb, h, w, layout) - 16 * c, R8.chroma16(cr, h, w, layout) - 16 * c
    out = np.stack([lum + crv * v, lum + cgu * u + cgv * v, lum + cbu * u], -1) >> (q + 4)      # arithmetic shift: floor
    return np.clip(out, 0, maxv(bits)).astype(np.uint16)


def yuv_to_rgb_exact(payload, h, w, layout, matrix, full_range, bits):
    """fp64, unrounded: (h, w, 3) in [0, M]."""
    y, cb, cr = split(payload, h, w, layout, bits)
    _, inv = real_matrices(matrix, full_range, bits)
    cy, crv, cgu, cgv, cbu = (float(v) for v in inv)
    y0, _, _, c = scales(full_range, bits)
    lum = cy * (y.astype(np.float64) - y0)
    if layout == "mono":
        u = v = np.zeros((h, w))
    else:
        u, v = R8.chroma16(cb, h, w, layout, np.float64) / 16.0 - c, R8.chroma16(cr, h, w, layout, np.float64) / 16.0 - c
    return np.clip(np.stack([lum + crv * v, lum + cgu * u + cgv * v, lum + cbu * u], -1), 0.0, float(maxv(bits)))


# ---- writing ---------------------------------------------------------------------------------------------------------------------
def _rgb(rgb, bits):
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint16 and rgb.ndim == 3 and rgb.shape[2] == 3
    return np.minimum(rgb, maxv(bits)).astype(np.int64)


def rgb_to_yuv(rgb, layout, matrix, full_range, bits):
    p = _rgb(rgb, bits)
    h, w = p.shape[:2]
    (ky, ku, kv), _ = int_matrices(matrix, full_range, bits)
    y0, _, _, c = scales(full_range, bits)
    q, m = qbits(bits), maxv(bits)
    y = np.clip(((p @ np.array(ky) + (1 << (q - 1))) >> q) + y0, 0, m).astype(np.uint16)
    planes = [y.reshape(-1)]
    if layout != "mono":
        for k in (ku, kv):
            s, sh = R8._filter(p @ np.array(k), h, w, layout)            # unrounded per pixel, filtered, rounded once
            planes.append(np.clip(((s + (1 << (q + sh - 1))) >> (q + sh)) + c, 0, m).astype(np.uint16).reshape(-1))
    return np.concatenate(planes)


def rgb_to_yuv_exact(rgb, layout, matrix, full_range, bits):
    """fp64, unrounded: the payload's values in [0, M], planes concatenated as in the payload."""
    p = _rgb(rgb, bits).astype(np.float64)
    h, w = p.shape[:2]
    fwd, _ = real_matrices(matrix, full_range, bits)
    y0, _, _, c = scales(full_range, bits)
    m = float(maxv(bits))
    planes = [np.clip(p @ np.array([float(v) for v in fwd[0]]) + y0, 0.0, m).reshape(-1)]
    if layout != "mono":
        for row in fwd[1:]:
            s, sh = R8._filter(p @ np.array([float(v) for v in row]), h, w, layout)
            planes.append(np.clip(s / float(1 << sh) + c, 0.0, m).reshape(-1))
    return np.concatenate(planes)


# ---- the derived bounds ----------------------------------------------------------------------------------------------------------
# |restatement - exact| per sample: half a level of the one rounding, plus for every coefficient k of the output's row
# |q_k / 2^Q - real_k| times the largest magnitude of its operand.  The chroma interpolation (sixteenths) and the chroma filter (the
# taps' sum is a power of two, divided out by the one shift) are exact in both, so they add nothing: an interpolated or filtered value
# is a convex combination of samples and has their range.  Clamping is 1-Lipschitz.  The figures are computed from the tables, not read
# off a run.
def read_bound(matrix, full_range, bits):
    _, q = int_matrices(matrix, full_range, bits)
    _, real = real_matrices(matrix, full_range, bits)
    e = [abs(Fraction(a, 1 << qbits(bits)) - b) for a, b in zip(q, real)]      # cy, crv, cgu, cgv, cbu
    y0, _, _, c = scales(full_range, bits)
    ymax, cmax = max(maxv(bits) - y0, y0), c                                   # |Y - y0|, |Cx - C| (a sample 0 is -C)
    return float(Fraction(1, 2) + max(e[0] * ymax + e[1] * cmax, e[0] * ymax + (e[2] + e[3]) * cmax, e[0] * ymax + e[4] * cmax))


def write_bound(matrix, full_range, bits):
    rows, _ = int_matrices(matrix, full_range, bits)
    real, _ = real_matrices(matrix, full_range, bits)
    worst = max(sum(abs(Fraction(a, 1 << qbits(bits)) - b) for a, b in zip(r, rr)) for r, rr in zip(rows, real))
    return float(Fraction(1, 2) + worst * maxv(bits))


# ---- the depth reduction ---------------------------------------------------------------------------------------------------------
def reduce_depth(v, bits):
    """v8 = (510 min(v, M) + M) // (2 M): round(255 v / M); a tie would need 2 * 255 v = (2 k + 1) M, even against odd."""
    m = maxv(bits)
    x = np.minimum(np.asarray(v), m).astype(np.int64)
    return ((510 * x + m) // (2 * m)).astype(np.uint8)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def inputs(h, w, layout, bits, seed=0, above=False):
    """[(name, payload)]: all 0, all M, random in 0..M; with `above` random over the whole uint16 range (samples above M)."""
    rng = np.random.default_rng(seed + 1000 * h + w + 17 * bits)
    n, m = frame_samples(h, w, layout), maxv(bits)
    out = [("all0", np.zeros(n, np.uint16)), ("allM", np.full(n, m, np.uint16)), ("random", rng.integers(0, m + 1, n).astype(np.uint16))]
    if above:
        out.append(("above", rng.integers(0, 65536, n).astype(np.uint16)))
    return out


def rgb_inputs(h, w, bits, seed=0, above=False):
    rng = np.random.default_rng(seed + 1000 * h + w + 17 * bits + 7)
    m = maxv(bits)
    out = [("all0", np.zeros((h, w, 3), np.uint16)), ("allM", np.full((h, w, 3), m, np.uint16)),
           ("random", rng.integers(0, m + 1, (h, w, 3)).astype(np.uint16))]
    if above:
        out.append(("above", rng.integers(0, 65536, (h, w, 3)).astype(np.uint16)))
    return out


def y4m_bytes(frames_rgb16, fps, layout, matrix, full_range, bits):
    """A whole deep .y4m stream (bytes) as ffmpeg's yuv4mpegpipe writes it, of uint16 RGB frames converted by rgb_to_yuv."""
    h, w = frames_rgb16[0].shape[:2]
    ss = {"444": "444", "422": "422", "420jpeg": "420"}.get(layout)
    tag = "mono%d" % bits if layout == "mono" else "%sp%d XYSCSS=%sP%d" % (ss, bits, ss, bits)
    head = "YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C%s XCOLORRANGE=%s" % (w, h, fps[0], fps[1], tag, "FULL" if full_range else "LIMITED")
    out = [head.encode() + b"\n"]
    for f in frames_rgb16:
        out += [b"FRAME\n", rgb_to_yuv(f, layout, matrix, full_range, bits).astype("<u2").tobytes()]
    return b"".join(out)
