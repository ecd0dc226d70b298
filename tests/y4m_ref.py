"""YCbCr <-> RGB of a YUV4MPEG2 frame payload, restated from the text of DESIGN.md §2.14 in whole-array numpy int64, and an fp64
"exact" twin (rational chroma interpolation / filtering, real-valued matrix, clamp, no rounding) to bound it.  Does not import the
package: the kernels (csrc/yuv.hip) are held against this file bit for bit, and this file against the exact twin within the derived
bounds READ_BOUND / WRITE_BOUND.

Payload: the Y plane h x w, then Cb, then Cr, each ch x cw (plane_size).  Image: (h, w, 3) uint8 RGB."""
from fractions import Fraction

import numpy as np

LAYOUTS = ("444", "422", "420jpeg", "420mpeg2", "mono")
MATRICES = ("bt601", "bt709")
BITS = 14                                                 # fraction bits of the coefficients
# (horizontal, vertical) sampling of the chroma planes: "full" (not subsampled), "centred" or "cosited" (left-cosited)
AXES = {"444": ("full", "full"), "422": ("cosited", "full"), "420jpeg": ("centred", "centred"), "420mpeg2": ("cosited", "centred"),
        "mono": ("full", "full")}
K = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000))}      # (Kr, Kb)
EXTREMES = (0, 1, 16, 128, 235, 240, 254, 255)
# |restatement - exact| per byte: half a level of the one rounding, plus the coefficients' quantisation (each within 2^-(BITS + 1)
# of its real value) times the largest operands: reading |Y - y0| <= 255 and |C - 128| <= 128 twice; writing three bytes <= 255 (the
# adjusted entry of a row carries the other two's errors: e_r R + e_g G - (e_r + e_g - t) B = e_r (R - B) + e_g (G - B) + t B with
# |t| < 0.05 ulp, which is smaller still).
READ_BOUND = 0.5 + (255 + 128 + 128) * 2.0 ** -(BITS + 1)
WRITE_BOUND = 0.5 + 3 * 255 * 2.0 ** -(BITS + 1)


def plane_size(h, w, layout):
    """(ch, cw) of the chroma planes; (0, 0) for mono."""
    if layout == "mono":
        return 0, 0
    hm, vm = AXES[layout]
    return (h if vm == "full" else (h + 1) // 2), (w if hm == "full" else (w + 1) // 2)


def frame_bytes(h, w, layout):
    ch, cw = plane_size(h, w, layout)
    return h * w + 2 * ch * cw


def scales(full_range):
    """(y0, sy, sc): Y = sy Y' + y0, C = sc C' + 128 for Y' in [0, 255], C' in [-127.5, 127.5]."""
    return (0, Fraction(1), Fraction(1)) if full_range else (16, Fraction(219, 255), Fraction(224, 255))


def real_matrices(matrix, full_range):
    """Exact rationals: (forward 3 x 3 rows Y, Cb, Cr over R, G, B; inverse coefficients cy, crv, cgu, cgv, cbu)."""
    kr, kb = K[matrix]
    kg = 1 - kr - kb
    _, sy, sc = scales(full_range)
    fwd = [[kr * sy, kg * sy, kb * sy],
           [-kr / (2 * (1 - kb)) * sc, -kg / (2 * (1 - kb)) * sc, Fraction(1, 2) * sc],
           [Fraction(1, 2) * sc, -kg / (2 * (1 - kr)) * sc, -kb / (2 * (1 - kr)) * sc]]
    inv = (1 / sy, 2 * (1 - kr) / sc, -2 * (1 - kb) * kb / kg / sc, -2 * (1 - kr) * kr / kg / sc, 2 * (1 - kb) / sc)
    return fwd, inv


def _q(v):
    return int(round(v * (1 << BITS)))                    # Fraction: round half to even of the exact value (no tie occurs)


def int_matrices(matrix, full_range):
    """The integer tables: rows rounded, then the largest entry of each forward row adjusted so that the luma row sums exactly to
    round(sy 2^BITS) and each chroma row to 0."""
    fwd, inv = real_matrices(matrix, full_range)
    _, sy, _ = scales(full_range)
    rows = []
    for row, target in zip(fwd, (_q(sy), 0, 0)):
        r = [_q(v) for v in row]
        big = max(range(3), key=lambda k: abs(r[k]))
        r[big] += target - sum(r)
        rows.append(r)
    return rows, tuple(_q(v) for v in inv)


def split(payload, h, w, layout):
    p = np.asarray(payload, dtype=np.uint8).reshape(-1)
    assert p.size == frame_bytes(h, w, layout), (p.size, frame_bytes(h, w, layout))
    ch, cw = plane_size(h, w, layout)
    y = p[:h * w].reshape(h, w)
    if layout == "mono":
        return y, None, None
    return y, p[h * w:h * w + ch * cw].reshape(ch, cw), p[h * w + ch * cw:].reshape(ch, cw)


# ---- reading ---------------------------------------------------------------------------------------------------------------------
def _read_axis(n, nc, mode):
    """For luma positions 0 .. n - 1 of one axis: (index a, index b, weight of a, weight of b) in quarters, into nc chroma samples."""
    x = np.arange(n)
    if mode == "full":
        return x, x, np.full(n, 4), np.zeros(n, np.int64)
    j = x // 2
    if mode == "centred":                                 # 3/4 own sample, 1/4 the neighbour on the pixel's side
        nb = np.where(x % 2 == 0, j - 1, j + 1)
        return j, np.clip(nb, 0, nc - 1), np.full(n, 3), np.ones(n, np.int64)
    odd = x % 2 == 1                                      # left-cosited: even x sits on sample j, odd x half-way to j + 1
    return j, np.clip(j + 1, 0, nc - 1), np.where(odd, 2, 4), np.where(odd, 2, 0)


def chroma16(plane, h, w, layout, dtype=np.int64):
    """Bilinear chroma at every luma position, edge clamped, in units of 1/16 (exact)."""
    hm, vm = AXES[layout]
    c = plane.astype(dtype)
    ya, yb, wa, wb = _read_axis(h, c.shape[0], vm)
    xa, xb, ua, ub = _read_axis(w, c.shape[1], hm)
    rows = wa[:, None] * c[ya] + wb[:, None] * c[yb]
    return ua[None, :] * rows[:, xa] + ub[None, :] * rows[:, xb]


def yuv_to_rgb(payload, h, w, layout, matrix, full_range):
    y, cb, cr = split(payload, h, w, layout)
    _, (cy, crv, cgu, cgv, cbu) = int_matrices(matrix, full_range)
    y0 = scales(full_range)[0]
    lum = cy * 16 * (y.astype(np.int64) - y0) + (1 << (BITS + 3))
    if layout == "mono":
        u = v = np.zeros((h, w), np.int64)
    else:
        u, v = chroma16(cb, h, w, layout) - 2048, chroma16(cr, h, w, layout) - 2048
    out = np.stack([lum + crv * v, lum + cgu * u + cgv * v, lum + cbu * u], -1) >> (BITS + 4)      # arithmetic shift: floor
    return np.clip(out, 0, 255).astype(np.uint8)


def yuv_to_rgb_exact(payload, h, w, layout, matrix, full_range):
    """fp64, unrounded: (h, w, 3) in [0, 255]."""
    y, cb, cr = split(payload, h, w, layout)
    _, inv = real_matrices(matrix, full_range)
    cy, crv, cgu, cgv, cbu = (float(v) for v in inv)
    lum = cy * (y.astype(np.float64) - scales(full_range)[0])
    if layout == "mono":
        u = v = np.zeros((h, w))
    else:
        u, v = chroma16(cb, h, w, layout, np.float64) / 16.0 - 128.0, chroma16(cr, h, w, layout, np.float64) / 16.0 - 128.0
    return np.clip(np.stack([lum + crv * v, lum + cgu * u + cgv * v, lum + cbu * u], -1), 0.0, 255.0)


# ---- writing ---------------------------------------------------------------------------------------------------------------------
def _write_axis(n, nc, mode):
    """For chroma samples 0 .. nc - 1 of one axis: ([index arrays], [taps], log2 of the taps' sum) over n full-resolution pixels."""
    j = np.arange(nc)
    if mode == "full":
        return [j], [1], 0
    if mode == "centred":                                 # the mean of the 2 covered pixels; an odd edge replicates the last one
        return [2 * j, np.minimum(2 * j + 1, n - 1)], [1, 1], 1
    return [np.maximum(2 * j - 1, 0), 2 * j, np.minimum(2 * j + 1, n - 1)], [1, 2, 1], 2      # [1, 2, 1] / 4 centred on luma column 2j


def _filter(c, h, w, layout):
    """Sum of the taps over a full-resolution plane -> (chroma-size plane, log2 of the divisor)."""
    hm, vm = AXES[layout]
    ch, cw = plane_size(h, w, layout)
    yi, yt, ys = _write_axis(h, ch, vm)
    xi, xt, xs = _write_axis(w, cw, hm)
    rows = sum(t * c[i] for i, t in zip(yi, yt))
    return sum(t * rows[:, i] for i, t in zip(xi, xt)), ys + xs


def rgb_to_yuv(rgb, layout, matrix, full_range):
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    h, w = rgb.shape[:2]
    (ky, ku, kv), _ = int_matrices(matrix, full_range)
    p = rgb.astype(np.int64)
    y = np.clip(((p @ np.array(ky) + (1 << (BITS - 1))) >> BITS) + scales(full_range)[0], 0, 255).astype(np.uint8)
    planes = [y.reshape(-1)]
    if layout != "mono":
        for k in (ku, kv):
            s, sh = _filter(p @ np.array(k), h, w, layout)            # unrounded per pixel, filtered, rounded once
            planes.append(np.clip(((s + (1 << (BITS + sh - 1))) >> (BITS + sh)) + 128, 0, 255).astype(np.uint8).reshape(-1))
    return np.concatenate(planes)


def rgb_to_yuv_exact(rgb, layout, matrix, full_range):
    """fp64, unrounded: the payload's values in [0, 255], planes concatenated as in the payload."""
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    fwd, _ = real_matrices(matrix, full_range)
    p = rgb.astype(np.float64)
    planes = [np.clip(p @ np.array([float(v) for v in fwd[0]]) + scales(full_range)[0], 0.0, 255.0).reshape(-1)]
    if layout != "mono":
        for row in fwd[1:]:
            s, sh = _filter(p @ np.array([float(v) for v in row]), h, w, layout)
            planes.append(np.clip(s / float(1 << sh) + 128.0, 0.0, 255.0).reshape(-1))
    return np.concatenate(planes)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def inputs(h, w, layout, seed=0):
    """[(name, payload)]: random planes, planes drawn from EXTREMES, and the constant planes of the extremes' corners."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    n = frame_bytes(h, w, layout)
    out = [("random", rng.integers(0, 256, n, dtype=np.uint8)), ("extremes", rng.choice(np.array(EXTREMES, np.uint8), n))]
    for v in (0, 255):
        out.append(("all%d" % v, np.full(n, v, np.uint8)))
    return out


def rgb_inputs(h, w, seed=0):
    rng = np.random.default_rng(seed + 1000 * h + w + 7)
    return [("random", rng.integers(0, 256, (h, w, 3), dtype=np.uint8)), ("extremes", rng.choice(np.array(EXTREMES, np.uint8), (h, w, 3))),
            ("all0", np.zeros((h, w, 3), np.uint8)), ("all255", np.full((h, w, 3), 255, np.uint8))]


# ---- the container, for tests that must not import the package -------------------------------------------------------------------
def y4m_bytes(frames_rgb, fps, layout, matrix, full_range, range_tag=True):
    """A whole .y4m stream (bytes) of RGB frames converted by rgb_to_yuv."""
    h, w = frames_rgb[0].shape[:2]
    tag = {"444": "444", "422": "422", "420jpeg": "420jpeg", "420mpeg2": "420mpeg2", "mono": "mono"}[layout]
    head = "YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C%s" % (w, h, fps[0], fps[1], tag)
    if range_tag:
        head += " XCOLORRANGE=%s" % ("FULL" if full_range else "LIMITED")
    out = [head.encode() + b"\n"]
    for f in frames_rgb:
        out += [b"FRAME\n", rgb_to_yuv(f, layout, matrix, full_range).tobytes()]
    return b"".join(out)
