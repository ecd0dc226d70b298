"""Test helper (not a test module): numpy restatement of cv2.resize(src, (dw, dh), interpolation=cv2.INTER_AREA) for uint8 images when
shrinking, as OpenCV 4.x imgproc/resize.cpp computes it (resizeAreaFast_, computeResizeAreaTab, ResizeArea_Invoker), and an independent
fp64 exact area average to bound it.  OpenCV's own bytes are pinned only once tests/golden/resize_area_cv2.npz exists
(tools/make_golden_resize_area.py); until then the kernel is held against this restatement bit for bit and against the exact average.

The restatement keeps OpenCV's roundings: tables built in fp64 with float weights, fp32 accumulation in table order, round half to even."""
import numpy as np

# (sh, sw, dh, dw): the shapes of the kernel tests, general path first (tests/test_gpu_resize_area.py, tools/make_golden_resize_area.py)
SHAPES = [(17, 23, 8, 11), (9, 10, 8, 8), (16, 40, 15, 39), (200, 288, 133, 192), (40, 30, 10, 20), (20, 30, 10, 15), (21, 30, 7, 10), (20, 30, 10, 10)]
GENERAL = SHAPES[:5]
EPS = float(np.finfo(np.float64).eps)      # DBL_EPSILON


def scales(ssize, dsize):
    scale = 1.0 / (float(dsize) / float(ssize))
    return scale, int(np.rint(scale))


def is_fast(sh, sw, dh, dw):
    (fx, ix), (fy, iy) = scales(sw, dw), scales(sh, dh)
    return abs(fx - ix) < EPS and abs(fy - iy) < EPS


def area_table(ssize, dsize):
    """[(d, s, float32 weight)] in OpenCV's order (computeResizeAreaTab)."""
    scale, _ = scales(ssize, dsize)
    tab = []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, ssize - f1)
        s1 = int(np.ceil(f1))
        s2 = min(int(np.floor(f2)), ssize - 1)
        s1 = min(s1, s2)
        if s1 - f1 > 1e-3:
            tab.append((d, s1 - 1, np.float32((s1 - f1) / cell)))
        for s in range(s1, s2):
            tab.append((d, s, np.float32(1.0 / cell)))
        if f2 - s2 > 1e-3:
            tab.append((d, s2, np.float32(min(min(f2 - s2, 1.0), cell) / cell)))
    return tab


def _saturate(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)      # np.rint: half to even, like cvRound


def resize_area(src, dh, dw):
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3
    sh, sw, ch = src.shape
    assert 1 <= dh <= sh and 1 <= dw <= sw and (dh, dw) != (sh, sw)
    if is_fast(sh, sw, dh, dw):
        ix, iy = scales(sw, dw)[1], scales(sh, dh)[1]
        block = src.reshape(dh, iy, dw, ix, ch).astype(np.int64).sum(axis=(1, 3))
        if ix == 2 and iy == 2 and ch != 2:
            return ((block + 2) >> 2).astype(np.uint8)
        inv = np.float32(np.float32(1.0) / np.float32(ix * iy))
        return _saturate(block.astype(np.float32) * inv)
    xtab, ytab = area_table(sw, dw), area_table(sh, dh)
    S = src.astype(np.float32)
    rows = np.zeros((sh, dw, ch), np.float32)      # the row buffer of every source row: it does not depend on the y entry
    for dx, sx, alpha in xtab:
        rows[:, dx] = rows[:, dx] + S[:, sx] * alpha
    out = np.zeros((dh, dw, ch), np.uint8)
    acc, prev = None, -1
    for dy, sy, beta in ytab:
        if dy != prev:
            if prev >= 0:
                out[prev] = _saturate(acc)
            acc, prev = beta * rows[sy], dy
        else:
            acc = acc + beta * rows[sy]
    out[prev] = _saturate(acc)
    assert rows.dtype == np.float32 and acc.dtype == np.float32
    return out


def _coverage(ssize, dsize):
    """(dsize, ssize) fp64 weights max(0, min(b, j + 1) - max(a, j)) of the cell [a, b) = [d * ssize / dsize, (d + 1) * ssize / dsize),
    normalised per row."""
    d = np.arange(dsize, dtype=np.float64)[:, None]
    j = np.arange(ssize, dtype=np.float64)[None, :]
    a, b = d * ssize / dsize, (d + 1) * ssize / dsize
    w = np.maximum(0.0, np.minimum(b, j + 1) - np.maximum(a, j))
    return w / w.sum(axis=1, keepdims=True)


def exact_area(src, dh, dw):
    """The exact area average in fp64 (no rounding to uint8): (dh, dw, ch) float64."""
    src = np.asarray(src, np.float64)
    wy, wx = _coverage(src.shape[0], dh), _coverage(src.shape[1], dw)
    rows = np.tensordot(wy, src, axes=(1, 0))                              # (dh, sw, ch)
    return np.tensordot(wx, rows, axes=(1, 1)).transpose(1, 0, 2)          # (dw, dh, ch) -> (dh, dw, ch)


def inputs(sh, sw, ch=3, seed=0):
    """The test images of one source shape: seeded random uint8, all 0, all 255."""
    rng = np.random.default_rng(1000 * sh + sw + 17 * ch + seed)
    return [rng.integers(0, 256, (sh, sw, ch), dtype=np.uint8), np.zeros((sh, sw, ch), np.uint8), np.full((sh, sw, ch), 255, np.uint8)]
