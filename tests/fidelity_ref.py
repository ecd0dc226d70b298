"""numpy restatement of the fidelity metrics (csrc/fidelity.hip, include/atlasfit.h af_fidelity), its fp64 twin (the skimage algorithm
stated with scipy.ndimage.uniform_filter) and the restatement of the flicker synthesiser.  Does not import the product.

The restatement performs the kernel's operations one by one: exact int64 window sums from a summed-area table, then the fp64 steps in
the kernel's order, each a single correctly rounded numpy operation, so a GPU result may be compared bit for bit."""
import math
import os
import re

import numpy as np

import guided_transfer_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K1, K2, L = 0.01, 0.03, 255.0


def tile():
    """(tile_x pixels, tile_y rows) of the SSIM kernel and the bytes of a frame one workgroup of the SSE kernel reads, from the kernel's header."""
    text = open(os.path.join(ROOT, "all-in-one-deflicker_amd", "csrc", "fidelity.h")).read()
    return tuple(int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1)) for name in ("AF_FID_TILE_X", "AF_FID_TILE_Y", "AF_FID_SSE_BYTES"))


def constants(win):
    n = win * win
    k1, k2 = K1 * L, K2 * L
    return (k1 * k1) * float(n * n), (k2 * k2) * float(n * (n - 1))


def box_sums(v, win):
    """Exact sums over every win x win window that lies inside the frame: int64 (h - win + 1, w - win + 1, ...), by summed-area table."""
    v = np.asarray(v, np.int64)
    c = np.cumsum(np.cumsum(v, 0), 1)
    c = np.pad(c, [(1, 0), (1, 0)] + [(0, 0)] * (v.ndim - 2))
    return c[win:, win:] - c[:-win, win:] - c[win:, :-win] + c[:-win, :-win]


def sse(a, b):
    """uint64 (..., 3): the integer sum of (a - b)^2 over each frame and channel."""
    d = np.asarray(a, np.int64) - np.asarray(b, np.int64)
    return (d * d).sum(axis=(-3, -2)).astype(np.uint64)


def ssim_map(a, b, win):
    """float64 (h - win + 1, w - win + 1, 3) of one frame pair: the kernel's S."""
    x, y = np.asarray(a, np.int64), np.asarray(b, np.int64)
    n = np.int64(win * win)
    c1, c2 = constants(win)
    sx, sy, sxx, syy, sxy = box_sums(x, win), box_sums(y, win), box_sums(x * x, win), box_sums(y * y, win), box_sums(x * y, win)
    a1 = (2 * sx * sy).astype(np.float64) + c1
    b1 = (sx * sx + sy * sy).astype(np.float64) + c1
    a2 = (2 * (n * sxy - sx * sy)).astype(np.float64) + c2
    b2 = ((n * sxx - sx * sx) + (n * syy - sy * sy)).astype(np.float64) + c2
    return (a1 * a2) / (b1 * b2)


def ssim_mean(smap):
    """(3,) float64: math.fsum of a frame's map over the windows, divided by their count."""
    count = smap.shape[0] * smap.shape[1]
    return np.array([math.fsum(smap[:, :, c].ravel().tolist()) / count for c in range(3)])


def ssim_twin(a, b, win):
    """The skimage algorithm (structural_similarity, uint8 defaults: uniform filter, sample covariance, K1, K2, data range 255) in fp64
    with scipy.ndimage.uniform_filter, cropped by (win - 1) / 2 to the windows that lie inside the frame."""
    from scipy.ndimage import uniform_filter
    out = []
    for c in range(3):
        x, y = np.asarray(a, np.float64)[:, :, c], np.asarray(b, np.float64)[:, :, c]
        npix = win * win
        cov_norm = npix / (npix - 1.0)
        ux, uy = uniform_filter(x, size=win), uniform_filter(y, size=win)
        uxx, uyy, uxy = uniform_filter(x * x, size=win), uniform_filter(y * y, size=win), uniform_filter(x * y, size=win)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        c1, c2 = (K1 * L) ** 2, (K2 * L) ** 2
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        pad = (win - 1) // 2
        out.append(s[pad:s.shape[0] - pad, pad:s.shape[1] - pad])
    return np.stack(out, -1)


def psnr(sse3, pixels):
    total = int(sum(int(v) for v in sse3))
    return math.inf if total == 0 else 10.0 * math.log10(255.0 ** 2 * 3 * pixels / total)


# ---- the flicker synthesiser ------------------------------------------------------------------------------------------------------
def flicker_planes(n, kind, strength, grid, seed):
    """The documented order of draws: per frame a ~ U(-s, s), then b ~ U(-64 s, 64 s), each (gh, gw, 3), 1 x 1 for `global`; float32."""
    gh, gw = (1, 1) if kind == "global" else grid
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        a = rng.uniform(-strength, strength, (gh, gw, 3)).astype(np.float32)
        b = rng.uniform(-64.0 * strength, 64.0 * strength, (gh, gw, 3)).astype(np.float32)
        out.append((a, b))
    return out


def flicker(frames, kind="global", strength=0.1, grid=(4, 4), seed=0):
    planes = flicker_planes(len(frames), kind, strength, grid, seed)
    return np.stack([G.apply(f, a, b) for f, (a, b) in zip(frames, planes)]), planes


# ---- the tests' frames ------------------------------------------------------------------------------------------------------------
def make_pair(h, w, seed, kind="structured"):
    """Two (h, w, 3) uint8 frames: `random` bytes, or a picture with structure and a flickered, noisy copy of it."""
    rng = np.random.RandomState(seed)
    if kind == "random":
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8), rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(x / 9.0 + c) * np.cos(y / 7.0 - c) for c in range(3)], -1)
    a = np.clip(base + rng.randint(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)
    gain = 1.0 + 0.15 * np.sin(x / 23.0)[:, :, None]
    b = np.clip(np.rint(a * gain + 12.0 * np.cos(y / 17.0)[:, :, None] + rng.randint(-3, 4, a.shape)), 0, 255).astype(np.uint8)
    return a, b
