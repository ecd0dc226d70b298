"""Fixture of the warping error (include/atlasfit.h: af_warp_error_pair / af_warp_error), computed by the REFERENCE's own
flow_warping and detect_occlusion (src/models/utils.py:504-572) on the CPU.

src/models/utils.py is imported read-only with a stub module for cv2 (none of the functions used here needs it).  detect_occlusion
moves its tensors with .cuda(); that is made a no-op for the duration of the call.  Geometry 0 ("reference") calls the functions as
they are, so grid_sample runs with today's default align_corners=False; geometry 1 ("exact") runs them with grid_sample partially
applied with align_corners=True.

    AF_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_warp_error.py
        -> tests/golden/warp_error.npz       (byte-identical on every run)

Data, per shape s (s0: 37x53, 5 frames; s1: 18x26, 5 frames), all fp32 unless noted:
  s{s}_frames (F, H, W, 3)      a smooth pattern moving with the flow, times a per-frame, per-channel gain (the flicker)
  s{s}_fw, s{s}_bw (F-1, H, W, 2) fw[t] = fw_t (t -> t+1): a rotation about the centre plus a translation, with a block moving on
                                its own; bw[t] = bw_{t+1} (t+1 -> t): the inverse motion, perturbed.  Some vectors leave the image.
  s{s}_g{g}_warped (F-1, H, W, 3) flow_warping(I_{t+1}, fw_t); _warped_e64 = |fp32 - fp64 twin| (float64 tensors through flow_warping)
  s{s}_g{g}_noc (F-1, H, W) uint8 1 - detect_occlusion(bw_{t+1}, fw_t)
  s{s}_g{g}_m1, _m2 (F-1, H, W) lhs - rhs of the two occlusion inequalities, from the fp64 twin (> 0: occluded)
  s{s}_g{g}_err (F-1,) float64  E_t = sum noc (warped - I_t)^2 / (3 sum noc), the reference's fp32 warped and mask, summed in fp64
  s{s}_g{g}_inband (2,) int64   pixels whose |m1| < BAND1 or |m2| < BAND2 (where the fp32 masks may legitimately differ)
  band                          (BAND1, BAND2)
"""
import functools
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch

REF = os.environ.get("AF_REFERENCE")
if not REF or not os.path.isfile(os.path.join(REF, "src", "models", "utils.py")):
    raise SystemExit("set AF_REFERENCE to a checkout of the reference repository (the directory holding src/models/utils.py)")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
_cv2 = types.ModuleType("cv2")
_cv2.__getattr__ = lambda name: 0       # module-level constants such as cv2.INTER_LINEAR in default arguments
sys.modules.setdefault("cv2", _cv2)
_spec = importlib.util.spec_from_file_location("ref_models_utils", os.path.join(REF, "src", "models", "utils.py"))
U = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(U)

OUT = os.path.join(ROOT, "tests", "golden", "warp_error.npz")
SHAPES = ((37, 53, 5), (18, 26, 5))
SEED = 20261016
BAND1, BAND2 = 1e-3, 1e-5       # fp32 rounding of either side of the two inequalities at these flow sizes is below 1e-5


def _pattern(x, y, t, H, W):
    """A smooth test image (3 channels) sampled at (x, y), fp64."""
    return np.stack([0.5 + 0.25 * np.sin(2 * np.pi * (x / W * (2 + c) + y / H * (1 + c)) + 0.7 * c + 0.3 * t)
                     + 0.15 * np.cos(2 * np.pi * (x * y) / (W * H) * 3 + c) for c in range(3)], axis=-1)


def make_sequence(H, W, F, rng):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    gain = 1.0 + 0.15 * rng.standard_normal((F, 3))
    frames, fw, bw = [], [], []
    for t in range(F):
        frames.append(_pattern(xx, yy, t, H, W) * gain[t])
    for t in range(F - 1):
        th = 0.03 + 0.01 * t
        tx, ty = 1.5 + 0.5 * t, -1.0 + 0.25 * t
        c, s = np.cos(th), np.sin(th)
        X, Y = xx - cx, yy - cy
        fx = c * X - s * Y + cx + tx - xx
        fy = s * X + c * Y + cy + ty - yy
        # the inverse of the rigid motion, evaluated on frame t+1's grid
        Xi, Yi = xx - cx - tx, yy - cy - ty
        bx = c * Xi + s * Yi + cx - xx
        by = -s * Xi + c * Yi + cy - yy
        # an independently moving block (frame t: rows/cols b0..b1, moving by (vx, vy)); a few vectors point far out of the image
        y0, x0 = H // 4 + t, W // 3 + t
        y1, x1 = y0 + H // 3, x0 + W // 4
        vx, vy = -4.0 + t, 3.0
        fx[y0:y1, x0:x1], fy[y0:y1, x0:x1] = vx, vy
        bx[y0 + 3:y1 + 3, x0 + t - 4:x1 + t - 4], by[y0 + 3:y1 + 3, x0 + t - 4:x1 + t - 4] = -vx, -vy
        fx[0, :3], fy[-1, -3:] = -2.0 * W, 3.0 * H
        bx += 0.05 * rng.standard_normal((H, W))
        by += 0.05 * rng.standard_normal((H, W))
        fw.append(np.stack([fx, fy], -1))
        bw.append(np.stack([bx, by], -1))
    return (np.stack(frames).astype(np.float32), np.stack(fw).astype(np.float32), np.stack(bw).astype(np.float32))


class _Geometry:
    """geometry 1: grid_sample with align_corners=True while the reference function runs; 0: as it is.  Also makes .cuda() a no-op."""

    def __init__(self, g):
        self.g = g

    def __enter__(self):
        self.gs, self.cuda = torch.nn.functional.grid_sample, torch.Tensor.cuda
        if self.g == 1:
            torch.nn.functional.grid_sample = functools.partial(self.gs, align_corners=True)
        torch.Tensor.cuda = lambda self_, *a, **k: self_
        return self

    def __exit__(self, *exc):
        torch.nn.functional.grid_sample, torch.Tensor.cuda = self.gs, self.cuda


def _warp(img_hwc, flow_hwc, dtype):
    x = torch.from_numpy(np.ascontiguousarray(img_hwc.transpose(2, 0, 1)[None]).astype(dtype))
    f = torch.from_numpy(np.ascontiguousarray(flow_hwc.transpose(2, 0, 1)[None]).astype(dtype))
    return U.flow_warping(x, f)[0].numpy().transpose(1, 2, 0)


def margins64(A, B, g):
    """lhs - rhs of both occlusion tests of detect_occlusion(A, B) in fp64 (A_w from the fp64 twin of flow_warping)."""
    with _Geometry(g):
        Aw = _warp(A.astype(np.float64), B.astype(np.float64), np.float64)
    B = B.astype(np.float64)
    s = Aw + B
    m1 = (s[..., 0] ** 2 + s[..., 1] ** 2) - (0.01 * ((Aw ** 2).sum(-1) + (B ** 2).sum(-1)) + 0.5)
    dxu, dxv, dyu, dyv = U.compute_flow_gradients(B)
    m2 = (dxu ** 2 + dxv ** 2 + dyu ** 2 + dyv ** 2) - (0.01 * (B ** 2).sum(-1) + 0.002)
    return m1, m2


def main():
    warnings.filterwarnings("ignore")
    torch.set_num_threads(1)
    rng = np.random.default_rng(SEED)
    out = {"band": np.array([BAND1, BAND2], np.float64)}
    for si, (H, W, F) in enumerate(SHAPES):
        frames, fw, bw = make_sequence(H, W, F, rng)
        out["s%d_frames" % si], out["s%d_fw" % si], out["s%d_bw" % si] = frames, fw, bw
        for g in (0, 1):
            warped, e64, noc, m1s, m2s, err = [], [], [], [], [], []
            inband = np.zeros(2, np.int64)
            for t in range(F - 1):
                with _Geometry(g):
                    w32 = _warp(frames[t + 1], fw[t], np.float32)
                    w64 = _warp(frames[t + 1].astype(np.float64), fw[t].astype(np.float64), np.float64)
                    occ = U.detect_occlusion(bw[t], fw[t])           # (fw_flow = A = bw_{t+1}, bw_flow = B = fw_t)
                n = (1 - occ).astype(np.uint8)
                m1, m2 = margins64(bw[t], fw[t], g)
                inband += [int((np.abs(m1) < BAND1).sum()), int((np.abs(m2) < BAND2).sum())]
                d = w32.astype(np.float64) - frames[t].astype(np.float64)
                N = 3.0 * n.sum() if n.sum() > 0 else 3.0 * H * W
                err.append(float((n[..., None] * d * d).sum() / N))
                warped.append(w32); e64.append(np.abs(w32.astype(np.float64) - w64).astype(np.float32)); noc.append(n)
                m1s.append(m1); m2s.append(m2)
            k = "s%d_g%d_" % (si, g)
            out[k + "warped"], out[k + "warped_e64"], out[k + "noc"] = np.stack(warped), np.stack(e64), np.stack(noc)
            out[k + "m1"], out[k + "m2"] = np.stack(m1s).astype(np.float32), np.stack(m2s).astype(np.float32)
            out[k + "err"], out[k + "inband"] = np.array(err, np.float64), inband
            print("shape %dx%d geometry %d: E %s, noc %.3f, in band %s" % (H, W, g, np.round(err, 6), np.stack(noc).mean(), inband))
    # np.savez_compressed writes zip entries with the current time: write a fixed date for byte-identical reruns
    import zipfile
    tmp = OUT + ".tmp"
    with zipfile.ZipFile(tmp, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name in sorted(out):
            import io
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(out[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    os.replace(tmp, OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
