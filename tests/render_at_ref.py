"""Test helper (not a test module): numpy restatement of the coordinates af_render_frame_at evaluates the nets at, and the oracle's
models (oracle/atlas_oracle.py) evaluated at them.

Geometry (include/atlasfit.h): an (oh, ow) grid over the stage-1 lattice (resy, resx) by OpenCV's pixel-centre rule, source position
(X + 0.5) * (resx / ow) - 0.5 in fp64, clamped to [0, resx - 1] as cv2.resize clamps its border taps, rounded to fp32, then the render's
fp32 normalisation x = sx / half_main - 1 with half_main = max(resx, resy) / 2 of the lattice.  No fused multiply-add anywhere."""
import numpy as np


def source_positions(src, dst):
    """fp64 lattice positions of the dst pixel centres along one axis, clamped: [dst]."""
    d = np.arange(int(dst), dtype=np.float64)
    s = (d + 0.5) * (float(src) / float(dst)) - 0.5
    return np.clip(s, 0.0, float(src - 1))


def frame_time(f, nframes):
    return f / (nframes / 2.0) - 1.0       # Python floats, as evaluate.py:656 computes it


def coords(resx, resy, oh, ow, f, nframes):
    """(oh * ow, 4) float32 rows (x, y, t, 0) in row-major pixel order: k_frame_coords_at's rows bit for bit."""
    half = np.float32(max(resx, resy) / 2.0)
    x = source_positions(resx, ow).astype(np.float32) / half - np.float32(1)
    y = source_positions(resy, oh).astype(np.float32) / half - np.float32(1)
    rows = np.zeros((oh, ow, 4), np.float32)
    rows[:, :, 0] = x[None, :]
    rows[:, :, 1] = y[:, None]
    rows[:, :, 2] = np.float32(frame_time(f, nframes))
    return rows.reshape(-1, 4)


def coords64(resx, resy, oh, ow, f, nframes):
    """The same positions without any fp32 rounding: (oh * ow, 3) float64 rows for an fp64 twin of the models."""
    half = max(resx, resy) / 2.0
    rows = np.zeros((oh, ow, 3), np.float64)
    rows[:, :, 0] = (source_positions(resx, ow) / half - 1.0)[None, :]
    rows[:, :, 1] = (source_positions(resy, oh) / half - 1.0)[:, None]
    rows[:, :, 2] = frame_time(f, nframes)
    return rows.reshape(-1, 3)


def render(models, xyt, oh, ow):
    """The oracle's render (atlas_oracle.render_frame / render_frame_seg) at the rows `xyt` (n, 3): (oh, ow, 3) numpy in the models'
    dtype.  models: (mapping, atlas), or (mapping1, mapping2, atlas, alpha) for the fg/bg path."""
    import torch
    from oracle import atlas_oracle as O
    dt = next(models[0].parameters()).dtype
    x = torch.from_numpy(np.ascontiguousarray(xyt[:, :3])).to(dt)
    with torch.no_grad():
        if len(models) == 2:
            mapping, atlas = models
            out = (atlas(mapping(x) * 0.5 + 0.5) + 1) * 0.5
        else:
            m1, m2, atlas, alpha = models
            r1 = (atlas(m1(x) * 0.5 + 0.5) + 1) * 0.5
            r2 = (atlas(m2(x) * 0.5 - 0.5) + 1) * 0.5
            a = O.alpha_of(alpha, x)
            out = r1 * a + r2 * (1.0 - a)
    return out.numpy().reshape(oh, ow, 3)


def fp64_twin(models):
    import copy
    twins = [copy.deepcopy(m).double() for m in models]
    for m in twins:
        if m.use_positional:
            m.b = m.b.double()
    return twins


def render_pair(models, twins, resx, resy, oh, ow, f, nframes):
    """(fp32 oracle render on the fp32 rows, fp64 twin's render on the unrounded positions)."""
    want = render(models, coords(resx, resy, oh, ow, f, nframes), oh, ow)
    want64 = render(twins, coords64(resx, resy, oh, ow, f, nframes), oh, ow)
    return want, want64
