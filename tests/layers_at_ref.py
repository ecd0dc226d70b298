"""Test helper (not a test module): the oracle's models (oracle/atlas_oracle.py) evaluated net by net at the coordinates
af_render_layers_at evaluates them at (tests/render_at_ref.py), and a numpy restatement of the reference's get_colors for the edits.

layers(models, rows, oh, ow): uv1 / uv2 the raw mapping outputs, alpha = O.alpha_of of the alpha net, rgb1 / rgb2 = (atlas + 1) / 2 at
uv1 * 0.5 + 0.5 / uv2 * 0.5 - 0.5; a single-atlas pair (mapping, atlas) has uv1 and rgb1 only."""
import numpy as np

import render_at_ref as R


def layers(models, xyt, oh, ow):
    """{name: numpy array (oh, ow[, 2 | 3]) in the models' dtype} at the rows `xyt` (n, >= 3)."""
    import torch
    from oracle import atlas_oracle as O
    dt = next(models[0].parameters()).dtype
    x = torch.from_numpy(np.ascontiguousarray(xyt[:, :3])).to(dt)
    out = {}
    with torch.no_grad():
        if len(models) == 2:
            mapping, atlas = models
            uv1 = mapping(x)
            out["uv1"], out["rgb1"] = uv1, (atlas(uv1 * 0.5 + 0.5) + 1) * 0.5
        else:
            m1, m2, atlas, alpha = models
            uv1, uv2 = m1(x), m2(x)
            out["uv1"], out["uv2"] = uv1, uv2
            out["alpha"] = O.alpha_of(alpha, x)
            out["rgb1"], out["rgb2"] = (atlas(uv1 * 0.5 + 0.5) + 1) * 0.5, (atlas(uv2 * 0.5 - 0.5) + 1) * 0.5
    return {k: (v.numpy().reshape(oh, ow) if k == "alpha" else v.numpy().reshape(oh, ow, -1)) for k, v in out.items()}


def layers_pair(models, twins, resx, resy, oh, ow, f, nframes):
    """(the fp32 oracle's layers on the fp32 rows, its fp64 twin's on the unrounded positions)."""
    want = layers(models, R.coords(resx, resy, oh, ow, f, nframes), oh, ow)
    want64 = layers(twins, R.coords64(resx, resy, oh, ow, f, nframes), oh, ow)
    return want, want64


def get_colors(res, minx, miny, edge, px_uv, py_uv, image):
    """evaluate.py:24-84 (get_colors + bilinear_interpolate_numpy) restated on numpy inputs, as tests/test_gpu_atlas_outputs.py restates it:
    (pixels of the relevant points in fp64, their texel x, their texel y, the relevant mask)."""
    minx, miny = np.float32(minx), np.float32(miny)
    pixel_size = np.float32(np.float32(res) / (np.float32(minx + np.float32(edge)) - minx))
    x = ((px_uv - minx) * pixel_size).astype(np.float32)
    y = ((py_uv - miny) * pixel_size).astype(np.float32)
    x0 = np.floor(x).astype(int); x1 = x0 + 1; y0 = np.floor(y).astype(int); y1 = y0 + 1
    x0 = np.clip(x0, 0, res - 1); x1 = np.clip(x1, 0, res - 1); y0 = np.clip(y0, 0, res - 1); y1 = np.clip(y1, 0, res - 1)
    wa, wb = (x1 - x) * (y1 - y), (x1 - x) * (y - y0)
    wc, wd = (x - x0) * (y1 - y), (x - x0) * (y - y0)
    pix = (image[y0, x0].T * wa).T + (image[y1, x0].T * wb).T + (image[y0, x1].T * wc).T + (image[y1, x1].T * wd).T
    rel = (np.ceil(y) >= 0) & (np.floor(y) >= 0) & (np.ceil(x) >= 0) & (np.floor(x) >= 0)
    rel &= (np.ceil(y) < res) & (np.floor(y) < res) & (np.ceil(x) < res) & (np.floor(x) < res)
    return pix[rel], x[rel], y[rel], rel


def edit_of(res, win_fg, win_bg, t1, t2, uv1, uv2, alpha):
    """The edits and texel usage of one frame from uv1, uv2 (n, 2) and alpha (n,) (evaluate.py:373-438, as test_edit_and_masks restates
    it): (edit, edit_fg, edit_bg) (n, 3) fp64, the shares of relevant pixels (fg, bg), and a function adding this frame's usage to the
    masks (m1, m2): np.maximum.at of alpha (fg) and 1 (bg) over the four floor / ceil texels."""
    h = np.float32(0.5)
    p1, x1, y1, r1 = get_colors(res, win_fg[0], win_fg[1], win_fg[2], uv1[:, 0] * h + h, uv1[:, 1] * h + h, t1)
    p2, x2, y2, r2 = get_colors(res, win_bg[0], win_bg[1], win_bg[2], uv2[:, 0] * h - h, uv2[:, 1] * h - h, t2)
    e1, e2, e = (np.zeros((alpha.size, 3)) for _ in range(3))
    e1[r1] = p1 * alpha[r1][:, None]
    e2[r2] = p2
    e[r1] += p1 * alpha[r1][:, None]
    e[r2] += p2 * (np.float32(1) - alpha)[r2][:, None]

    def add_usage(m1, m2):
        for yy, xx in ((np.ceil(y1), np.ceil(x1)), (np.floor(y1), np.floor(x1)), (np.floor(y1), np.ceil(x1)), (np.ceil(y1), np.floor(x1))):
            np.maximum.at(m1, (yy.astype(int), xx.astype(int)), alpha[r1])
        for yy, xx in ((np.ceil(y2), np.ceil(x2)), (np.floor(y2), np.floor(x2)), (np.floor(y2), np.ceil(x2)), (np.ceil(y2), np.floor(x2))):
            m2[yy.astype(int), xx.astype(int)] = 1
    return (e, e1, e2), (int(r1.sum()), int(r2.sum())), add_usage
