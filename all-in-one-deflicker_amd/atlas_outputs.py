"""Layer outputs of a two-layer stage-1 evaluation (reference: src/models/stage_1/evaluate.py:235-257,361-369,485-560), written as
PNG sequences instead of the reference's mp4s (no encoder dependency).  The GPU work is libatlasfit.so's (af_render_layers,
af_mapping_area, af_render_atlas_texture, af_render_edit; af_render_layers_at for sequences at another size); this module is numpy / PIL only.

    <eval_dir>/texture_orig1.png, texture_orig2.png    (masks * texture * 255).astype(uint8), 1000^2 (:485-496)
    <eval_dir>/alpha/%05d.png                           (alpha * 255).astype(uint8)
    <eval_dir>/uv_1/%05d.png, uv_2/%05d.png             normalize_uv_images (:193-200), then * 255 -> uint8
"""
import os

import numpy as np

TEXTURE_RES = 1000
FG_WINDOW = (np.float32(0), np.float32(0), np.float32(1))      # evaluate.py:233-235: the fg texture always covers [0, 1]^2


def linspace_f32(start, end, n):
    """torch.linspace(start, end, n) in fp32 as torch's CPU kernel rounds it, restated in numpy (the device grid of
    af_render_atlas_texture uses the same formula): step = (end - start) / (n - 1); below n // 2 fma(step, i, start), from there
    fma(-step, n - 1 - i, end).  The fp32 product step * i is exact in fp64, so the fp64 sum rounded once to fp32 is the fma."""
    s, e = np.float32(start), np.float32(end)
    if n == 1:
        return np.array([s], np.float32)
    step = np.float32((e - s) / np.float32(n - 1))
    i = np.arange(n)
    lo = np.float64(s) + np.float64(step) * i
    hi = np.float64(e) - np.float64(step) * (n - 1 - i)
    return np.where(i < n // 2, lo, hi).astype(np.float32)


def normalize_uv(uv, shift, edge, minx, miny):
    """normalize_uv_images (evaluate.py:193-200) of one frame: (H, W, 2) raw uv -> (H, W, 3) in [0, 1], channel 2 zero, fp64."""
    out = np.zeros(uv.shape[:2] + (3,), np.float64)
    out[:, :, 0] = ((uv[:, :, 0].astype(np.float64) * 0.5 + shift) - np.float64(minx)) / np.float64(edge)
    out[:, :, 1] = ((uv[:, :, 1].astype(np.float64) * 0.5 + shift) - np.float64(miny)) / np.float64(edge)
    return np.clip(out, 0.0, 1.0)


def to_u8(x):
    """The reference's truncating cast: (x * 255).astype(uint8), in fp64."""
    return (np.asarray(x, np.float64) * 255).astype(np.uint8)


def masked_texture(masks, texture):
    """evaluate.py:485-496: (masks[:, :, None] * texture * 255).astype(uint8)."""
    return to_u8(masks.astype(np.float64)[:, :, None] * texture.astype(np.float64))


def parse_size(text, full=None):
    """A --size value: "stage1" -> None (the lattice), "full" -> `full` (the decoded frames' (h, w)), "HxW" -> (H, W), each 1..16384."""
    if text == "stage1":
        return None
    if text == "full":
        if full is None:
            raise ValueError("size 'full' needs the decoded frames' size")
        return int(full[0]), int(full[1])
    parts = str(text).lower().split("x")
    if len(parts) != 2 or not all(p.isdigit() for p in parts):
        raise ValueError("size must be stage1, full or HxW, got %r" % (text,))
    h, w = int(parts[0]), int(parts[1])
    if not (1 <= h <= 16384 and 1 <= w <= 16384):
        raise ValueError("size %r: H and W must be 1..16384" % (text,))
    return h, w


def write_atlas_outputs(af, eval_dir, res=TEXTURE_RES, size=None):
    """All layer outputs of a two_layer AtlasFit into eval_dir (see the module docstring).  size = (h, w): the alpha/, uv_1/, uv_2/
    sequences at that size, the nets evaluated at its pixels (render_layers_at; alpha/ is the library's own bytes); the textures and
    their masks are the same either way.  Returns the bg window (minx, miny, edge)."""
    from PIL import Image
    if not af.two_layer:
        raise ValueError("atlas outputs need a two_layer handle (stage1_seg.py)")
    win_bg = af.area_window(af.mapping_area(1))
    tex1, tex2 = af.atlas_texture(res, FG_WINDOW), af.atlas_texture(res, win_bg)
    m1, m2 = af.texture_masks(res, FG_WINDOW, win_bg)
    Image.fromarray(masked_texture(m1, tex1)).save(os.path.join(eval_dir, "texture_orig1.png"))
    Image.fromarray(masked_texture(m2, tex2)).save(os.path.join(eval_dir, "texture_orig2.png"))
    for d in ("alpha", "uv_1", "uv_2"):
        os.makedirs(os.path.join(eval_dir, d), exist_ok=True)
    for f in range(af.cfg.number_of_frames):
        name = "%05d.png" % f
        if size is None:
            L = af.render_layers(f)
            Image.fromarray(to_u8(L["alpha"])).save(os.path.join(eval_dir, "alpha", name))
        else:
            L = af.render_layers_at(f, int(size[0]), int(size[1]), which=("uv1", "uv2"), alpha_u8=True)
            Image.fromarray(L["alpha_u8"]).save(os.path.join(eval_dir, "alpha", name))
        Image.fromarray(to_u8(normalize_uv(L["uv1"], 0.5, FG_WINDOW[2], FG_WINDOW[0], FG_WINDOW[1]))).save(os.path.join(eval_dir, "uv_1", name))
        Image.fromarray(to_u8(normalize_uv(L["uv2"], -0.5, win_bg[2], win_bg[0], win_bg[1]))).save(os.path.join(eval_dir, "uv_2", name))
    return win_bg
