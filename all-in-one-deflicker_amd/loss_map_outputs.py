"""Per-pixel loss maps of a stage-1 evaluation (reference: src/models/stage_1/evaluate.py:338-384,545-563 fg/bg, :650-705,736 single),
written as PNG sequences and one npz instead of the reference's mp4s and matplotlib panels.  The GPU work is libatlasfit.so's
(af_render_loss_maps, af_render_layers); this module is numpy / PIL only.

    <eval_dir>/residuals/%05d.png      ((rgb_residual + 0.5) * 255).astype(uint8), the frames of residuals_*.mp4 (:557 / :736)
    <eval_dir>/loss_maps.npz           every map of every frame, float32 (F, resy, resx[, 3]), named as AtlasFit.loss_maps
  fg/bg path only:
    <eval_dir>/uv_1_masked/%05d.png    (normalize_uv(uv1) * alpha * 255).astype(uint8) (:561-563)
    <eval_dir>/alpha_vs_mask/%05d.png  (stack(mask, alpha, 0) * 255).astype(uint8) (:551-553)
"""
import os

import numpy as np

from .atlas_outputs import FG_WINDOW, normalize_uv, to_u8


def residual_u8(residual):
    """The reference's cast of a residual frame: ((residual + 0.5) * 255).astype(uint8) in fp64 (truncating; out-of-range values
    wrap as numpy's cast does)."""
    return ((np.asarray(residual, np.float64) + 0.5) * 255).astype(np.uint8)


def uv1_masked(uv1, alpha):
    """evaluate.py:561-563: normalize_uv_images of uv1 on the fg window (0, 0, 1), times alpha, * 255 -> uint8."""
    return to_u8(normalize_uv(uv1, 0.5, FG_WINDOW[2], FG_WINDOW[0], FG_WINDOW[1]) * np.asarray(alpha, np.float64)[:, :, None])


def alpha_vs_mask(mask, alpha):
    """evaluate.py:551-553: channels (mask, alpha, 0) * 255 -> uint8."""
    m = np.asarray(mask, np.float64)
    return to_u8(np.stack((m, np.asarray(alpha, np.float64), np.zeros_like(m)), axis=2))


def write_loss_maps(af, eval_dir, mask_frames=None):
    """All loss-map outputs of an AtlasFit into eval_dir (see the module docstring).  mask_frames (resy, resx, F): the uploaded
    foreground masks, needed on the fg/bg path for alpha_vs_mask."""
    from PIL import Image
    F = af.cfg.number_of_frames
    if af.two_layer:
        if mask_frames is None:
            raise ValueError("the fg/bg loss-map outputs need the mask frames")
        mask_frames = mask_frames.cpu().numpy() if hasattr(mask_frames, "cpu") else np.asarray(mask_frames)
    dirs = ("residuals", "uv_1_masked", "alpha_vs_mask") if af.two_layer else ("residuals",)
    for d in dirs:
        os.makedirs(os.path.join(eval_dir, d), exist_ok=True)
    clip = {}
    for f in range(F):
        maps = af.loss_maps(f)
        for k, v in maps.items():
            clip.setdefault(k, []).append(v)
        name = "%05d.png" % f
        Image.fromarray(residual_u8(maps["rgb_residual"])).save(os.path.join(eval_dir, "residuals", name))
        if af.two_layer:
            L = af.render_layers(f)
            Image.fromarray(uv1_masked(L["uv1"], L["alpha"])).save(os.path.join(eval_dir, "uv_1_masked", name))
            Image.fromarray(alpha_vs_mask(mask_frames[:, :, f], L["alpha"])).save(os.path.join(eval_dir, "alpha_vs_mask", name))
    np.savez_compressed(os.path.join(eval_dir, "loss_maps.npz"), **{k: np.stack(v) for k, v in clip.items()})
