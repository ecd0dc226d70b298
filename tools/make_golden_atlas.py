"""Fixture of the layer-decomposition outputs (include/atlasfit.h: af_render_layers, af_mapping_area, af_render_atlas_texture,
af_render_edit), computed by the REFERENCE's own evaluate.py functions on the CPU.

The reference's src/models/stage_1/evaluate.py is imported read-only with stub modules for cv2 (putText a no-op: the text
overlay is out of scope), skimage and imageio, none of which the functions used here need.  The nets are the four of
tests/golden/ckpt_seg.pt (written by the reference's own modules at iteration 2) on the seg fixture's synthetic video
(tests/golden/seg_small.npz, regenerated from its recorded seed by the oracle).  At iteration 2 the raw alpha is nearly
constant, so the foreground selection (a > 0.95) is empty; a second "scaled" state multiplies the alpha net's output layer
by ALPHA_SCALE around ALPHA_CENTRE (w' = s w, b' = s (b - c)) so that the raw alpha spans about (-1, 1) over the clip.

    AF_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_atlas.py
        -> tests/golden/atlas_seg.npz

Contents (all per-pixel arrays (F, resy, resx, ...)):
  area_{fg,bg}_{raw,scaled}      get_mapping_area's (maxx, minx, maxy, miny, edge) for both alpha states
  uv1, uv2, alpha, rgb1, rgb2    the per-frame layers of evaluate.py:302-337 (scaled state), fp32; *_64 the same in an fp64 twin,
                                 stored rounded to fp32 (the yardstick only needs it to ~3e-8)
  tex_fg, tex_bg                 texture_orig of get_high_res_texture at res 1000 (window (0, 0, 1)) and TEX_BG_RES (the scaled bg
                                 window), SAMPLED to keep the file small: the texels k = 0, s, 2s, ... of the flattened res^2 grid
                                 (s = tex_fg_stride / tex_bg_stride, coprime with res so every row and column is hit), shape (n, 3);
                                 tex_*_e64 = max |fp32 - fp64 twin| over the WHOLE texture
  edit                           the get_colors-driven edit of the synthetic texture pair (EDIT_RES^2, see edit_textures())
  masks1_ref                     masks1 exactly as the reference's fancy-indexed np.maximum assignment leaves it (order-dependent)
  masks1_max, masks2             the true per-texel maximum of alpha, and the bg usage mask
"""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("AF_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "src", "models", "stage_1")):
    raise SystemExit("set AF_REFERENCE to a checkout of the reference repository (the directory holding src/models/stage_1)")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)

_cv2 = types.ModuleType("cv2")
_cv2.putText = lambda *a, **k: None
_cv2.FONT_HERSHEY_SIMPLEX, _cv2.LINE_AA = 0, 16
sys.modules.setdefault("cv2", _cv2)
for _name in ("skimage", "skimage.metrics", "skimage.measure", "imageio"):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules["skimage"].metrics = sys.modules["skimage.metrics"]
sys.modules["skimage"].measure = sys.modules["skimage.measure"]

from src.models.stage_1 import evaluate as E                                  # noqa: E402
from src.models.stage_1.implicit_neural_networks import IMLP                   # noqa: E402
from oracle import atlas_oracle as O                                           # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
ALPHA_SCALE, ALPHA_CENTRE = 0.0, 0.0      # set by main(): recorded in the npz
TEX_RES, TEX_BG_RES, EDIT_RES = 1000, 333, 1000
TEX_FG_STRIDE, TEX_BG_STRIDE = 97, 7          # sampled texels of the stored textures (coprime with 1000 and 333)
EDIT_FREQ = np.array([[3.0, 2.0], [1.0, 4.0]])          # (layer, axis) cycles per texture side of the synthetic edit textures
EDIT_PHASE = np.array([[0.0, 2.0, 4.0], [1.0, 3.0, 5.0]])   # (layer, channel)


def edit_textures(res):
    """The deterministic texture pair the edit vectors use: 0.5 + 0.4 sin(2 pi (kx x + ky y) / res + phase_c), fp32."""
    y, x = np.mgrid[0:res, 0:res].astype(np.float64)
    out = []
    for L in range(2):
        t = np.stack([0.5 + 0.4 * np.sin(2 * np.pi * (EDIT_FREQ[L, 0] * x + EDIT_FREQ[L, 1] * y) / res + EDIT_PHASE[L, c]) for c in range(3)], axis=2)
        out.append(t.astype(np.float32))
    return out


def load_models(scaled, scale=1.0, centre=0.0):
    """mapping1, mapping2, atlas, alpha of ckpt_seg.pt (stage1_neural_atlas_seg.py:127-161 shapes)."""
    g = dict(np.load(os.path.join(GOLDEN, "seg_small.npz")))
    cfg = {str(k): float(v) for k, v in zip(g["config_keys"], g["config_vals"])}
    ck = torch.load(os.path.join(GOLDEN, "ckpt_seg.pt"), map_location="cpu", weights_only=False)
    m1 = IMLP(input_dim=3, output_dim=2, hidden_dim=256, use_positional=False, positional_dim=4, num_layers=6, skip_layers=[], verbose=False)
    m2 = IMLP(input_dim=3, output_dim=2, hidden_dim=256, use_positional=False, positional_dim=2, num_layers=4, skip_layers=[], verbose=False)
    at = IMLP(input_dim=2, output_dim=3, hidden_dim=256, use_positional=True, positional_dim=10, num_layers=8, skip_layers=[4, 7], verbose=False)
    al = IMLP(input_dim=3, output_dim=1, hidden_dim=256, use_positional=True, positional_dim=int(cfg["positional_encoding_num_alpha"]), num_layers=8,
              skip_layers=[], verbose=False)
    for m, key in ((m1, "model_F_mapping1_state_dict"), (m2, "model_F_mapping2_state_dict"), (at, "F_atlas_state_dict"), (al, "model_F_alpha_state_dict")):
        m.load_state_dict(ck[key])
    if scaled:
        with torch.no_grad():
            last = al.hidden[-1]
            last.weight.mul_(scale)
            last.bias.copy_((last.bias - centre) * scale)
    return (m1, m2, at, al), g


def to64(models):
    import copy
    out = [copy.deepcopy(m).double() for m in models]
    for m in out:
        if m.use_positional:
            m.b = m.b.double()
    return out


def layers(models, resx, resy, F):
    """evaluate.py:300-337 for every frame (one batch: the clip has fewer than 100k pixels): raw uv of both mappings, alpha, layer colours."""
    m1, m2, at, al = models
    larger_dim = np.maximum(np.int64(resx), np.int64(resy))
    outs = {k: [] for k in ("uv1", "uv2", "alpha", "rgb1", "rgb2")}
    with torch.no_grad():
        for f in range(F):
            relis_i, reljs_i = torch.where(torch.ones(resy, resx) > 0)
            relis = relis_i.unsqueeze(1) / (larger_dim / 2) - 1
            reljs = reljs_i.unsqueeze(1) / (larger_dim / 2) - 1
            x = torch.cat((reljs, relis, (f / (F / 2.0) - 1) * torch.ones_like(relis)), dim=1)
            u1, u2 = m1(x), m2(x)
            r1, r2 = (at(u1 * 0.5 + 0.5) + 1) * 0.5, (at(u2 * 0.5 - 0.5) + 1) * 0.5
            a = 0.5 * (al(x) + 1.0)
            a = a * 0.99
            a = a + 0.001
            for k, v in (("uv1", u1), ("uv2", u2), ("alpha", a[:, 0]), ("rgb1", r1), ("rgb2", r2)):
                outs[k].append(v.numpy().reshape((resy, resx) + tuple(v.shape[1:])))
    return {k: np.stack(v) for k, v in outs.items()}


def areas(models, mask, resx, resy, F):
    m1, m2, at, al = models
    larger_dim = np.maximum(np.int64(resx), np.int64(resy))
    bg = E.get_mapping_area(m2, al, mask > -1, larger_dim, F, torch.tensor([-0.5, -0.5]), "cpu", invert_alpha=True)
    fg = E.get_mapping_area(m1, al, mask > 0.5, larger_dim, F, torch.tensor([0.5, 0.5]), "cpu", invert_alpha=False, alpha_thresh=0.95)
    return [np.array([float(v) for v in fg], np.float32), np.array([float(v) for v in bg], np.float32)], bg


def main():
    global ALPHA_SCALE, ALPHA_CENTRE
    import contextlib, io
    models, g = load_models(False)
    resx, resy, F = int(g["resx"]), int(g["resy"]), int(g["nframes"])
    video = O.synthetic_seg_video(resx, resy, F, seed=int(g["video_seed"]))
    assert abs(float(video.mask_frames.double().sum()) - float(g["mask_checksum"])) < 1e-6
    mask = video.mask_frames
    quiet = contextlib.redirect_stdout(io.StringIO())
    # the raw alpha of the unscaled net: pre-tanh values z over the clip -> scale / centre that spread z over about (-2.5, 2.5)
    with torch.no_grad():
        larger_dim = max(resx, resy)
        ii, jj, ff = torch.where(torch.ones(resy, resx, F) > 0)
        x = torch.cat((jj.unsqueeze(1) / (larger_dim / 2) - 1, ii.unsqueeze(1) / (larger_dim / 2) - 1, ff.unsqueeze(1) / (F / 2) - 1), dim=1)
        z = np.arctanh(np.clip(models[3](x).numpy().astype(np.float64), -1 + 1e-12, 1 - 1e-12))
    ALPHA_CENTRE = float(np.float32(np.median(z)))
    ALPHA_SCALE = float(np.float32(float("%.3g" % (2.5 / np.abs(z - ALPHA_CENTRE).max()))))
    with quiet:
        area_raw, _ = areas(models, mask, resx, resy, F)
    smodels, _ = load_models(True, ALPHA_SCALE, ALPHA_CENTRE)
    with quiet:
        area_scaled, bg = areas(smodels, mask, resx, resy, F)
    print("alpha scale %g centre %g; areas raw fg %s bg %s; scaled fg %s bg %s" % (ALPHA_SCALE, ALPHA_CENTRE, area_raw[0], area_raw[1], area_scaled[0], area_scaled[1]))
    maxx2, minx2, maxy2, miny2, edge2 = bg
    print("bg window types", type(minx2), type(edge2))
    L = layers(smodels, resx, resy, F)
    torch.set_default_dtype(torch.float64)
    try:
        L64 = layers(to64(smodels), resx, resy, F)
    finally:
        torch.set_default_dtype(torch.float32)
    at = smodels[2]
    _, tex_fg = E.get_high_res_texture(TEX_RES, 0, 0 + 1, 0, 0 + 1, at, "cpu")
    _, tex_bg = E.get_high_res_texture(TEX_BG_RES, minx2, minx2 + edge2, miny2, miny2 + edge2, at, "cpu")
    at64 = to64([at])[0]
    torch.set_default_dtype(torch.float64)
    try:
        _, tex_fg64 = E.get_high_res_texture(TEX_RES, 0, 0 + 1, 0, 0 + 1, at64, "cpu")
        _, tex_bg64 = E.get_high_res_texture(TEX_BG_RES, float(minx2), float(minx2) + float(edge2), float(miny2), float(miny2) + float(edge2), at64, "cpu")
    finally:
        torch.set_default_dtype(torch.float32)
    tex_fg, tex_bg = tex_fg.numpy(), tex_bg.numpy()
    e_fg, e_bg = float(np.abs(tex_fg - tex_fg64.numpy()).max()), float(np.abs(tex_bg - tex_bg64.numpy()).max())
    # evaluate.py:373-438 with the synthetic texture pair (windows as at :248-257: fg (0, 0, 1), bg the scaled state's area)
    t1, t2 = edit_textures(EDIT_RES)
    minx, miny, edge_size = 0, 0, 1
    npx = resy * resx
    ri, rj = np.divmod(np.arange(npx), resx)
    edit = np.zeros((F, resy, resx, 3))
    masks1, masks1_max, masks2 = np.zeros((EDIT_RES, EDIT_RES)), np.zeros((EDIT_RES, EDIT_RES)), np.zeros((EDIT_RES, EDIT_RES))
    for f in range(F):
        u1, u2 = torch.from_numpy(L["uv1"][f].reshape(-1, 2)), torch.from_numpy(L["uv2"][f].reshape(-1, 2))
        alpha = torch.from_numpy(L["alpha"][f].reshape(-1, 1))
        rgb21, px1, py1, rel1 = E.get_colors(EDIT_RES, minx, minx + edge_size, miny, miny + edge_size, u1[:, 0] * 0.5 + 0.5, u1[:, 1] * 0.5 + 0.5, torch.from_numpy(t1))
        rgb22, px2, py2, rel2 = E.get_colors(EDIT_RES, minx2, minx2 + edge2, miny2, miny2 + edge2, u2[:, 0] * 0.5 - 0.5, u2[:, 1] * 0.5 - 0.5, torch.from_numpy(t2))
        a1 = alpha.squeeze()[rel1].numpy()
        for yy, xx in ((np.ceil(py1), np.ceil(px1)), (np.floor(py1), np.floor(px1)), (np.floor(py1), np.ceil(px1)), (np.ceil(py1), np.floor(px1))):
            yy, xx = yy.astype(np.int64), xx.astype(np.int64)
            masks1[yy, xx] = np.maximum(masks1[yy, xx], a1)            # :398-414, duplicates: the last one wins
            np.maximum.at(masks1_max, (yy, xx), a1)                      # the maximum the comment at :417 asks for
        for yy, xx in ((np.ceil(py2), np.ceil(px2)), (np.floor(py2), np.floor(px2)), (np.floor(py2), np.ceil(px2)), (np.ceil(py2), np.floor(px2))):
            masks2[yy.astype(np.int64), xx.astype(np.int64)] = 1
        e1 = rgb21 * alpha.numpy()[rel1]
        e2 = rgb22 * (1 - alpha).numpy()[rel2]
        edit[f, ri[rel1], rj[rel1]] += e1
        edit[f, ri[rel2], rj[rel2]] += e2
    np.savez_compressed(
        os.path.join(GOLDEN, "atlas_seg.npz"),
        resx=resx, resy=resy, nframes=F, video_seed=int(g["video_seed"]), checkpoint="ckpt_seg.pt",
        alpha_scale=np.float32(ALPHA_SCALE), alpha_centre=np.float32(ALPHA_CENTRE),
        area_fg_raw=area_raw[0], area_bg_raw=area_raw[1], area_fg_scaled=area_scaled[0], area_bg_scaled=area_scaled[1],
        tex_res=TEX_RES, tex_bg_res=TEX_BG_RES, edit_res=EDIT_RES, edit_freq=EDIT_FREQ, edit_phase=EDIT_PHASE,
        tex_fg_stride=TEX_FG_STRIDE, tex_bg_stride=TEX_BG_STRIDE,
        tex_fg=tex_fg.reshape(-1, 3)[::TEX_FG_STRIDE].astype(np.float32), tex_bg=tex_bg.reshape(-1, 3)[::TEX_BG_STRIDE].astype(np.float32),
        tex_fg_e64=np.float64(e_fg), tex_bg_e64=np.float64(e_bg),
        edit=edit.astype(np.float32),
        masks1_ref=masks1.astype(np.float32), masks1_max=masks1_max.astype(np.float32), masks2=masks2.astype(np.float32),
        **{k: L[k] for k in L}, **{k + "_64": L64[k].astype(np.float32) for k in L64})
    print("texture fp32-vs-fp64: fg %.3g bg %.3g; masks1 texels where the reference order differs from the max: %d; fg texels used %d, bg %d"
          % (e_fg, e_bg, int((masks1 != masks1_max).sum()), int((masks1_max > 0).sum()), int(masks2.sum())))


if __name__ == "__main__":
    main()
