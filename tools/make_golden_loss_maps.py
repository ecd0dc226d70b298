"""Fixture of the per-pixel loss maps (include/atlasfit.h: af_render_loss_maps), computed by the REFERENCE's own loss_utils.py
functions on the CPU, per frame as evaluate.py:300-384 (fg/bg) and :640-705 (single) call them.

The reference's src/models/stage_1/loss_utils.py is imported read-only.  Two parts:
  seg_*     the four nets of tests/golden/ckpt_seg.pt (as stored, no alpha rescale) on the seg fixture's video
            (tests/golden/seg_small.npz, regenerated from its recorded seed by the oracle, constant flow)
  single_*  mapping1 and atlas of tests/golden/ckpt_single.pt on the single fixture's video (tests/golden/single_small.npz)

    AF_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_loss_maps.py
        -> tests/golden/loss_maps.npz

Per path, every map of the whole clip (the videos are 40 x 24 x 6): rigidity_loss1/2, flow_loss1/2, flow_alpha_loss (F, resy, resx),
rgb_error (F, resy, resx), rgb_residual (F, resy, resx, 3), fp32; <name>_64 the same from an fp64 twin of the nets and inputs, fp64.
The single path has no rigidity_loss2 / flow_loss2 / flow_alpha_loss.
"""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("AF_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "src", "models", "stage_1")):
    raise SystemExit("set AF_REFERENCE to a checkout of the reference repository (the directory holding src/models/stage_1)")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)

from src.models.stage_1.loss_utils import (get_rigidity_loss, get_optical_flow_loss_all,            # noqa: E402
                                           get_optical_flow_alpha_loss_all)
from src.models.stage_1.implicit_neural_networks import IMLP                                         # noqa: E402
from oracle import atlas_oracle as O                                                                  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _config(g):
    return {str(k): float(v) for k, v in zip(g["config_keys"], g["config_vals"])}


def seg_models():
    """mapping1, mapping2, atlas, alpha of ckpt_seg.pt (stage1_neural_atlas_seg.py:127-161 shapes)."""
    g = dict(np.load(os.path.join(GOLDEN, "seg_small.npz")))
    cfg = _config(g)
    ck = torch.load(os.path.join(GOLDEN, "ckpt_seg.pt"), map_location="cpu", weights_only=False)
    m1 = IMLP(input_dim=3, output_dim=2, hidden_dim=256, use_positional=False, positional_dim=4, num_layers=6, skip_layers=[], verbose=False)
    m2 = IMLP(input_dim=3, output_dim=2, hidden_dim=256, use_positional=False, positional_dim=2, num_layers=4, skip_layers=[], verbose=False)
    at = IMLP(input_dim=2, output_dim=3, hidden_dim=256, use_positional=True, positional_dim=10, num_layers=8, skip_layers=[4, 7], verbose=False)
    al = IMLP(input_dim=3, output_dim=1, hidden_dim=256, use_positional=True, positional_dim=int(cfg["positional_encoding_num_alpha"]), num_layers=8,
              skip_layers=[], verbose=False)
    for m, key in ((m1, "model_F_mapping1_state_dict"), (m2, "model_F_mapping2_state_dict"), (at, "F_atlas_state_dict"), (al, "model_F_alpha_state_dict")):
        m.load_state_dict(ck[key])
    video = O.synthetic_seg_video(int(g["resx"]), int(g["resy"]), int(g["nframes"]), seed=int(g["video_seed"]))
    assert abs(float(video.video_frames.double().sum()) - float(g["video_checksum"])) < 1e-6
    return (m1, m2, at, al), video, cfg


def single_models():
    """mapping1, atlas of ckpt_single.pt (stage1_neural_atlas.py:112-128 shapes from the fixture's config)."""
    g = dict(np.load(os.path.join(GOLDEN, "single_small.npz")))
    cfg = _config(g)
    ck = torch.load(os.path.join(GOLDEN, "ckpt_single.pt"), map_location="cpu", weights_only=False)
    m1 = IMLP(input_dim=3, output_dim=2, hidden_dim=int(cfg["number_of_channels_mapping1"]), use_positional=bool(cfg["use_positional_encoding_mapping1"]),
              positional_dim=int(cfg["number_of_positional_encoding_mapping1"]), num_layers=int(cfg["number_of_layers_mapping1"]), skip_layers=[], verbose=False)
    at = IMLP(input_dim=2, output_dim=3, hidden_dim=int(cfg["number_of_channels_atlas"]), use_positional=True,
              positional_dim=int(cfg["positional_encoding_num_atlas"]), num_layers=int(cfg["number_of_layers_atlas"]), skip_layers=[4, 7], verbose=False)
    m1.load_state_dict(ck["model_F_mapping1_state_dict"])
    at.load_state_dict(ck["F_atlas_state_dict"])
    video = O.synthetic_video(int(g["resx"]), int(g["resy"]), int(g["nframes"]), seed=int(g["video_seed"]))
    assert abs(float(video.video_frames.double().sum()) - float(g["video_checksum"])) < 1e-6
    return (m1, at), video, cfg


def to64(models):
    import copy
    out = [copy.deepcopy(m).double() for m in models]
    for m in out:
        if m.use_positional:
            m.b = m.b.double()
    return out


def loss_maps(models, video, cfg, seg, f64=False):
    """evaluate.py:300-384 (seg) / :640-705 (single) for every frame, one batch per frame (the clip has fewer than 100k pixels)."""
    resx, resy, F = video.resx, video.resy, video.F
    larger_dim = np.maximum(resx, resy)
    d, uvs = int(cfg["derivative_amount"]), cfg["uv_mapping_scale"]
    dt = torch.float64 if f64 else torch.float32
    frames = video.video_frames.to(dt)
    flows, mask = video.optical_flows.to(dt), video.optical_flows_mask
    if seg:
        m1, m2, at, al = models
    else:
        m1, at = models
    names = ("rigidity_loss1", "flow_loss1", "rgb_error", "rgb_residual") + (("rigidity_loss2", "flow_loss2", "flow_alpha_loss") if seg else ())
    outs = {k: [] for k in names}
    with torch.no_grad():
        for f in range(F):
            relis_i, reljs_i = torch.where(torch.ones(resy, resx) > 0)
            relis = relis_i.unsqueeze(1) / (larger_dim / 2) - 1
            reljs = reljs_i.unsqueeze(1) / (larger_dim / 2) - 1
            x = torch.cat((reljs, relis, (f / (F / 2.0) - 1) * torch.ones_like(relis)), dim=1)
            jif = torch.cat((reljs_i.unsqueeze(-1), relis_i.unsqueeze(-1), torch.ones_like(relis_i.unsqueeze(-1)) * f), dim=1).T.unsqueeze(-1)
            u1 = m1(x)
            r1 = (at(u1 * 0.5 + 0.5) + 1) * 0.5
            if seg:
                u2 = m2(x)
                r2 = (at(u2 * 0.5 - 0.5) + 1) * 0.5
                alpha = 0.5 * (al(x) + 1.0)
                alpha = alpha * 0.99
                alpha = alpha + 0.001
                rgb = r1 * alpha + r2 * (1.0 - alpha)
            else:
                alpha = torch.ones(r1.shape[0], 1, dtype=dt)
                rgb = r1
            res = {"rigidity_loss1": get_rigidity_loss(jif, d, larger_dim, F, m1, u1, "cpu", uv_mapping_scale=uvs, return_all=True)}
            if f < F - 1:
                res["flow_loss1"] = get_optical_flow_loss_all(jif, u1, larger_dim, F, m1, flows, mask, uvs, "cpu", alpha=alpha)
            else:
                res["flow_loss1"] = torch.zeros_like(relis).squeeze()
            if seg:
                res["rigidity_loss2"] = get_rigidity_loss(jif, d, larger_dim, F, m2, u2, "cpu", uv_mapping_scale=uvs, return_all=True)
                if f < F - 1:
                    res["flow_loss2"] = get_optical_flow_loss_all(jif, u2, larger_dim, F, m2, flows, mask, uvs, "cpu", alpha=1 - alpha)
                else:
                    res["flow_loss2"] = torch.zeros_like(relis).squeeze()
                res["flow_alpha_loss"] = get_optical_flow_alpha_loss_all(al, jif, alpha, larger_dim, F, flows, mask, "cpu")
            gt = frames[relis_i, reljs_i, :, f]
            res["rgb_error"] = (gt - rgb).norm(dim=1) ** 2
            res["rgb_residual"] = gt - rgb
            for k in names:
                v = res[k].numpy()
                outs[k].append(v.reshape((resy, resx, 3) if k == "rgb_residual" else (resy, resx)))
    return {k: np.stack(v) for k, v in outs.items()}


def run(models, video, cfg, seg):
    out32 = loss_maps(models, video, cfg, seg)
    torch.set_default_dtype(torch.float64)
    try:
        out64 = loss_maps(to64(models), video, cfg, seg, f64=True)
    finally:
        torch.set_default_dtype(torch.float32)
    for k in out32:
        assert out32[k].dtype == np.float32 and out64[k].dtype == np.float64, (k, out32[k].dtype, out64[k].dtype)
    return out32, out64


def main():
    parts = {}
    for tag, (models, video, cfg), seg in (("seg", seg_models(), True), ("single", single_models(), False)):
        m32, m64 = run(models, video, cfg, seg)
        for k in m32:
            parts["%s_%s" % (tag, k)] = m32[k]
            parts["%s_%s_64" % (tag, k)] = m64[k]
            print("%-6s %-16s max %.4g  fp32-vs-fp64 %.3g" % (tag, k, float(np.abs(m32[k]).max()), float(np.abs(m32[k] - m64[k]).max())))
        parts["%s_shape" % tag] = np.array([video.F, video.resy, video.resx])
    np.savez_compressed(os.path.join(GOLDEN, "loss_maps.npz"), seg_checkpoint="ckpt_seg.pt", single_checkpoint="ckpt_single.pt", **parts)


if __name__ == "__main__":
    main()
