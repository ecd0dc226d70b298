"""Layer decomposition of the fg/bg path on the GPU (include/atlasfit.h: af_render_layers, af_mapping_area, af_render_atlas_texture,
af_render_edit) against tests/golden/atlas_seg.npz, which tools/make_golden_atlas.py computed with the reference's own evaluate.py
functions from the nets of ckpt_seg.pt on the seg fixture's video.  Per-pixel rule as tests/test_gpu_seg.py's render test: no further
from the fixture than 2e-6 + twice the reference's own fp32-vs-fp64 distance."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODES = [3, 1, 0]


@pytest.fixture(scope="module")
def ga():
    return dict(np.load(os.path.join(GOLDEN, "atlas_seg.npz")))


def _seg_handle(golden_seg, video, ga, scaled=True, mode=3):
    """Two-layer handle on the seg video with the nets of ckpt_seg.pt; `scaled`: the alpha net's output layer rescaled as the
    fixture generator does (w * s, (b - c) * s in fp32)."""
    import aiod_amd
    ck = torch.load(os.path.join(GOLDEN, "ckpt_seg.pt"), map_location="cpu", weights_only=False)
    af = aiod_amd.AtlasFit(aiod_amd.default_config(video.resx, video.resy, video.F, golden_seg["config"], two_layer=True))
    af.upload_video(video.video_frames, video.optical_flows, video.optical_flows_reverse, video.optical_flows_mask, video.optical_flows_reverse_mask,
                    video.mask_frames)
    sd_al = {k: v.clone() for k, v in ck["model_F_alpha_state_dict"].items()}
    if scaled:
        last = max(int(k.split(".")[1]) for k in sd_al)
        s, c = torch.tensor(float(ga["alpha_scale"])), torch.tensor(float(ga["alpha_centre"]))
        sd_al["hidden.%d.weight" % last] = sd_al["hidden.%d.weight" % last] * s
        sd_al["hidden.%d.bias" % last] = (sd_al["hidden.%d.bias" % last] - c) * s
    af.load_state_dict(aiod_amd.NET_MAPPING1, ck["model_F_mapping1_state_dict"])
    af.load_state_dict(aiod_amd.NET_MAPPING2, ck["model_F_mapping2_state_dict"])
    af.load_state_dict(aiod_amd.NET_ATLAS, ck["F_atlas_state_dict"])
    af.load_state_dict(aiod_amd.NET_ALPHA, sd_al)
    af.set_mlp_mode(mode)
    return af


def _check(got, want, want64, what, k=2.0):
    d, e_ref, e_hip = float(np.abs(got - want).max()), float(np.abs(want - want64).max()), float(np.abs(got - want64).max())
    assert e_hip <= max(2e-6, k * e_ref) and d <= 2e-6 + k * e_ref, (what, d, e_hip, e_ref)
    return d


def _uv_tol(ga):
    return 2e-6 + 2.0 * max(float(np.abs(ga[k] - ga[k + "_64"]).max()) for k in ("uv1", "uv2"))


@pytest.mark.parametrize("mode", MODES)
def test_layers_match_reference_per_pixel(mode, ga, golden_seg, small_seg_video):
    af = _seg_handle(golden_seg, small_seg_video, ga, mode=mode)
    worst = {}
    for f in range(small_seg_video.F):
        L = af.render_layers(f)
        for k in ("uv1", "uv2", "alpha", "rgb1", "rgb2"):
            # alpha of the scaled state: the fixture multiplies the alpha net's output layer by ~1400, so each arithmetic's last-layer
            # rounding reaches alpha 1400-fold and one fp32 realisation (e_ref) is a thin yardstick: 4x for the bf16x6 / fp32 chains
            # (measured 2.5x and 3.0x; f16x3 stays inside 2x)
            worst[k] = max(worst.get(k, 0.0), _check(L[k], ga[k][f], ga[k + "_64"][f], (mode, f, k), 4.0 if (k == "alpha" and mode != 3) else 2.0))
    print("mode %d layers vs reference, worst per output:" % mode, worst)
    af.close()


def test_layers_compose_to_render_frame_and_leave_psnr_alone(ga, golden_seg, small_seg_video):
    """af_render_frame's rgb is the finish kernel's written-out blend of af_render_layers' values, bit for bit (tests/blend_ref.py):
    channel 1 = fl(fl(rgb1 a) + fl(rgb2 fl(1 - a))), channels 0 and 2 = the correctly rounded fma(a, rgb1, fl(rgb2 fl(1 - a))).  The two
    kernels round alpha differently (one fma in k_layer_finish, two roundings in the finish kernel), so a pixel may need an alpha one or
    two float32 steps from render_layers'; those pixels also keep the earlier rule (either fused form, or within two ulps).  The count is
    printed and recorded in MEASUREMENTS.md Part T.  af_psnr's cache does not move under interleaved layer / area / texture / edit calls."""
    from blend_ref import check_composes
    af = _seg_handle(golden_seg, small_seg_video, ga)
    m0, per0 = af.psnr()
    for f in range(small_seg_video.F):
        L = af.render_layers(f)
        af.mapping_area(1); af.atlas_texture(37, (0.0, 0.0, 1.0))
        af.render_edit(f, 64, np.full((64, 64, 3), 0.5, np.float32), (0, 0, 1), None, None, outputs=("edit",))
        rgb, _ = af.render_frame(f)
        check_composes(rgb, L, "ckpt state, frame %d" % f)
    m1, per1 = af.psnr()
    assert m1 == m0 and np.array_equal(per0, per1)
    af2 = _seg_handle(golden_seg, small_seg_video, ga)         # and from a fresh handle: the same per-frame PSNR
    assert np.array_equal(af2.psnr()[1], per0)
    af.close(); af2.close()


def test_single_handle_rgb1_is_render_frame(golden, small_video):
    import aiod_amd
    from aiod_amd import stage1 as S
    v = small_video
    af = aiod_amd.AtlasFit(aiod_amd.default_config(v.resx, v.resy, v.F, golden["config"]))
    af.upload_video(v.video_frames, v.optical_flows, v.optical_flows_reverse, v.optical_flows_mask, v.optical_flows_reverse_mask)
    S.load_checkpoint(af, os.path.join(GOLDEN, "ckpt_single.pt"))
    for f in range(v.F):
        L = af.render_layers(f)
        rgb, _ = af.render_frame(f)
        assert np.array_equal(L["rgb1"], rgb) and (L["alpha"] == 1).all() and L["uv2"] is None and np.isfinite(L["uv1"]).all()
    tex = af.atlas_texture(50, (0.0, 0.0, 1.0))
    assert tex.shape == (50, 50, 3) and np.isfinite(tex).all()
    with pytest.raises(aiod_amd.AtlasFitError) as e:
        af.mapping_area(1)
    assert e.value.code == -5
    with pytest.raises(aiod_amd.AtlasFitError) as e:
        af.render_edit(0, 16, None, (0, 0, 1), None, None, use_fg=np.zeros((16, 16), np.float32), outputs=())
    assert e.value.code == -5
    uv2 = np.empty((v.resy, v.resx, 2), np.float32)
    assert af.lib.af_render_layers(af.h, 0, None, uv2.ctypes.data_as(C.c_void_p), None, None, None) == -1
    af.close()


@pytest.mark.parametrize("mode", MODES)
def test_mapping_area_matches_reference(mode, ga, golden_seg, small_seg_video):
    tol = _uv_tol(ga)
    for scaled in (False, True):
        af = _seg_handle(golden_seg, small_seg_video, ga, scaled=scaled, mode=mode)
        tag = "scaled" if scaled else "raw"
        for which, name in ((0, "fg"), (1, "bg")):
            got = np.array(af.mapping_area(which), np.float32)
            want = ga["area_%s_%s" % (name, tag)]
            print("mode %d %s %s area: got %s want %s" % (mode, tag, name, got, want))
            if want[4] == -2:           # the empty selection: the reference's exact values
                assert got.tolist() == [-1.0, 1.0, -1.0, 1.0, -2.0]
            else:
                assert np.abs(got[:4] - want[:4]).max() <= tol and abs(got[4] - want[4]) <= 2 * tol, (got, want, tol)
        af.close()


@pytest.mark.parametrize("mode", MODES)
def test_atlas_texture_matches_reference(mode, ga, golden_seg, small_seg_video):
    af = _seg_handle(golden_seg, small_seg_video, ga, mode=mode)
    fg = af.atlas_texture(int(ga["tex_res"]), (0.0, 0.0, 1.0))
    e = float(ga["tex_fg_e64"])
    # the fixture stores every tex_*_stride-th texel of the flattened grid (strides coprime with res: every row and column is sampled)
    d_fg = float(np.abs(fg.reshape(-1, 3)[::int(ga["tex_fg_stride"])] - ga["tex_fg"]).max())
    assert d_fg <= 2e-6 + 2.0 * e, (d_fg, e)
    area = ga["area_bg_scaled"]
    win = (area[1], area[3], area[4])
    res = int(ga["tex_bg_res"])
    bg = af.atlas_texture(res, win)
    d_bg = float(np.abs(bg.reshape(-1, 3)[::int(ga["tex_bg_stride"])] - ga["tex_bg"]).max())
    assert d_bg <= 2e-6 + 2.0 * float(ga["tex_bg_e64"]), (d_bg, float(ga["tex_bg_e64"]))
    # the grid itself: torch.linspace's rows / columns through the same atlas chain give the texture bit for bit
    import aiod_amd
    xs = torch.linspace(float(win[0]), float(np.float32(win[0] + win[2])), res).numpy()
    ys = torch.linspace(float(win[1]), float(np.float32(win[1] + win[2])), res).numpy()
    rows = np.zeros((res * res, 4), np.float32)
    rows[:, 0] = np.tile(xs, res); rows[:, 1] = np.repeat(ys, res)
    t = af.debug_forward(aiod_amd.NET_ATLAS, rows)[:, :3]
    assert np.array_equal(bg.reshape(-1, 3), (np.float32(0.5) * (t + np.float32(1))).astype(np.float32))
    print("mode %d texture vs reference: fg 1000^2 %.3g (fp64 yardstick %.3g), bg %d^2 %.3g" % (mode, d_fg, e, res, d_bg))
    af.close()


def _get_colors(res, minx, miny, edge, px_uv, py_uv, image):
    """evaluate.py:24-84 (get_colors + bilinear_interpolate_numpy) restated on numpy inputs: returns pixels, pointx2, pointy2, relevant."""
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


def _textures(ga):
    """The synthetic texture pair of tools/make_golden_atlas.py (edit_textures), from the parameters recorded in the fixture."""
    res = int(ga["edit_res"])
    y, x = np.mgrid[0:res, 0:res].astype(np.float64)
    out = []
    for L in range(2):
        t = np.stack([0.5 + 0.4 * np.sin(2 * np.pi * (ga["edit_freq"][L, 0] * x + ga["edit_freq"][L, 1] * y) / res + ga["edit_phase"][L, c]) for c in range(3)], axis=2)
        out.append(t.astype(np.float32))
    return out


def test_edit_and_masks(ga, golden_seg, small_seg_video):
    """Edits of the library's OWN uv / alpha agree with the reference's get_colors (restated) to 1e-6; masks1 is the true maximum of
    the library's own alpha over the touched texels; masks2 equals the fixture except on texels a floor / ceil flip moves."""
    v = small_seg_video
    af = _seg_handle(golden_seg, v, ga)
    t1, t2 = _textures(ga)
    res = int(ga["edit_res"])
    area = ga["area_bg_scaled"]
    win_fg, win_bg = (0.0, 0.0, 1.0), (area[1], area[3], area[4])
    u1, u2 = np.zeros((res, res), np.float32), np.zeros((res, res), np.float32)
    m1_want, m2_want = np.zeros((res, res)), np.zeros((res, res))
    worst = 0.0
    for f in range(v.F):
        got = af.render_edit(f, res, t1, win_fg, t2, win_bg, use_fg=u1, use_bg=u2)
        L = af.render_layers(f)
        uv1, uv2, a = L["uv1"].reshape(-1, 2), L["uv2"].reshape(-1, 2), L["alpha"].reshape(-1)
        p1, x1, y1, r1 = _get_colors(res, win_fg[0], win_fg[1], win_fg[2], uv1[:, 0] * np.float32(0.5) + np.float32(0.5), uv1[:, 1] * np.float32(0.5) + np.float32(0.5), t1)
        p2, x2, y2, r2 = _get_colors(res, win_bg[0], win_bg[1], win_bg[2], uv2[:, 0] * np.float32(0.5) - np.float32(0.5), uv2[:, 1] * np.float32(0.5) - np.float32(0.5), t2)
        e1, e2, e = (np.zeros((a.size, 3)) for _ in range(3))
        e1[r1] = p1 * a[r1][:, None]
        e2[r2] = p2
        e[r1] += p1 * a[r1][:, None]
        e[r2] += p2 * (np.float32(1) - a)[r2][:, None]
        for k, want in (("edit", e), ("edit_fg", e1), ("edit_bg", e2)):
            d = float(np.abs(got[k].reshape(-1, 3) - want).max())
            worst = max(worst, d)
            assert d <= 1e-6, (f, k, d)
        for yy, xx in ((np.ceil(y1), np.ceil(x1)), (np.floor(y1), np.floor(x1)), (np.floor(y1), np.ceil(x1)), (np.ceil(y1), np.floor(x1))):
            np.maximum.at(m1_want, (yy.astype(int), xx.astype(int)), a[r1])
        for yy, xx in ((np.ceil(y2), np.ceil(x2)), (np.floor(y2), np.floor(x2)), (np.floor(y2), np.ceil(x2)), (np.ceil(y2), np.floor(x2))):
            m2_want[yy.astype(int), xx.astype(int)] = 1
    assert np.array_equal(u1, m1_want.astype(np.float32)) and np.array_equal(u2, m2_want.astype(np.float32))
    # against the fixture: the texels the reference touched and the library did not (or the other way round) are floor / ceil flips
    flips2 = int((u2 != ga["masks2"]).sum())
    flips1 = int(((u1 > 0) != (ga["masks1_max"] > 0)).sum())
    print("edit vs restated get_colors: worst %.3g; masks2 texels that differ from the fixture: %d of %d used; masks1 support: %d of %d"
          % (worst, flips2, int(ga["masks2"].sum()), flips1, int((ga["masks1_max"] > 0).sum())))
    assert flips2 <= max(4, 0.01 * ga["masks2"].sum()) and flips1 <= max(4, 0.05 * (ga["masks1_max"] > 0).sum())
    m1b, m2b = af.texture_masks(res, win_fg, win_bg)          # the convenience: the same accumulation over all frames
    assert np.array_equal(m1b, u1) and np.array_equal(m2b, u2)
    af.close()


def test_error_paths_and_null_outputs(ga, golden_seg, small_seg_video):
    import aiod_amd
    v = small_seg_video
    af = _seg_handle(golden_seg, v, ga)
    for call in (lambda: af.render_layers(-1), lambda: af.render_layers(v.F), lambda: af.atlas_texture(0, (0, 0, 1)),
                 lambda: af.render_edit(v.F, 8, None, (0, 0, 1), None, None, use_fg=np.zeros((8, 8), np.float32), outputs=()),
                 lambda: af.render_edit(0, 0, None, (0, 0, 1), None, None, outputs=()), lambda: af.mapping_area(2),
                 lambda: af.render_edit(0, 8, None, (0, 0, 1), None, None, outputs=("edit_fg",))):
        with pytest.raises(aiod_amd.AtlasFitError) as e:
            call()
        assert e.value.code == -1
    full = af.render_layers(2)
    alpha = np.full((v.resy, v.resx), -7.0, np.float32)
    assert af.lib.af_render_layers(af.h, 2, None, None, alpha.ctypes.data_as(C.c_void_p), None, None) == 0
    assert np.array_equal(alpha, full["alpha"])
    bg_use = np.full((8, 8), -7.0, np.float32)          # a layer without a window is skipped: its usage array is not touched
    edit_bg = np.full((v.resy, v.resx, 3), -7.0, np.float32)
    fg_use = np.zeros((8, 8), np.float32)
    tex = np.full((8, 8, 3), 0.25, np.float32)
    win = np.array([0, 0, 1], np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert af.lib.af_render_edit(af.h, 1, 8, p(tex), p(win), None, None, None, None, None, p(fg_use), None) == 0
    assert (bg_use == -7.0).all() and (edit_bg == -7.0).all() and fg_use.max() > 0
    af.close()
    bare = aiod_amd.AtlasFit(aiod_amd.default_config(v.resx, v.resy, v.F, golden_seg["config"], two_layer=True))   # no video
    with pytest.raises(aiod_amd.AtlasFitError) as e:
        bare.mapping_area(1)
    assert e.value.code == -5
    bare.close()


def test_cli_atlas_outputs_and_identity_edit(tmp_path, small_seg_video, monkeypatch):
    """stage1_seg --atlas_outputs writes texture_orig1/2.png, alpha/, uv_1/, uv_2/ with the values the library's calls give on the
    checkpoint; without the flag the tree is today's; atlas_edit.py fed the unmasked textures reproduces the reconstruction."""
    from PIL import Image
    import aiod_amd
    import aiod_amd.stage1 as S
    from aiod_amd import atlas_edit
    from aiod_amd.atlas_outputs import FG_WINDOW, masked_texture, normalize_uv, to_u8
    from test_stage1_host import _write_masks, _write_video
    v = small_seg_video
    _write_video(tmp_path / "data", v, "clip")
    _write_masks(tmp_path / "data", v, "clip")
    cfg = dict(aiod_amd.atlasfit.REFERENCE_CONFIG)
    cfg.update(samples_batch=256, iters_num=21, evaluate_every=20, pretrain_iter_number=2, stop_global_rigidity=10, stop_bootstrapping_iteration=15)
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    argv = ["--config", str(tmp_path / "cfg.json"), "--vid_name", "clip", "--root", str(tmp_path / "data"), "--seed", "5"]
    plain, flagged = tmp_path / "plain", tmp_path / "flagged"
    plain.mkdir(); flagged.mkdir()
    monkeypatch.chdir(plain)
    S._cli(argv, two_layer=True)
    monkeypatch.chdir(flagged)
    S._cli(argv + ["--atlas_outputs"], two_layer=True)
    tree = lambda d: sorted(str(p.relative_to(d)) for p in d.rglob("*") if p.is_file())
    res_dir = flagged / "results" / "clip" / "stage_1"
    ev = res_dir / "000020"
    new = {"000020/texture_orig1.png", "000020/texture_orig2.png"} | {"000020/%s/%05d.png" % (d, f) for d in ("alpha", "uv_1", "uv_2") for f in range(v.F)}
    got_tree = tree(res_dir)
    assert set(got_tree) - new == set(tree(plain / "results" / "clip" / "stage_1")) and new <= set(got_tree)
    # expected values from the checkpoint the run wrote
    af = aiod_amd.AtlasFit(aiod_amd.default_config(v.resx, v.resy, v.F, cfg, two_layer=True))
    af.upload_video(v.video_frames, v.optical_flows, v.optical_flows_reverse, v.optical_flows_mask, v.optical_flows_reverse_mask, v.mask_frames)
    S.load_checkpoint(af, res_dir / "checkpoint")
    win_bg = af.area_window(af.mapping_area(1))
    tex1, tex2 = af.atlas_texture(1000, FG_WINDOW), af.atlas_texture(1000, win_bg)
    m1, m2 = af.texture_masks(1000, FG_WINDOW, win_bg)
    assert m2.sum() > 0
    png = lambda p: np.array(Image.open(p))
    assert np.array_equal(png(ev / "texture_orig1.png"), masked_texture(m1, tex1)) and np.array_equal(png(ev / "texture_orig2.png"), masked_texture(m2, tex2))
    for f in range(v.F):
        L = af.render_layers(f)
        assert np.array_equal(png(ev / "alpha" / ("%05d.png" % f)), to_u8(L["alpha"]))
        assert np.array_equal(png(ev / "uv_1" / ("%05d.png" % f)), to_u8(normalize_uv(L["uv1"], 0.5, 1, 0, 0)))
        assert np.array_equal(png(ev / "uv_2" / ("%05d.png" % f)), to_u8(normalize_uv(L["uv2"], -0.5, win_bg[2], win_bg[0], win_bg[1])))
    # identity edit: the unmasked textures re-fed through atlas_edit.py
    Image.fromarray(to_u8(tex1)).save(str(tmp_path / "t1.png")); Image.fromarray(to_u8(tex2)).save(str(tmp_path / "t2.png"))
    atlas_edit._cli(["--vid_name", "clip", "--root", str(tmp_path / "data"), "--edit_fg", str(tmp_path / "t1.png"), "--edit_bg", str(tmp_path / "t2.png")])
    t1r = (png(tmp_path / "t1.png").astype(np.float64) / 255).astype(np.float32)
    t2r = (png(tmp_path / "t2.png").astype(np.float64) / 255).astype(np.float32)
    diffs = []
    for f in range(v.F):
        e = af.render_edit(f, 1000, t1r, FG_WINDOW, t2r, win_bg)
        both = (np.abs(e["edit_fg"]).sum(axis=2) > 0) & (np.abs(e["edit_bg"]).sum(axis=2) > 0)
        out = png(res_dir / "edit" / ("%05d.png" % f))
        assert np.array_equal(out, to_u8(e["edit"]))
        rec = png(res_dir / "output" / ("%05d.png" % f)).astype(int)
        diffs.append(np.abs(out.astype(int) - rec)[both])
    diffs = np.concatenate(diffs)
    print("identity edit vs reconstruction (uint8 levels) where both layers are relevant: n %d, max %d, 99th pct %.1f, mean %.3f"
          % (diffs.size, diffs.max(), np.percentile(diffs, 99), diffs.mean()))
    # not exact: the edit resamples a 1000^2 uint8 image of the atlas bilinearly, and a 21-iteration atlas still carries its high positional-
    # encoding frequencies (periods of a few texels); measured mean 2.1, 99th percentile 7 levels (MEASUREMENTS.md).  The exact statement
    # is the one above: the written frames are af_render_edit's values
    assert diffs.size > 0 and np.percentile(diffs, 99) <= 12 and diffs.mean() <= 3.0
    af.close()
