"""Per-pixel loss maps on the GPU (include/atlasfit.h: af_render_loss_maps) against tests/golden/loss_maps.npz, which
tools/make_golden_loss_maps.py computed with the reference's own loss_utils.py functions from the nets of ckpt_seg.pt / ckpt_single.pt
on the seg / single fixture videos.  Rule as tests/test_gpu_atlas_outputs.py: over the clip, no further from the fixture than
2e-6 + twice the reference's own fp32-vs-fp64 distance."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODES = [3, 1, 0]
SEG_MAPS = ("rigidity_loss1", "rigidity_loss2", "flow_loss1", "flow_loss2", "flow_alpha_loss", "rgb_error", "rgb_residual")
SINGLE_MAPS = ("rigidity_loss1", "flow_loss1", "rgb_error", "rgb_residual")
AF_EINVAL = -1


@pytest.fixture(scope="module")
def gl():
    return dict(np.load(os.path.join(GOLDEN, "loss_maps.npz")))


def _seg_handle(golden_seg, video, mode=3, upload=True):
    import aiod_amd
    ck = torch.load(os.path.join(GOLDEN, "ckpt_seg.pt"), map_location="cpu", weights_only=False)
    af = aiod_amd.AtlasFit(aiod_amd.default_config(video.resx, video.resy, video.F, golden_seg["config"], two_layer=True))
    if upload:
        af.upload_video(video.video_frames, video.optical_flows, video.optical_flows_reverse, video.optical_flows_mask,
                        video.optical_flows_reverse_mask, video.mask_frames)
    for net, key in ((aiod_amd.NET_MAPPING1, "model_F_mapping1_state_dict"), (aiod_amd.NET_MAPPING2, "model_F_mapping2_state_dict"),
                     (aiod_amd.NET_ATLAS, "F_atlas_state_dict"), (aiod_amd.NET_ALPHA, "model_F_alpha_state_dict")):
        af.load_state_dict(net, ck[key])
    af.set_mlp_mode(mode)
    return af


def _single_handle(golden, video, mode=3):
    import aiod_amd
    from aiod_amd import stage1 as S
    af = aiod_amd.AtlasFit(aiod_amd.default_config(video.resx, video.resy, video.F, golden["config"]))
    af.upload_video(video.video_frames, video.optical_flows, video.optical_flows_reverse, video.optical_flows_mask, video.optical_flows_reverse_mask)
    S.load_checkpoint(af, os.path.join(GOLDEN, "ckpt_single.pt"))
    af.set_mlp_mode(mode)
    return af


def _clip(af, F, which=None):
    maps = [af.loss_maps(f, which) for f in range(F)]
    return {k: np.stack([m[k] for m in maps]) for k in maps[0]}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", ["seg", "single"])
def test_maps_match_reference(path, mode, gl, golden, golden_seg, small_video, small_seg_video):
    if path == "seg":
        af, names, F = _seg_handle(golden_seg, small_seg_video, mode), SEG_MAPS, small_seg_video.F
    else:
        af, names, F = _single_handle(golden, small_video, mode), SINGLE_MAPS, small_video.F
    got = _clip(af, F)
    assert sorted(got) == sorted(names)
    ratios = {}
    for k in names:
        want, want64 = gl["%s_%s" % (path, k)], gl["%s_%s_64" % (path, k)]
        assert got[k].shape == want.shape and got[k].dtype == np.float32, (k, got[k].shape, want.shape)
        d = float(np.abs(got[k] - want).max())
        e_ref = float(np.abs(want.astype(np.float64) - want64).max())
        e_hip = float(np.abs(got[k].astype(np.float64) - want64).max())
        ratios[k] = (d, e_hip, e_ref)
        assert e_hip <= max(2e-6, 2.0 * e_ref) and d <= 2e-6 + 2.0 * e_ref, (path, mode, k, d, e_hip, e_ref)
    print("%s mode %d (max |hip - ref32|, max |hip - ref64|, max |ref32 - ref64|):" % (path, mode),
          {k: tuple("%.3g" % x for x in v) for k, v in ratios.items()})
    af.close()


def test_rgb_error_sums_to_render_frame_sse(golden, golden_seg, small_video, small_seg_video):
    for af, v in ((_seg_handle(golden_seg, small_seg_video), small_seg_video), (_single_handle(golden, small_video), small_video)):
        _, per0 = af.psnr()
        frames = v.video_frames.numpy()                      # (resy, resx, 3, F)
        for f in range(v.F):
            m = af.loss_maps(f, ("rgb_error", "rgb_residual"))
            rgb, sse = af.render_frame(f)
            s = float(m["rgb_error"].astype(np.float64).sum())
            assert abs(s - sse) <= 1e-5 * sse + 1e-9, (f, s, sse)
            # the residual is the frame minus af_render_frame's rgb (to the blend's fma contraction)
            assert np.abs(m["rgb_residual"] - (frames[..., f] - rgb)).max() <= 1e-6, f
        assert np.array_equal(af.psnr()[1], per0)            # af_psnr's cache does not move
        af.close()


def test_last_frame_flow_and_masked_pixels_are_zero(golden, golden_seg, small_video, small_seg_video):
    for af, v, names in ((_seg_handle(golden_seg, small_seg_video), small_seg_video, ("flow_loss1", "flow_loss2", "flow_alpha_loss")),
                         (_single_handle(golden, small_video), small_video, ("flow_loss1",))):
        mask = v.optical_flows_mask.numpy()[..., 0]          # (resy, resx, F)
        assert (mask[..., -1] == 0).all() and 0 < (mask[..., 0] == 0).sum() < mask[..., 0].size
        for f in range(v.F):
            m = af.loss_maps(f)
            for k in names:
                assert (m[k][mask[..., f] == 0] == 0).all(), (f, k)
                if f < v.F - 1 and k != "flow_alpha_loss":
                    assert (m[k][mask[..., f] > 0] != 0).any(), (f, k)
            if f == v.F - 1:
                for k in ("flow_loss1", "flow_loss2"):
                    if k in m:
                        assert (m[k] == 0).all(), k
        af.close()


def test_null_outputs_untouched_and_subset_matches_all(golden_seg, small_seg_video):
    af = _seg_handle(golden_seg, small_seg_video)
    H, W, F = small_seg_video.resy, small_seg_video.resx, small_seg_video.F
    sentinel = np.float32(-1234.5)
    for f in (0, F - 1):
        full = af.loss_maps(f)
        for k in SEG_MAPS:
            assert np.array_equal(af.loss_maps(f, (k,))[k], full[k]), (f, k)
        assert set(af.loss_maps(f, ("flow_loss2", "rgb_error"))) == {"flow_loss2", "rgb_error"}
        # raw ABI: a guard tail behind every buffer, and outputs passed as NULL stay sentinel-filled in the caller's arrays
        bufs = [np.full(H * W * (3 if k == "rgb_residual" else 1) + 64, sentinel, np.float32) for k in SEG_MAPS]
        on = {"rigidity_loss2", "flow_alpha_loss", "rgb_residual"}
        ptrs = [b.ctypes.data_as(C.c_void_p) if k in on else None for k, b in zip(SEG_MAPS, bufs)]
        assert af.lib.af_render_loss_maps(af.h, f, *ptrs) == 0
        for k, b in zip(SEG_MAPS, bufs):
            n = H * W * (3 if k == "rgb_residual" else 1)
            assert (b[n:] == sentinel).all(), k
            if k in on:
                assert np.array_equal(b[:n], full[k].reshape(-1)), (f, k)
            else:
                assert (b[:n] == sentinel).all(), k
    with pytest.raises(ValueError):
        af.loss_maps(0, ("rigidity",))
    af.close()


def test_error_paths(golden, golden_seg, small_video, small_seg_video):
    import aiod_amd
    af = _seg_handle(golden_seg, small_seg_video)
    H, W, F = small_seg_video.resy, small_seg_video.resx, small_seg_video.F
    buf = np.zeros(H * W * 3, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    for f in (-1, F):
        assert af.lib.af_render_loss_maps(af.h, f, p, None, None, None, None, None, None) == AF_EINVAL
        with pytest.raises(aiod_amd.AtlasFitError) as e:
            af.loss_maps(f)
        assert e.value.code == AF_EINVAL
    af.close()
    nov = _seg_handle(golden_seg, small_seg_video, upload=False)
    assert nov.lib.af_render_loss_maps(nov.h, 0, p, None, None, None, None, None, None) == AF_EINVAL
    nov.close()
    single = _single_handle(golden, small_video)
    for slot in (1, 3, 4):           # rigidity2, flow2, flow_alpha
        args = [None] * 7
        args[slot] = p
        assert single.lib.af_render_loss_maps(single.h, 0, *args) == AF_EINVAL, slot
    with pytest.raises(aiod_amd.AtlasFitError) as e:
        single.loss_maps(0, ("flow_alpha_loss",))
    assert e.value.code == AF_EINVAL
    assert sorted(single.loss_maps(0)) == sorted(SINGLE_MAPS)
    single.close()


def test_call_between_train_blocks_changes_nothing(golden_seg, small_seg_video):
    import aiod_amd
    af = _seg_handle(golden_seg, small_seg_video)
    ck = torch.load(os.path.join(GOLDEN, "ckpt_seg.pt"), map_location="cpu", weights_only=False)
    nets = ((aiod_amd.NET_MAPPING1, "model_F_mapping1_state_dict"), (aiod_amd.NET_MAPPING2, "model_F_mapping2_state_dict"),
            (aiod_amd.NET_ATLAS, "F_atlas_state_dict"), (aiod_amd.NET_ALPHA, "model_F_alpha_state_dict"))
    outs = []
    for call in (False, True):
        for net, key in nets:
            af.load_state_dict(net, ck[key])
            z = np.zeros(af.param_count(net), np.float32)
            af.set_adam_state(net, z, z, 0)
        first = af.train_steps(0, 3, None, seed=7)
        if call:
            for f in range(small_seg_video.F):
                af.loss_maps(f)
        outs.append((first, af.train_steps(3, 3, None, seed=7)))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1]), (outs[0][1], outs[1][1])
    assert np.isfinite(outs[1][1]).all()
    af.close()
