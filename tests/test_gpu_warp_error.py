"""Warping error on the GPU (include/atlasfit.h: af_warp_error_pair, af_warp_error) against tests/golden/warp_error.npz, which
tools/make_golden_warp_error.py computed with the reference's own flow_warping / detect_occlusion (src/models/utils.py:504-572).

Rules: warped within 2e-6 + twice the reference's own fp32-vs-fp64 distance; noc identical wherever both fp64 margins of the
occlusion tests lie outside the fixture's band (the fixture records how many pixels fall inside it: none); E_t within a relative
ERR_RTOL of the fixture's (the fixture's E sums the reference's fp32 warp in fp64, the kernel sums its own; measured ~1e-7)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
AF_EINVAL, AF_ESTATE = -1, -5
ERR_RTOL = 1e-6
MODES = [3, 1, 0]


@pytest.fixture(scope="module")
def gw():
    return dict(np.load(os.path.join(GOLDEN, "warp_error.npz")))


def _pair(i1, i2, f12, f21, align, maps=True):
    import aiod_amd
    return aiod_amd.warp_error_pair(i1, i2, f12, f21, align_corners=bool(align), return_maps=maps)


@pytest.mark.parametrize("geometry", [0, 1])
@pytest.mark.parametrize("shape", [0, 1])
def test_pair_matches_reference(shape, geometry, gw):
    fr, fw, bw = gw["s%d_frames" % shape], gw["s%d_fw" % shape], gw["s%d_bw" % shape]
    k = "s%d_g%d_" % (shape, geometry)
    b1, b2 = gw["band"]
    assert (gw[k + "inband"] == 0).all(), gw[k + "inband"]
    errs = []
    for t in range(fr.shape[0] - 1):
        e, noc, warped = _pair(fr[t], fr[t + 1], fw[t], bw[t], geometry)
        want, e64 = gw[k + "warped"][t], gw[k + "warped_e64"][t].astype(np.float64)
        d = np.abs(warped.astype(np.float64) - want)
        assert (d <= 2e-6 + 2.0 * e64).all(), (t, d.max(), float(e64.max()))
        out_band = (np.abs(gw[k + "m1"][t]) >= b1) & (np.abs(gw[k + "m2"][t]) >= b2)
        assert np.array_equal(noc[out_band], gw[k + "noc"][t][out_band].astype(np.float32)), t
        assert set(np.unique(noc)) <= {0.0, 1.0}
        assert 0 < noc.sum() < noc.size
        want_e = gw[k + "err"][t]
        assert abs(e - want_e) <= ERR_RTOL * want_e, (t, e, want_e, abs(e - want_e) / want_e)
        errs.append(abs(e - want_e) / want_e)
    print("shape %d geometry %d: max relative E error %.3g" % (shape, geometry, max(errs)))


def test_identities(gw):
    fr = gw["s0_frames"]
    H, W = fr.shape[1:3]
    z = np.zeros((H, W, 2), np.float32)
    e, noc, warped = _pair(fr[0], fr[1], z, z, 1)
    assert (noc == 1).all()
    # zero flow, align_corners=1: the sample position is x to within its fp32 rounding, so the weights are 1 / ~1e-7
    assert np.abs(warped - fr[1]).max() <= 4e-7 * max(1.0, float(np.abs(fr[1]).max())) * 8, np.abs(warped - fr[1]).max()
    e_same = _pair(fr[0], fr[0], z, z, 1, maps=False)
    assert 0.0 <= e_same <= 1e-12, e_same
    # fully occluded: flows that fail the forward-backward test everywhere -> E = 0, finite
    big = np.full((H, W, 2), 5.0, np.float32)
    e_occ, noc_occ, _ = _pair(fr[0], fr[1], big, big, 1)
    assert (noc_occ == 0).all() and e_occ == 0.0 and np.isfinite(e_occ)
    # reference geometry resamples even at zero flow
    _, _, w0 = _pair(fr[0], fr[1], z, z, 0)
    assert np.abs(w0 - fr[1]).max() > 1e-2


def test_repeat_and_device_pointers_bitwise(gw):
    fr, fw, bw = gw["s0_frames"], gw["s0_fw"], gw["s0_bw"]
    for g in (0, 1):
        a = _pair(fr[1], fr[2], fw[1], bw[1], g)
        b = _pair(fr[1], fr[2], fw[1], bw[1], g)
        dev = [torch.from_numpy(x).cuda() for x in (fr[1], fr[2], fw[1], bw[1])]
        c = _pair(*dev, g)
        assert a[0] == b[0] == c[0], (a[0], b[0], c[0])
        for x, y in ((a[1], b[1]), (a[2], b[2]), (a[1], c[1].cpu().numpy()), (a[2], c[2].cpu().numpy())):
            assert np.array_equal(x, y)
        assert _pair(*dev, g, maps=False) == a[0]


def test_pair_error_paths(gw):
    import aiod_amd
    lib = aiod_amd.load_library()
    fr, fw, bw = gw["s1_frames"], gw["s1_fw"], gw["s1_bw"]
    H, W = fr.shape[1:3]
    i1, i2, f12, f21 = (np.ascontiguousarray(x) for x in (fr[0], fr[1], fw[0], bw[0]))
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    err = C.c_double(-1)
    ok = [p(i1), p(i2), p(f12), p(f21)]
    assert lib.af_warp_error_pair(0, *ok, H, W, 1, C.byref(err), None, None, 0) == 0 and err.value > 0
    for hh, ww in ((1, W), (H, 1), (0, W)):
        assert lib.af_warp_error_pair(0, *ok, hh, ww, 1, C.byref(err), None, None, 0) == AF_EINVAL, (hh, ww)
    for i in range(4):
        args = list(ok)
        args[i] = None
        assert lib.af_warp_error_pair(0, *args, H, W, 1, C.byref(err), None, None, 0) == AF_EINVAL, i
    for ac in (-1, 2):
        assert lib.af_warp_error_pair(0, *ok, H, W, ac, C.byref(err), None, None, 0) == AF_EINVAL, ac
    with pytest.raises(aiod_amd.AtlasFitError) as e:
        aiod_amd.warp_error_pair(fr[0][:1], fr[1][:1], fw[0][:1], bw[0][:1])
    assert e.value.code == AF_EINVAL
    with pytest.raises(ValueError):
        aiod_amd.warp_error_pair(fr[0], fr[1], fw[0][:, :-1], bw[0])


# ---- handle path: the nets and videos of tests/test_gpu_loss_maps.py
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


def _single_handle(golden, video, mode=3, upload=True):
    import aiod_amd
    from aiod_amd import stage1 as S
    af = aiod_amd.AtlasFit(aiod_amd.default_config(video.resx, video.resy, video.F, golden["config"]))
    if upload:
        af.upload_video(video.video_frames, video.optical_flows, video.optical_flows_reverse, video.optical_flows_mask,
                        video.optical_flows_reverse_mask)
    S.load_checkpoint(af, os.path.join(GOLDEN, "ckpt_single.pt"))
    af.set_mlp_mode(mode)
    return af


def _arrays(video):
    fr = video.video_frames.numpy()
    ff = video.optical_flows.numpy().reshape(video.resy, video.resx, 2, video.F)
    fb = video.optical_flows_reverse.numpy().reshape(video.resy, video.resx, 2, video.F)
    return fr, ff, fb


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", ["seg", "single"])
def test_handle_matches_pair_calls(path, mode, golden, golden_seg, small_video, small_seg_video):
    v = small_seg_video if path == "seg" else small_video
    af = _seg_handle(golden_seg, v, mode) if path == "seg" else _single_handle(golden, v, mode)
    fr, ff, fb = _arrays(v)
    _, psnr0 = af.psnr()
    for align in (True, False):
        m_in, per_in = af.warp_error("input", align)
        m_rec, per_rec = af.warp_error("reconstruction", align)
        assert per_in.shape == per_rec.shape == (v.F - 1,)
        rgb = [af.render_frame(f)[0] for f in range(v.F)]
        for t in range(v.F - 1):
            f12, f21 = np.ascontiguousarray(ff[..., t]), np.ascontiguousarray(fb[..., t + 1])
            e_in = _pair(np.ascontiguousarray(fr[..., t]), np.ascontiguousarray(fr[..., t + 1]), f12, f21, align, maps=False)
            e_rec = _pair(rgb[t], rgb[t + 1], f12, f21, align, maps=False)
            assert per_in[t] == e_in, (t, per_in[t], e_in)
            assert per_rec[t] == e_rec, (t, per_rec[t], e_rec)
        assert m_in == sum(per_in.tolist()) / (v.F - 1) and m_rec == sum(per_rec.tolist()) / (v.F - 1)
        assert np.isfinite(per_rec).all() and (per_in > 0).all()
        assert af.warp_error("reconstruction", align)[0] == m_rec
    assert np.array_equal(af.psnr()[1], psnr0)          # af_psnr's cache does not move
    af.close()


@pytest.mark.parametrize("path", ["seg", "single"])
def test_call_between_train_blocks_changes_nothing(path, golden, golden_seg, small_video, small_seg_video):
    import aiod_amd
    v = small_seg_video if path == "seg" else small_video
    af = _seg_handle(golden_seg, v) if path == "seg" else _single_handle(golden, v)
    start = {n: af.get_params_flat(n) for n in ((aiod_amd.NET_MAPPING1, aiod_amd.NET_MAPPING2, aiod_amd.NET_ATLAS, aiod_amd.NET_ALPHA)
                                                 if path == "seg" else (aiod_amd.NET_MAPPING1, aiod_amd.NET_ATLAS))}
    outs = []
    for call in (False, True):
        for net, flat in start.items():
            af.lib.af_set_params(af.h, net, flat.ctypes.data_as(C.c_void_p), flat.size)
            z = np.zeros(flat.size, np.float32)
            af.set_adam_state(net, z, z, 0)
        first = af.train_steps(0, 3, None, seed=7)
        psnr = af.psnr()[1]
        if call:
            af.warp_error("input")
            af.warp_error("reconstruction")
            assert np.array_equal(af.psnr()[1], psnr)
        outs.append((first, af.train_steps(3, 3, None, seed=7)))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1]), (outs[0][1], outs[1][1])
    af.close()


def test_handle_error_paths(golden, golden_seg, small_video, small_seg_video):
    import aiod_amd
    af = _single_handle(golden, small_video)
    mean = C.c_double(0)
    for which, ac in ((-1, 1), (2, 1), (0, -1), (1, 2)):
        assert af.lib.af_warp_error(af.h, which, ac, None, C.byref(mean)) == AF_EINVAL, (which, ac)
    assert af.lib.af_warp_error(None, 0, 1, None, None) == AF_EINVAL
    assert af.lib.af_warp_error(af.h, 0, 1, None, None) == 0          # NULL outputs are fine
    with pytest.raises(ValueError):
        af.warp_error("stage_2")
    af.close()
    for nov in (_single_handle(golden, small_video, upload=False), _seg_handle(golden_seg, small_seg_video, upload=False)):
        assert nov.lib.af_warp_error(nov.h, 0, 1, None, C.byref(mean)) == AF_ESTATE
        with pytest.raises(aiod_amd.AtlasFitError) as e:
            nov.warp_error("reconstruction")
        assert e.value.code == AF_ESTATE
        nov.close()
    # a one-frame clip has no pair (checked before the upload state)
    one = aiod_amd.AtlasFit(aiod_amd.default_config(small_video.resx, small_video.resy, 1, golden["config"]))
    assert one.lib.af_warp_error(one.h, 0, 1, None, C.byref(mean)) == AF_EINVAL
    one.close()


# ---- CLIs
def _write_png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(str(path))


def test_warp_error_cli_matches_pair_calls(tmp_path, gw):
    """warp_error.py on a synthetic clip whose flows are stored at a different resolution equals direct pair calls on the resized flows."""
    import aiod_amd
    from aiod_amd.atlasfit import resize_bilinear_device
    fr, fw, bw = gw["s0_frames"], gw["s0_fw"], gw["s0_bw"]          # 37x53 frames; the flows are stored at 18x26 (resized down here)
    F, H, W = fr.shape[:3]
    root, results, vid = tmp_path / "data", tmp_path / "results", "clip"
    (root / vid).mkdir(parents=True)
    (root / (vid + "_flow")).mkdir()
    names = ["%05d.png" % i for i in range(F)]
    u8 = [np.clip(fr[i] * 200, 0, 255).astype(np.uint8) for i in range(F)]
    for n, im in zip(names, u8):
        _write_png(root / vid / n, im)
    stage = results / vid / "stage_1" / "output"
    stage.mkdir(parents=True)
    u8b = [np.ascontiguousarray(im[::2, ::2]) for im in u8[:F - 1]]     # a stage at another resolution and with one frame fewer
    for i, im in enumerate(u8b):
        _write_png(stage / ("%05d.png" % i), im)
    fh, fwd = 18, 26
    small = []
    for t in range(F - 1):
        f12 = fw[t][::2, ::2][:fh, :fwd] * 0.5
        f21 = bw[t][::2, ::2][:fh, :fwd] * 0.5
        np.save(root / (vid + "_flow") / ("%s_%s.npy" % (names[t], names[t + 1])), f12)
        np.save(root / (vid + "_flow") / ("%s_%s.npy" % (names[t + 1], names[t])), f21)
        small.append((np.ascontiguousarray(f12), np.ascontiguousarray(f21)))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "all-in-one-deflicker_amd", "warp_error.py"), "--vid_name", vid, "--root", str(root),
                        "--results", str(results)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    rep = json.load(open(results / vid / "warp_error.json"))
    assert rep["geometry"] == "exact" and rep["align_corners"] == 1 and sorted(rep["sequences"]) == ["input", "stage_1"]

    def resized(f, h, w):
        src = torch.from_numpy(f).cuda()
        dst = torch.empty((h, w, 2), device="cuda")
        resize_bilinear_device(src, dst, h, w, 2, 1, 0, scale=(h / f.shape[0], w / f.shape[1]))
        return dst

    for stage_name, ims in (("input", u8), ("stage_1", u8b)):
        h, w = ims[0].shape[:2]
        frames = [torch.from_numpy(np.float32(im) / 255.0).cuda() for im in ims]
        want = [aiod_amd.warp_error_pair(frames[t], frames[t + 1], resized(small[t][0], h, w), resized(small[t][1], h, w))
                for t in range(len(ims) - 1)]
        got = rep["sequences"][stage_name]
        assert (got["height"], got["width"], got["frames"]) == (h, w, len(ims))
        assert got["per_pair"] == want, (stage_name, got["per_pair"], want)
        assert got["mean"] == float(np.mean(want))
    assert "input" in r.stdout and "stage_1" in r.stdout


def test_stage1_warp_error_flag(tmp_path, golden, small_video):
    """--warp_error's evaluation hook writes <iter>/warp_error.json from the handle; without it the evaluation folder is unchanged."""
    from aiod_amd import stage1 as S
    af = _single_handle(golden, small_video)
    trees = []
    for flag in (None, True, False):
        out = tmp_path / ("run_%s" % flag)
        S.evaluate_model_single(af, small_video.video_frames.numpy(), out, 2, save_checkpoint_file=False, warp_error=flag)
        trees.append(sorted(str(p.relative_to(out)) for p in out.rglob("*")))
        if flag is not None:
            rec = json.load(open(out / "000002" / "warp_error.json"))
            assert rec["geometry"] == ("exact" if flag else "reference") and rec["align_corners"] == int(flag)
            for which in ("input", "reconstruction"):
                mean, per = af.warp_error(which, flag)
                assert rec[which]["mean"] == mean and rec[which]["per_pair"] == per.tolist()
    assert "000002/warp_error.json" not in trees[0]
    assert trees[1] == sorted(trees[0] + ["000002/warp_error.json"]) == trees[2]
    af.close()
