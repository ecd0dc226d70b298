"""af_render_layers_at and the edit sessions on the GPU (include/atlasfit.h): the layer decomposition and the texture-edit propagation on a
grid other than the stage-1 lattice, with the textures and usage masks of a session resident on the device.  The 40x24x6 clips of
conftest.py in two states: the oracle's start models (the arrangement of tests/test_gpu_render_at.py) and the nets of ckpt_seg.pt with the
scaled alpha layer (the arrangement of tests/test_gpu_atlas_outputs.py, restated here).  Same-size and coinciding pixels are held bit for
bit against af_render_layers / af_render_edit; other sizes against the oracle's models at the restated coordinates (tests/layers_at_ref.py)
and against the reference's get_colors restated on the library's own uv and alpha."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
import layers_at_ref as LR  # noqa: E402
import render_at_ref as R  # noqa: E402

SIZES = [(41, 67), (72, 120), (12, 20)]      # non-integer factors and a ragged last tile; k = 3 in nine bands; a down-scale
LAYERS = ("uv1", "uv2", "alpha", "rgb1", "rgb2")
EDITS = ("edit", "edit_fg", "edit_bg")
FG_NARROW = (0.4919348, 0.5084051, 0.0042198)      # case (b): a window a tenth of the fg mapping's range


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a) if a.dtype == np.float32 else a, _bits(b) if b.dtype == np.float32 else b)


def _to_u8(x):
    return (np.asarray(x, np.float64) * 255).astype(np.uint8)


def _nets(two_layer):
    import aiod_amd
    return (aiod_amd.NET_MAPPING1, aiod_amd.NET_MAPPING2, aiod_amd.NET_ATLAS, aiod_amd.NET_ALPHA) if two_layer else (aiod_amd.NET_MAPPING1, aiod_amd.NET_ATLAS)


def _frames(v):
    return (0, v.F // 2, v.F - 1)


# ---- the two states ----------------------------------------------------------------------------------------------------------------
def _start_models(g, two_layer):
    if two_layer:
        from conftest import seg_start_models
        return list(seg_start_models(g))
    from test_gpu_parity import _oracle_models
    return list(_oracle_models(g))


def _start_handle(g, v, two_layer, models, upload=True):
    import aiod_amd
    h = aiod_amd.AtlasFit(aiod_amd.default_config(int(g["resx"]), int(g["resy"]), int(g["nframes"]), dict(g["config"]), two_layer=two_layer))
    if upload:
        h.upload_video(v.video_frames, v.optical_flows, v.optical_flows_reverse, v.optical_flows_mask, v.optical_flows_reverse_mask,
                       *((v.mask_frames,) if two_layer else ()))
    for net, m in zip(_nets(two_layer), models):
        h.load_state_dict(net, m.state_dict())
    return h


def _ckpt_handle(golden_seg, video, ga, upload=True):
    """Two-layer handle with the nets of ckpt_seg.pt, the alpha net's output layer rescaled as the fixture generator does (w * s,
    (b - c) * s in fp32): alpha spans its range."""
    import aiod_amd
    ck = torch.load(os.path.join(GOLDEN, "ckpt_seg.pt"), map_location="cpu", weights_only=False)
    af = aiod_amd.AtlasFit(aiod_amd.default_config(video.resx, video.resy, video.F, golden_seg["config"], two_layer=True))
    if upload:
        af.upload_video(video.video_frames, video.optical_flows, video.optical_flows_reverse, video.optical_flows_mask, video.optical_flows_reverse_mask,
                        video.mask_frames)
    sd_al = {k: t.clone() for k, t in ck["model_F_alpha_state_dict"].items()}
    last = max(int(k.split(".")[1]) for k in sd_al)
    s, c = torch.tensor(float(ga["alpha_scale"])), torch.tensor(float(ga["alpha_centre"]))
    sd_al["hidden.%d.weight" % last] = sd_al["hidden.%d.weight" % last] * s
    sd_al["hidden.%d.bias" % last] = (sd_al["hidden.%d.bias" % last] - c) * s
    af.load_state_dict(aiod_amd.NET_MAPPING1, ck["model_F_mapping1_state_dict"])
    af.load_state_dict(aiod_amd.NET_MAPPING2, ck["model_F_mapping2_state_dict"])
    af.load_state_dict(aiod_amd.NET_ATLAS, ck["F_atlas_state_dict"])
    af.load_state_dict(aiod_amd.NET_ALPHA, sd_al)
    return af


def _textures(ga, res):
    """The synthetic texture pair of tools/make_golden_atlas.py (edit_textures) at side `res`, from the parameters recorded in the fixture."""
    y, x = np.mgrid[0:res, 0:res].astype(np.float64)
    out = []
    for L in range(2):
        t = np.stack([0.5 + 0.4 * np.sin(2 * np.pi * (ga["edit_freq"][L, 0] * x + ga["edit_freq"][L, 1] * y) / res + ga["edit_phase"][L, c]) for c in range(3)], axis=2)
        out.append(t.astype(np.float32))
    return out


@pytest.fixture(scope="module")
def ga():
    return dict(np.load(os.path.join(GOLDEN, "atlas_seg.npz")))


@pytest.fixture(scope="module")
def start(golden, small_video, golden_seg, small_seg_video):
    """{name: (handle, fixture, video, two_layer, oracle models)} with the oracle's start state loaded."""
    out = {}
    for name, g, v, two in (("single", golden, small_video, False), ("seg", golden_seg, small_seg_video, True)):
        models = _start_models(g, two)
        out[name] = (_start_handle(g, v, two, models), g, v, two, models)
    yield out
    for c in out.values():
        c[0].close()


@pytest.fixture(scope="module")
def ckpt(ga, golden_seg, small_seg_video):
    """(handle, video, case (a): (res, textures, fg window, bg window) of the fixture, case (b): the res 64 pair with the narrowed windows,
    case (s): the res 64 pair with the unit windows the start state's pre-trained mappings (uv = 0.8 xy) fall into)."""
    af = _ckpt_handle(golden_seg, small_seg_video, ga)
    area = ga["area_bg_scaled"]
    res_a = int(ga["edit_res"])
    t1a, t2a = _textures(ga, res_a)
    t1b, t2b = _textures(ga, 64)
    case_a = (res_a, t1a, t2a, (0.0, 0.0, 1.0), (area[1], area[3], area[4]))
    case_b = (64, t1b, t2b, FG_NARROW, (area[1], area[3], np.float32(area[4]) / np.float32(2)))
    case_s = (64, t1b, t2b, (0.0, 0.0, 1.0), (-1.0, -1.0, 1.0))
    yield af, small_seg_video, case_a, case_b, case_s
    af.close()


@pytest.fixture(params=["single", "seg"])
def case2(request, start):
    return start[request.param]


def _session(af, case, **kw):
    res, t1, t2, win_fg, win_bg = case
    return af.edit_session(res, t1, win_fg, t2, win_bg, **kw)


# ---- 1. identity -------------------------------------------------------------------------------------------------------------------
def _check_layers_identity(h, v, two, frames):
    for f in frames:
        want = h.render_layers(f)
        got = h.render_layers_at(f, v.resy, v.resx, alpha_u8=True)
        names = LAYERS if two else ("uv1", "alpha", "rgb1")
        assert set(got) == set(names) | {"alpha_u8"}
        for k in names:
            assert _same(got[k], want[k]), (f, k, float(np.abs(got[k] - want[k]).max()))
        assert _same(got["alpha_u8"], _to_u8(want["alpha"]))
        if not two:
            assert (got["alpha"] == 1).all() and (got["alpha_u8"] == 255).all()


def test_same_size_layers_are_render_layers_bit_for_bit(case2):
    """af_render_layers is af_render_layers_at's core at (resy, resx): one kernel, two entry points, the same bits."""
    h, g, v, two, _ = case2
    _check_layers_identity(h, v, two, _frames(v))


def _check_edit_identity(af, v, case, frames):
    res, t1, t2, win_fg, win_bg = case
    u1, u2 = np.zeros((res, res), np.float32), np.zeros((res, res), np.float32)
    with _session(af, case, track_usage=True) as s:
        for f in frames:
            want = af.render_edit(f, res, t1, win_fg, t2, win_bg, use_fg=u1, use_bg=u2)
            got = s.frame(f, outputs=EDITS, u8=True)
            for k in EDITS:
                assert got[k].shape == (v.resy, v.resx, 3) and _same(got[k], want[k]), (f, k, float(np.abs(got[k] - want[k]).max()))
            assert _same(got["edit_u8"], _to_u8(want["edit"]))
        g1, g2 = s.usage()
    assert u1.max() > 0 and u2.max() == 1
    assert _same(g1, u1) and _same(g2, u2)


def test_same_size_on_the_ckpt_state_layers_edit_and_usage(ckpt):
    """One k_layer_finish and one k_edit through two host routes each: af_render_edit's textures and masks uploaded per call against a
    session's resident ones, host staging in both; colours, bytes and usage masks agree bit for bit."""
    af, v, case_a, case_b, _ = ckpt
    _check_layers_identity(af, v, True, _frames(v))
    _check_edit_identity(af, v, case_a, range(v.F))
    _check_edit_identity(af, v, case_b, range(v.F))


def test_same_size_edit_on_the_start_state(start, ckpt):
    """As test_same_size_on_the_ckpt_state_layers_edit_and_usage's edit part, on the start state: one kernel, two host routes."""
    h, g, v, two, _ = start["seg"]
    _check_edit_identity(h, v, ckpt[4], _frames(v))


# ---- 2. coinciding pixels, 3. borders ----------------------------------------------------------------------------------------------
def _sub3(a):
    return np.ascontiguousarray(a[1::3, 1::3])


def test_odd_factor_hits_the_lattice_pixels_bit_for_bit(case2):
    """k = 3: output pixel 3i + 1 has lattice pixel i's coordinate exactly; nine bands, the lattice pixels spread over all of them."""
    h, g, v, two, _ = case2
    for f in _frames(v):
        want = h.render_layers(f)
        got = h.render_layers_at(f, 3 * v.resy, 3 * v.resx, alpha_u8=True)
        for k in (LAYERS if two else ("uv1", "alpha", "rgb1")):
            assert _same(_sub3(got[k]), want[k]), (f, k)
        assert _same(_sub3(got["alpha_u8"]), _to_u8(want["alpha"]))


def test_odd_factor_edit_hits_the_lattice_pixels_bit_for_bit(ckpt):
    af, v, case_a, case_b, _ = ckpt
    for case in (case_a, case_b):
        res, t1, t2, win_fg, win_bg = case
        with _session(af, case) as s:
            for f in _frames(v):
                want = af.render_edit(f, res, t1, win_fg, t2, win_bg)
                got = s.frame(f, 3 * v.resy, 3 * v.resx, outputs=EDITS, u8=True)
                for k in EDITS:
                    assert _same(_sub3(got[k]), want[k]), (f, k)
                assert _same(_sub3(got["edit_u8"]), _to_u8(want["edit"]))
        for f in _frames(v):
            want = af.render_layers(f)
            got = af.render_layers_at(f, 3 * v.resy, 3 * v.resx)
            for k in LAYERS:
                assert _same(_sub3(got[k]), want[k]), (f, k)


def test_border_pixels_are_clamped_to_the_lattice(case2, ckpt):
    for h, v in ((case2[0], case2[2]), (ckpt[0], ckpt[1])):
        L = h.render_layers_at(v.F // 2, 3 * v.resy, 3 * v.resx, which=("uv1", "alpha"))
        for k in ("uv1", "alpha"):
            a = _bits(L[k])
            assert np.array_equal(a[:, 0], a[:, 1]) and np.array_equal(a[:, -1], a[:, -2]), k
            assert np.array_equal(a[0], a[1]) and np.array_equal(a[-1], a[-2]), k
        assert not np.array_equal(_bits(L["uv1"])[:, 1], _bits(L["uv1"])[:, 2])


# ---- 4. oracle ---------------------------------------------------------------------------------------------------------------------
def test_layers_match_the_oracle_at_the_restated_coordinates(case2):
    """Every output, size and frame: no further from the fp64 twin of the oracle's models (on the unrounded positions) than
    max(2e-6, 2 e_ref), e_ref the oracle's own fp32 values against that twin on the same grid."""
    h, g, v, two, models = case2
    twins = R.fp64_twin(models)
    names = LAYERS if two else ("uv1", "rgb1")
    bad = []
    for oh, ow in SIZES:
        for f in _frames(v):
            want, want64 = LR.layers_pair(models, twins, v.resx, v.resy, oh, ow, f, v.F)
            got = h.render_layers_at(f, oh, ow, which=names)
            for k in names:
                assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
                d, e_ref, e_hip = float(np.abs(got[k] - want[k]).max()), float(np.abs(want[k] - want64[k]).max()), float(np.abs(got[k] - want64[k]).max())
                print("%dx%d frame %d %s: vs fp32 oracle %.3g, oracle vs twin %.3g, hip vs twin %.3g" % (ow, oh, f, k, d, e_ref, e_hip))
                if not e_hip <= max(2e-6, 2.0 * e_ref):
                    bad.append((oh, ow, f, k, d, e_hip, e_ref))
    assert not bad, bad


# ---- 5. compose --------------------------------------------------------------------------------------------------------------------
def test_layers_compose_to_render_frame_at(start, ckpt):
    """render_frame_at's rgb is the finish kernel's written-out blend of render_layers_at's values at the same size, bit for bit: the
    criterion of test_layers_compose_to_render_frame_and_leave_psnr_alone (tests/blend_ref.py), at 41x67 and at the lattice."""
    from blend_ref import check_composes
    for name, h, v in (("start", start["seg"][0], start["seg"][2]), ("ckpt", ckpt[0], ckpt[1])):
        for oh, ow in ((41, 67), (v.resy, v.resx)):
            for f in _frames(v):
                check_composes(h.render_frame_at(f, oh, ow), h.render_layers_at(f, oh, ow), "%s state, %dx%d, frame %d" % (name, ow, oh, f))


# ---- 6. edit against the restated get_colors ---------------------------------------------------------------------------------------
def _check_edit_against_get_colors(af, v, case, narrowed):
    res, t1, t2, win_fg, win_bg = case
    with _session(af, case, track_usage=True) as s:
        for oh, ow in [(v.resy, v.resx)] + SIZES:
            s.reset_usage()
            m1, m2 = np.zeros((res, res)), np.zeros((res, res))
            n_fg = n_bg = 0
            worst = 0.0
            for f in _frames(v):
                got = s.frame(f, oh, ow, outputs=EDITS)
                L = af.render_layers_at(f, oh, ow, which=("uv1", "uv2", "alpha"))
                want, (r1, r2), add_usage = LR.edit_of(res, win_fg, win_bg, t1, t2, L["uv1"].reshape(-1, 2), L["uv2"].reshape(-1, 2), L["alpha"].reshape(-1))
                n_fg += r1; n_bg += r2
                for k, w in zip(EDITS, want):
                    d = float(np.abs(got[k].reshape(-1, 3) - w).max())
                    worst = max(worst, d)
                    assert d <= 1e-6, (oh, ow, f, k, d)
                add_usage(m1, m2)
            u1, u2 = s.usage()
            share = (n_fg / (3.0 * oh * ow), n_bg / (3.0 * oh * ow))
            print("res %d at %dx%d: relevant fg %.1f %%, bg %.1f %%, worst edit error %.3g" % (res, ow, oh, 100 * share[0], 100 * share[1], worst))
            assert _same(u1, m1.astype(np.float32)) and _same(u2, m2.astype(np.float32)), (oh, ow)
            if narrowed:      # the "not relevant" branch and the zero fill run, and so does the relevant one
                assert 0.05 <= share[0] <= 0.5 and 0.05 <= share[1] <= 0.5, (oh, ow, share)
            else:
                assert share[0] > 0.99 and share[1] > 0.99, (oh, ow, share)


def test_edit_matches_get_colors_with_the_fixture_windows(ckpt):
    af, v, case_a, _, _ = ckpt
    _check_edit_against_get_colors(af, v, case_a, narrowed=False)


def test_edit_matches_get_colors_with_narrowed_windows(ckpt):
    af, v, _, case_b, _ = ckpt
    _check_edit_against_get_colors(af, v, case_b, narrowed=True)


# ---- 7. plumbing -------------------------------------------------------------------------------------------------------------------
def test_device_pointers_repeats_and_null_subsets(ckpt):
    af, v, _, case_b, _ = ckpt
    res, t1, t2, win_fg, win_bg = case_b
    f = v.F - 1
    for oh, ow in ((41, 67), (72, 120)):
        L = af.render_layers_at(f, oh, ow, alpha_u8=True)
        D = af.render_layers_at_device(f, oh, ow, alpha_u8=True)
        L2 = af.render_layers_at(f, oh, ow, alpha_u8=True)
        for k in LAYERS + ("alpha_u8",):
            assert D[k].is_cuda and _same(D[k].cpu().numpy(), L[k]) and _same(L2[k], L[k]), (oh, ow, k)
        assert _same(L["alpha_u8"], _to_u8(L["alpha"]))
        only = af.render_layers_at(f, oh, ow, which=("alpha",))
        assert set(only) == {"alpha"} and _same(only["alpha"], L["alpha"])
        only = af.render_layers_at_device(f, oh, ow, which=("rgb2", "uv1"))
        assert set(only) == {"rgb2", "uv1"} and _same(only["rgb2"].cpu().numpy(), L["rgb2"]) and _same(only["uv1"].cpu().numpy(), L["uv1"])
        only = af.render_layers_at(f, oh, ow, which=(), alpha_u8=True)
        assert set(only) == {"alpha_u8"} and _same(only["alpha_u8"], L["alpha_u8"])
        with _session(af, case_b, track_usage=True) as s:
            E = s.frame(f, oh, ow, outputs=EDITS, u8=True)
            use1 = s.usage()
            Dv = s.frame_device(f, oh, ow, outputs=EDITS, u8=True)
            E2 = s.frame(f, oh, ow, outputs=EDITS, u8=True)
            for k in EDITS + ("edit_u8",):
                assert Dv[k].is_cuda and _same(Dv[k].cpu().numpy(), E[k]) and _same(E2[k], E[k]), (oh, ow, k)
            assert _same(E["edit_u8"], _to_u8(E["edit"]))
            assert all(_same(a, b) for a, b in zip(s.usage(), use1))             # max and set-to-1: the same frame again changes nothing
            assert _same(s.frame(f, oh, ow, outputs=("edit_bg",))["edit_bg"], E["edit_bg"])
            only = s.frame(f, oh, ow, outputs=(), u8=True)
            assert set(only) == {"edit_u8"} and _same(only["edit_u8"], E["edit_u8"])
            s.reset_usage()
            assert all((u == 0).all() for u in s.usage())
            s.frame(f, oh, ow, outputs=())                                        # usage tracking alone is something to do
            assert all(_same(a, b) for a, b in zip(s.usage(), use1))
        with af.edit_session(res, None, win_fg, None, win_bg, track_usage=True) as s:      # windows without textures: usage masks only
            assert s.frame(f, oh, ow, outputs=()) == {}
            assert all(_same(a, b) for a, b in zip(s.usage(), use1))
        with af.edit_session(res, t1, win_fg) as s:                                         # one layer: the other is skipped
            one = s.frame(f, oh, ow, outputs=("edit", "edit_fg"))
            assert _same(one["edit_fg"], E["edit_fg"]) and _same(one["edit"], E["edit_fg"])
    with af.edit_session(res, t1, win_fg) as s:       # the one-layer session at the lattice is render_edit with the same arguments
        assert _same(s.frame(f)["edit"], af.render_edit(f, res, t1, win_fg, None, None, outputs=("edit",))["edit"])


def test_a_session_survives_every_mlp_mode(ckpt):
    af, v, _, case_b, _ = ckpt
    res, t1, t2, win_fg, win_bg = case_b
    begin = af.arithmetic["mlp_mode"]
    seen = []
    try:
        with _session(af, case_b, track_usage=True) as s:
            for mode in (0, 1, 2, 3):
                af.set_mlp_mode(mode)
                _check_layers_identity(af, v, True, (1,))
                s.reset_usage()
                u1, u2 = np.zeros((res, res), np.float32), np.zeros((res, res), np.float32)
                want = af.render_edit(1, res, t1, win_fg, t2, win_bg, use_fg=u1, use_bg=u2)
                got = s.frame(1, outputs=EDITS)
                assert all(_same(got[k], want[k]) for k in EDITS), mode
                assert all(_same(a, b) for a, b in zip(s.usage(), (u1, u2))), mode
                assert _same(_sub3(s.frame(1, 3 * v.resy, 3 * v.resx)["edit"]), want["edit"]), mode
                seen.append(want["edit"])
    finally:
        af.set_mlp_mode(begin)
    assert not _same(seen[0], seen[3])       # the modes are different arithmetic: the session followed the handle


def test_a_session_uses_the_nets_of_each_call(start, ckpt):
    _, g, v, two, models = start["seg"]
    case_b = ckpt[4]
    h = _start_handle(g, v, True, models)
    try:
        old = _session(h, case_b)
        before = old.frame(1, 41, 67)["edit"]
        h.train_steps(0, 2, g["inds"][:2].astype(np.int64))
        after = old.frame(1, 41, 67)["edit"]
        with _session(h, case_b) as fresh:
            assert _same(fresh.frame(1, 41, 67)["edit"], after)
        assert not _same(before, after)
        old.close()
    finally:
        h.close()


# ---- 8. forward-only, 9. no video ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["single", "seg"])
def test_forward_only(name, start, ckpt):
    """af_psnr and a following train_steps trajectory are bitwise what they are without the calls in between."""
    _, g, v, two, models = start[name]
    case_b = ckpt[4]
    inds = g["inds"][:3].astype(np.int64)
    runs = []
    for with_calls in (False, True):
        h = _start_handle(g, v, two, models)
        try:
            s = _session(h, case_b, track_usage=True) if (with_calls and two) else None
            if with_calls:
                h.render_layers_at(0, 41, 67, alpha_u8=True)      # before af_psnr has cached anything
                if s:
                    s.frame(0, 41, 67, u8=True)
            mean, per = h.psnr()
            if with_calls:
                h.render_layers_at(2, 72, 120)
                if s:
                    s.frame(2, 72, 120, outputs=EDITS)
            l1 = h.train_steps(0, 2, inds[:2])
            if with_calls:
                h.render_layers_at_device(1, 12, 20, which=("alpha",))
                if s:
                    s.frame_device(1, 12, 20)
                    s.usage()
            l2 = h.train_steps(2, 1, inds[2:])
            params = [h.get_params_flat(n) for n in _nets(two)]
            adam = [h.adam_state(n) for n in _nets(two)]
            runs.append((mean, per, l1, l2, params, adam, h.psnr()[1]))
        finally:
            h.close()
    a, b = runs
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[6], b[6])
    assert np.array_equal(_bits(a[2]), _bits(b[2])) and np.array_equal(_bits(a[3]), _bits(b[3]))
    for p, q in zip(a[4], b[4]):
        assert np.array_equal(_bits(p), _bits(q))
    for (m0, v0, s0), (m1, v1, s1) in zip(a[5], b[5]):
        assert s0 == s1 and np.array_equal(_bits(m0), _bits(m1)) and np.array_equal(_bits(v0), _bits(v1))


@pytest.mark.parametrize("name", ["single", "seg"])
def test_needs_no_video(name, start, ckpt):
    ref_h, g, v, two, models = start[name]
    h = _start_handle(g, v, two, models, upload=False)
    try:
        got, want = h.render_layers_at(2, 41, 67, alpha_u8=True), ref_h.render_layers_at(2, 41, 67, alpha_u8=True)
        assert set(got) == set(want) and all(_same(got[k], want[k]) for k in want)
        if two:
            with _session(h, ckpt[4], track_usage=True) as s, _session(ref_h, ckpt[4], track_usage=True) as s_ref:
                assert _same(s.frame(2, 41, 67)["edit"], s_ref.frame(2, 41, 67)["edit"])
                assert all(_same(x, y) for x, y in zip(s.usage(), s_ref.usage()))
    finally:
        h.close()


# ---- 10. lifetime, 11. invalid arguments -------------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_a_session_outlives_its_handle_safely(start, ckpt):
    import aiod_amd
    _, g, v, two, models = start["seg"]
    case_b = ckpt[4]
    res, t1, t2, win_fg, win_bg = case_b
    h = _start_handle(g, v, True, models, upload=False)
    s = _session(h, case_b, track_usage=True)
    assert s.frame(0)["edit"].shape == (v.resy, v.resx, 3)
    h.close()
    for call in (lambda: s.frame(0), lambda: s.usage(), lambda: s.reset_usage(), lambda: s.frame_device(0)):
        with pytest.raises(aiod_amd.AtlasFitError) as e:
            call()
        assert e.value.code == -5
    s.close(); s.close()
    # the library's own rule, through ctypes: the handle goes first, the session's calls report AF_ESTATE, then its struct is freed
    h = _start_handle(g, v, True, models, upload=False)
    lib = h.lib
    wf, wb = np.asarray(win_fg, np.float32), np.asarray(win_bg, np.float32)
    e = C.c_void_p()
    assert lib.af_edit_create(h.h, res, _p(t1), _p(wf), _p(t2), _p(wb), 1, C.byref(e)) == 0 and e.value
    e2 = C.c_void_p()
    assert lib.af_edit_create(h.h, res, None, _p(wf), None, None, 1, C.byref(e2)) == 0
    out = np.zeros((v.resy, v.resx, 3), np.float32)
    assert lib.af_edit_frame(e, 0, v.resy, v.resx, _p(out), None, None, None, 0) == 0 and np.abs(out).max() > 0
    lib.af_edit_destroy(e2)                  # a session destroyed before its handle
    lib.af_destroy(h.h)
    h.h = None
    use = np.zeros((res, res), np.float32)
    for rc, what in ((lib.af_edit_frame(e, 0, v.resy, v.resx, _p(out), None, None, None, 0), "af_edit_frame"), (lib.af_edit_usage(e, _p(use), None), "af_edit_usage"),
                     (lib.af_edit_reset_usage(e), "af_edit_reset_usage")):
        assert rc == -5, (what, rc)
    assert lib.af_edit_frame(e, 0, v.resy, v.resx, _p(out), None, None, None, 0) == -5
    assert "af_edit_frame" in lib.af_last_error(None).decode() and "destroyed" in lib.af_last_error(None).decode()
    lib.af_edit_destroy(e)
    lib.af_edit_destroy(None)


def test_invalid_arguments(start, ckpt):
    import aiod_amd
    single, seg = start["single"][0], start["seg"][0]
    lib, F = seg.lib, seg.cfg.number_of_frames
    res, t1, t2, win_fg, win_bg = ckpt[3]
    wf, wb = np.asarray(win_fg, np.float32), np.asarray(win_bg, np.float32)
    f4 = np.zeros((4, 4, 3), np.float32); u8 = np.zeros((4, 4, 3), np.uint8)
    msg = lambda h: lib.af_last_error(h.h).decode()      # noqa: E731
    # af_render_layers_at(h, frame, oh, ow, uv1, uv2, alpha, rgb1, rgb2, alpha_u8, on_device)
    bad = [(seg, (F, 4, 4, _p(f4), None, None, None, None, None), "af_render_layers_at: frame index"),
           (seg, (-1, 4, 4, _p(f4), None, None, None, None, None), "af_render_layers_at: frame index"),
           (seg, (0, 0, 4, _p(f4), None, None, None, None, None), "af_render_layers_at: oh and ow must be 1..16384"),
           (seg, (0, 4, 16385, _p(f4), None, None, None, None, None), "af_render_layers_at: oh and ow must be 1..16384"),
           (seg, (0, 4, 4, None, None, None, None, None, None), "af_render_layers_at: every output pointer is NULL"),
           (single, (0, 4, 4, None, _p(f4), None, None, None, None), "af_render_layers_at: uv2 / rgb2 need a two_layer handle"),
           (single, (0, 4, 4, None, None, None, None, _p(f4), None), "af_render_layers_at: uv2 / rgb2 need a two_layer handle")]
    for h, args, want in bad:
        rc = lib.af_render_layers_at(h.h, *args, 0)
        assert rc == -1 and want in msg(h), (args[:3], rc, msg(h))
    assert lib.af_render_layers_at(single.h, 0, 4, 4, None, None, None, None, None, _p(u8), 0) == 0 and (u8.reshape(-1)[:16] == 255).all()
    # af_edit_create(h, res, tex_fg, win_fg, tex_bg, win_bg, track_usage, out)
    e = C.c_void_p()
    bad = [((res, _p(t1), None, None, _p(wb), 0), -1, "af_edit_create: a layer's texture without its window"),
           ((res, None, _p(wf), _p(t2), None, 0), -1, "af_edit_create: a layer's texture without its window"),
           ((0, _p(t1), _p(wf), None, None, 0), -1, "af_edit_create: res must be 1..16384"),
           ((16385, None, _p(wf), None, None, 1), -1, "af_edit_create: res must be 1..16384"),
           ((res, None, None, None, None, 1), -1, "af_edit_create: no layer has a window")]
    for args, code, want in bad:
        rc = lib.af_edit_create(seg.h, *args, C.byref(e))
        assert rc == code and want in msg(seg) and not e.value, (args[0], rc, msg(seg))
    assert lib.af_edit_create(single.h, res, _p(t1), _p(wf), None, None, 0, C.byref(e)) == -5 and "af_edit_create: needs a two_layer handle" in msg(single)
    assert not e.value
    # af_edit_frame(e, frame, oh, ow, edit, edit_fg, edit_bg, edit_u8, on_device)
    fg_only, usage_only, plain = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.af_edit_create(seg.h, res, _p(t1), _p(wf), None, None, 0, C.byref(fg_only)) == 0
    assert lib.af_edit_create(seg.h, res, _p(t1), _p(wf), None, _p(wb), 1, C.byref(usage_only)) == 0      # the bg layer has a window and no texture
    assert lib.af_edit_create(seg.h, res, _p(t1), _p(wf), _p(t2), _p(wb), 0, C.byref(plain)) == 0
    try:
        bad = [(plain, (F, 4, 4, _p(f4), None, None, None), "af_edit_frame: frame index"),
               (plain, (-1, 4, 4, _p(f4), None, None, None), "af_edit_frame: frame index"),
               (plain, (0, 4, 0, _p(f4), None, None, None), "af_edit_frame: oh and ow must be 1..16384"),
               (plain, (0, 16385, 4, _p(f4), None, None, None), "af_edit_frame: oh and ow must be 1..16384"),
               (plain, (0, 4, 4, None, None, None, None), "af_edit_frame: no output asked for and no usage tracked"),
               (fg_only, (0, 4, 4, None, None, _p(f4), None), "af_edit_frame: edit_fg / edit_bg need that layer's texture"),
               (usage_only, (0, 4, 4, None, None, _p(f4), None), "af_edit_frame: edit_fg / edit_bg need that layer's texture"),
               (usage_only, (0, 4, 4, _p(f4), None, None, None), "af_edit_frame: edit / edit_u8 need the texture of every layer with a window"),
               (usage_only, (0, 4, 4, None, None, None, _p(u8)), "af_edit_frame: edit / edit_u8 need the texture of every layer with a window")]
        for s, args, want in bad:
            rc = lib.af_edit_frame(s, *args, 0)
            assert rc == -1 and want in msg(seg), (args[:3], rc, msg(seg))
        assert lib.af_edit_frame(usage_only, 0, 4, 4, None, _p(f4), None, None, 0) == 0      # the layer that has its texture
        assert lib.af_edit_usage(plain, None, None) == -5 and "af_edit_usage: the session does not track usage" in msg(seg)
        assert lib.af_edit_reset_usage(plain) == -5
        assert lib.af_edit_frame(None, 0, 4, 4, _p(f4), None, None, None, 0) == -1
    finally:
        for s in (fg_only, usage_only, plain):
            lib.af_edit_destroy(s)
    # the binding: library errors are AtlasFitError, shape errors ValueError before the call
    with pytest.raises(aiod_amd.AtlasFitError, match="frame index"):
        seg.render_layers_at(F, 4, 4)
    with pytest.raises(aiod_amd.AtlasFitError, match="oh and ow"):
        seg.render_layers_at(0, 0, 4)
    with pytest.raises(ValueError, match="two_layer"):
        single.render_layers_at(0, 4, 4, which=("uv2",))
    with pytest.raises(ValueError, match=r"\(res, res, 3\)"):
        seg.edit_session(res + 1, t1, win_fg)
    with pytest.raises(aiod_amd.AtlasFitError) as err:
        single.edit_session(res, t1, win_fg)
    assert err.value.code == -5
    assert seg.render_layers_at(0, 1, 1, which=("alpha",))["alpha"].shape == (1, 1)


# ---- 12. the CLIs ------------------------------------------------------------------------------------------------------------------
DOWN = 2      # the lattice is half the decoded frames: "full" is another size than "stage1"


def _png(p):
    from PIL import Image
    return np.array(Image.open(str(p)))


def _pngs(d):
    return {str(p.relative_to(d)): p.read_bytes() for p in sorted(d.rglob("*.png"))}


@pytest.fixture(scope="module")
def clip(tmp_path_factory, small_seg_video):
    import aiod_amd
    from test_stage1_host import _write_masks, _write_video
    d = tmp_path_factory.mktemp("layers_at_cli")
    _write_video(d / "data", small_seg_video, "clip")
    _write_masks(d / "data", small_seg_video, "clip")
    cfg = dict(aiod_amd.atlasfit.REFERENCE_CONFIG)
    cfg.update(samples_batch=256, iters_num=21, evaluate_every=20, pretrain_iter_number=2, stop_global_rigidity=10, stop_bootstrapping_iteration=15)
    (d / "cfg.json").write_text(json.dumps(cfg))
    argv = ["--config", str(d / "cfg.json"), "--vid_name", "clip", "--root", str(d / "data"), "--seed", "5", "--down", str(DOWN), "--atlas_outputs"]
    return d, cfg, argv


def _fit(clip, name, extra, monkeypatch):
    import aiod_amd.stage1 as S
    d, cfg, argv = clip
    (d / name).mkdir()
    monkeypatch.chdir(d / name)
    S._cli(argv + extra, two_layer=True)
    return d / name / "results" / "clip" / "stage_1"


def test_cli_full_size_outputs_and_edit(clip, small_seg_video, monkeypatch):
    """stage1_seg --atlas_outputs --atlas_outputs_size full writes alpha/, uv_1/, uv_2/ at the frames' size with render_layers_at's values
    on the checkpoint's nets; atlas_edit.py --size full writes a session's edit_u8; --size stage1 is a run without the flag."""
    from PIL import Image
    import aiod_amd
    import aiod_amd.stage1 as S
    from aiod_amd import atlas_edit
    from aiod_amd.atlas_outputs import FG_WINDOW, normalize_uv, to_u8
    d, cfg, argv = clip
    v = small_seg_video
    H, W, resy, resx = v.resy, v.resx, v.resy // DOWN, v.resx // DOWN
    res_dir = _fit(clip, "full", ["--atlas_outputs_size", "full"], monkeypatch)
    ev = res_dir / "000020"
    assert json.load(open(res_dir / "config.json"))["atlas_outputs_size"] == "full"
    af = aiod_amd.AtlasFit(aiod_amd.default_config(resx, resy, v.F, cfg, two_layer=True))
    try:
        t = S.load_input_data_device(resy, resx, cfg["maximum_number_of_frames"], d / "data" / "clip", True, d / "data", "clip", with_masks=True)
        af.upload_video(t[1], t[4], t[3], t[0], t[2], t[5])
        assert S.load_checkpoint(af, res_dir / "checkpoint") == 20
        win_bg = af.area_window(af.mapping_area(1))
        names = ["%05d.png" % f for f in range(v.F)]
        for sub in ("alpha", "uv_1", "uv_2"):
            assert sorted(os.listdir(ev / sub)) == names
        for f in range(v.F):
            L = af.render_layers_at(f, H, W, which=("uv1", "uv2"), alpha_u8=True)
            a = _png(ev / "alpha" / names[f])
            assert a.shape == (H, W) and np.array_equal(a, L["alpha_u8"])
            assert np.array_equal(_png(ev / "uv_1" / names[f]), to_u8(normalize_uv(L["uv1"], 0.5, 1, 0, 0)))
            assert np.array_equal(_png(ev / "uv_2" / names[f]), to_u8(normalize_uv(L["uv2"], -0.5, win_bg[2], win_bg[0], win_bg[1])))
        # the unedited textures through atlas_edit.py: the frames are a session's bytes at the asked size
        res = 200
        tex1, tex2 = af.atlas_texture(res, FG_WINDOW), af.atlas_texture(res, win_bg)
        Image.fromarray(to_u8(tex1)).save(str(d / "t1.png")); Image.fromarray(to_u8(tex2)).save(str(d / "t2.png"))
        edit = ["--vid_name", "clip", "--root", str(d / "data"), "--down", str(DOWN), "--edit_fg", str(d / "t1.png"), "--edit_bg", str(d / "t2.png")]
        atlas_edit._cli(edit + ["--size", "full", "--out", str(d / "edit_full")])
        atlas_edit._cli(edit + ["--size", "%dx%d" % (31, 53), "--out", str(d / "edit_hxw")])
        atlas_edit._cli(edit + ["--size", "stage1", "--out", str(d / "edit_stage1")])
        atlas_edit._cli(edit)
        t1r = (_png(d / "t1.png").astype(np.float64) / 255).astype(np.float32)
        t2r = (_png(d / "t2.png").astype(np.float64) / 255).astype(np.float32)
        with af.edit_session(res, t1r, FG_WINDOW, t2r, win_bg) as s:
            for f in range(v.F):
                for sub, (oh, ow) in (("edit_full", (H, W)), ("edit_hxw", (31, 53)), ("edit_stage1", (resy, resx))):
                    out = _png(d / sub / names[f])
                    assert out.shape == (oh, ow, 3) and np.array_equal(out, s.frame(f, oh, ow, outputs=(), u8=True)["edit_u8"]), (sub, f)
                assert np.array_equal(_png(res_dir / "edit" / names[f]), to_u8(af.render_edit(f, res, t1r, FG_WINDOW, t2r, win_bg, outputs=("edit",))["edit"]))
        assert _pngs(d / "edit_stage1") == _pngs(res_dir / "edit") and len(_pngs(res_dir / "edit")) == v.F
    finally:
        af.close()


def test_cli_default_bytes_and_textures(clip, small_seg_video, monkeypatch):
    """--atlas_outputs_size stage1 is a run without the flag, byte for byte; the textures of the full-size run are the same files."""
    d, cfg, argv = clip
    v = small_seg_video
    plain = _fit(clip, "plain", [], monkeypatch)
    flag = _fit(clip, "flag", ["--atlas_outputs_size", "stage1"], monkeypatch)
    a, b = _pngs(plain), _pngs(flag)
    assert a == b and len(a) == 2 + 4 * v.F
    assert (plain / "config.json").read_bytes() == (flag / "config.json").read_bytes() and "atlas_outputs_size" not in json.load(open(plain / "config.json"))
    assert _png(plain / "000020" / "alpha" / "00000.png").shape == (v.resy // DOWN, v.resx // DOWN)
    full = d / "full" / "results" / "clip" / "stage_1"
    if not full.exists():
        full = _fit(clip, "full", ["--atlas_outputs_size", "full"], monkeypatch)
    for t in ("texture_orig1.png", "texture_orig2.png"):
        assert (full / "000020" / t).read_bytes() == (plain / "000020" / t).read_bytes(), t
    for f in range(v.F):
        assert (full / "output" / ("%05d.png" % f)).read_bytes() == (plain / "output" / ("%05d.png" % f)).read_bytes()
