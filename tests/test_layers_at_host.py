"""Host-side pieces of the layer products at any size (atlas_outputs.parse_size / write_atlas_outputs(size=), the CLIs' flags, the
binding's surface): no GPU needed."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_size_parsing():
    from aiod_amd.atlas_outputs import parse_size
    assert parse_size("stage1") is None and parse_size("stage1", full=(7, 9)) is None
    assert parse_size("full", full=(1080, 1920)) == (1080, 1920)
    assert parse_size("41x67") == (41, 67) and parse_size("2160X3840") == (2160, 3840) and parse_size("1x16384") == (1, 16384)
    for bad in ("", "4k", "41", "41x", "x67", "41x67x3", "0x5", "5x0", "16385x4", "-4x4", "4.5x4", "full "):
        with pytest.raises(ValueError):
            parse_size(bad, full=(4, 4))
    with pytest.raises(ValueError):
        parse_size("full")


class _StubAtlas:
    """The AtlasFit surface write_atlas_outputs uses; records every call."""
    two_layer = True

    class cfg:
        number_of_frames, resy, resx = 2, 3, 4

    def __init__(self):
        self.calls = []

    def mapping_area(self, which):
        self.calls.append(("area", which))
        return tuple(np.float32(v) for v in (0.5, -1.0, 0.25, -0.75, 1.5))

    @staticmethod
    def area_window(area):
        return (np.float32(area[1]), np.float32(area[3]), np.float32(area[4]))

    def atlas_texture(self, res, window):
        self.calls.append(("texture", res, tuple(float(w) for w in window)))
        return np.full((res, res, 3), 0.5, np.float32)

    def texture_masks(self, res, win_fg, win_bg):
        self.calls.append(("masks", res))
        return np.ones((res, res), np.float32), np.ones((res, res), np.float32)

    def render_layers(self, f):
        self.calls.append(("layers", f))
        H, W = self.cfg.resy, self.cfg.resx
        return {"uv1": np.zeros((H, W, 2), np.float32), "uv2": np.zeros((H, W, 2), np.float32), "alpha": np.full((H, W), 0.5, np.float32),
                "rgb1": np.zeros((H, W, 3), np.float32), "rgb2": np.zeros((H, W, 3), np.float32)}

    def render_layers_at(self, f, oh, ow, which=("uv1", "uv2", "alpha", "rgb1", "rgb2"), alpha_u8=False):
        self.calls.append(("layers_at", f, oh, ow, tuple(which), alpha_u8))
        out = {"uv1": np.zeros((oh, ow, 2), np.float32), "uv2": np.full((oh, ow, 2), 0.25, np.float32)}
        out = {k: v for k, v in out.items() if k in which}
        if alpha_u8:
            out["alpha_u8"] = np.full((oh, ow), 40 + f, np.uint8)
        return out


def _png(p):
    from PIL import Image
    return np.array(Image.open(str(p)))


def test_write_atlas_outputs_default_makes_todays_calls_and_size_goes_through_layers_at(tmp_path):
    from aiod_amd.atlas_outputs import normalize_uv, to_u8, write_atlas_outputs
    head = [("area", 1), ("texture", 8, (0.0, 0.0, 1.0)), ("texture", 8, (-1.0, -0.75, 1.5)), ("masks", 8)]
    a, b, c = _StubAtlas(), _StubAtlas(), _StubAtlas()
    for d in ("plain", "none", "sized"):
        (tmp_path / d).mkdir()
    win = write_atlas_outputs(a, str(tmp_path / "plain"), res=8)
    assert a.calls == head + [("layers", 0), ("layers", 1)]
    assert write_atlas_outputs(b, str(tmp_path / "none"), res=8, size=None) == win and b.calls == a.calls
    assert write_atlas_outputs(c, str(tmp_path / "sized"), res=8, size=(5, 7)) == win
    assert c.calls == head + [("layers_at", 0, 5, 7, ("uv1", "uv2"), True), ("layers_at", 1, 5, 7, ("uv1", "uv2"), True)]
    for f in range(2):
        name = "%05d.png" % f
        for d in ("alpha", "uv_1", "uv_2"):      # the default's files: a run with size=None writes the same bytes
            assert (tmp_path / "plain" / d / name).read_bytes() == (tmp_path / "none" / d / name).read_bytes()
        assert _png(tmp_path / "plain" / "alpha" / name).shape == (3, 4) and (_png(tmp_path / "plain" / "alpha" / name) == 127).all()
        al = _png(tmp_path / "sized" / "alpha" / name)
        assert al.shape == (5, 7) and al.dtype == np.uint8 and (al == 40 + f).all()                  # the library's bytes, not a host cast
        assert np.array_equal(_png(tmp_path / "sized" / "uv_1" / name), to_u8(normalize_uv(np.zeros((5, 7, 2), np.float32), 0.5, 1, 0, 0)))
        assert np.array_equal(_png(tmp_path / "sized" / "uv_2" / name),
                              to_u8(normalize_uv(np.full((5, 7, 2), 0.25, np.float32), -0.5, win[2], win[0], win[1])))
    for t in ("texture_orig1.png", "texture_orig2.png"):      # the textures do not depend on the size
        assert (tmp_path / "plain" / t).read_bytes() == (tmp_path / "sized" / t).read_bytes()


def test_evaluation_passes_the_size_on(tmp_path, monkeypatch):
    from aiod_amd import atlas_outputs, stage1
    seen = []
    monkeypatch.setattr(atlas_outputs, "write_atlas_outputs", lambda af, d, res=1000, size=None: seen.append(size))

    class _Eval:
        two_layer = False

        def render_frame(self, f):
            return np.full((2, 3, 3), 0.5, np.float32), 4.5
    video = np.zeros((2, 3, 3, 2), np.float32)
    stage1.evaluate_model_single(_Eval(), video, tmp_path / "a", 30, save_checkpoint_file=False, atlas_outputs=True)
    stage1.evaluate_model_single(_Eval(), video, tmp_path / "b", 30, save_checkpoint_file=False, atlas_outputs=True, atlas_outputs_hw=(8, 12))
    stage1.evaluate_model_single(_Eval(), video, tmp_path / "c", 30, save_checkpoint_file=False, atlas_outputs_hw=(8, 12))
    assert seen == [None, (8, 12)]


def test_cli_flags(monkeypatch, tmp_path):
    from aiod_amd import atlas_edit, stage1, stage1_seg
    seen = []
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "0")      # _cli sets both: restored when the test ends
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0")
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(stage1, "main", lambda config, args, two_layer=False: seen.append((args.atlas_outputs, args.atlas_outputs_size, args.style_size)))
    base = ["--vid_name", "clip", "--skip_preprocess"]
    stage1_seg._cli(base)
    stage1_seg._cli(base + ["--atlas_outputs"])
    stage1_seg._cli(base + ["--atlas_outputs", "--atlas_outputs_size", "stage1"])
    stage1_seg._cli(base + ["--atlas_outputs", "--atlas_outputs_size", "full"])
    stage1_seg._cli(base + ["--atlas_outputs", "--style_size", "full"])                  # not tied to --style_size
    assert seen == [(False, "stage1", "stage1"), (True, "stage1", "stage1"), (True, "stage1", "stage1"), (True, "full", "stage1"), (True, "stage1", "full")]
    for bad in (base + ["--atlas_outputs_size", "full"], base + ["--atlas_outputs", "--atlas_outputs_size", "4k"]):
        with pytest.raises(SystemExit):
            stage1_seg._cli(bad)
    with pytest.raises(SystemExit):      # the single-atlas CLI has no layer outputs
        stage1._cli(base + ["--atlas_outputs_size", "full"])
    ran = []
    monkeypatch.setattr(atlas_edit, "run", lambda args: ran.append(args.size))
    atlas_edit._cli(["--vid_name", "clip", "--edit_fg", "a.png"])
    atlas_edit._cli(["--vid_name", "clip", "--edit_fg", "a.png", "--size", "full"])
    atlas_edit._cli(["--vid_name", "clip", "--edit_bg", "b.png", "--size", "90x160"])
    assert ran == ["stage1", "full", "90x160"]
    for bad in ("4k", "90x", "0x4"):
        with pytest.raises(SystemExit):
            atlas_edit._cli(["--vid_name", "clip", "--edit_fg", "a.png", "--size", bad])
    assert len(ran) == 3


def test_symbols_and_wrappers_exist():
    import aiod_amd
    hdr = open(os.path.join(ROOT, "include", "atlasfit.h")).read()
    declared = set(re.findall(r"\b(af_[a-z_0-9]+)\s*\(", hdr))
    new = {"af_render_layers_at", "af_edit_create", "af_edit_frame", "af_edit_usage", "af_edit_reset_usage", "af_edit_destroy"}
    assert new <= declared and new <= set(aiod_amd.atlasfit.ABI_SYMBOLS)
    lib = aiod_amd.load_library()
    for s in new:
        assert hasattr(lib, s), s
    for name in ("render_layers_at", "render_layers_at_device", "edit_session"):
        assert callable(getattr(aiod_amd.AtlasFit, name))
    for name in ("frame", "frame_device", "usage", "reset_usage", "close", "__enter__", "__exit__"):
        assert callable(getattr(aiod_amd.EditSession, name))


def test_python_checks_come_before_the_library():
    """Shape, dtype and name errors are ValueErrors raised before any library call (no handle is touched)."""
    import aiod_amd

    class _NoLib:
        def __getattr__(self, name):
            raise AssertionError("library call %s" % name)
    af = aiod_amd.AtlasFit.__new__(aiod_amd.AtlasFit)
    af.lib, af.h, af.two_layer, af.device = _NoLib(), None, False, 0
    af.cfg = aiod_amd.default_config(8, 6, 3)
    with pytest.raises(ValueError, match="unknown outputs"):
        af.render_layers_at(0, 4, 4, which=("uv1", "depth"))
    with pytest.raises(ValueError, match="two_layer"):
        af.render_layers_at(0, 4, 4, which=("uv2",))
    with pytest.raises(ValueError, match=r"\(res, res, 3\)"):
        af.edit_session(8, tex_fg=np.zeros((8, 7, 3), np.float32), win_fg=(0, 0, 1))
    with pytest.raises(ValueError, match="window"):
        af.edit_session(8, tex_fg=np.zeros((8, 8, 3), np.float32), win_fg=(0, 0))
    s = aiod_amd.EditSession.__new__(aiod_amd.EditSession)
    s.af, s.lib, s.e, s.res = af, af.lib, None, 8
    with pytest.raises(ValueError, match="unknown outputs"):
        s.frame(0, outputs=("edit", "matte"))
    with pytest.raises(aiod_amd.AtlasFitError) as e:      # a closed session: the state error, without a library call
        s.frame(0)
    assert e.value.code == -5
    s.close()
    af.h = None
