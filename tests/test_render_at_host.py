"""Host-side checks of the render-at-any-size feature (no GPU): the identities of the coordinate restatement (tests/render_at_ref.py),
what Deflicker.run asks of its engines with style_size "full" and that "stage1" asks nothing new, the --style_size flag of the four CLIs
and the keys of the records."""
import argparse
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "all-in-one-deflicker_amd")
sys.path.insert(0, HERE)
import render_at_ref as R  # noqa: E402
from test_deflicker_host import SMALL, _StubAtlas, _StubEngines, _frames, _load  # noqa: E402


# ---- the coordinate rule -------------------------------------------------------------------------------------------------------
def _lattice(resx, resy, f=1, nframes=6):
    """The lattice's rows: (float)x / half_main - 1 in fp32."""
    half = np.float32(max(resx, resy) / 2.0)
    rows = np.zeros((resy, resx, 4), np.float32)
    rows[:, :, 0] = (np.arange(resx, dtype=np.float32) / half - np.float32(1))[None, :]
    rows[:, :, 1] = (np.arange(resy, dtype=np.float32) / half - np.float32(1))[:, None]
    rows[:, :, 2] = np.float32(R.frame_time(f, nframes))
    return rows


@pytest.mark.parametrize("resx,resy", [(24, 33), (97, 24), (768, 432), (40, 24)])
def test_same_size_gives_the_lattice_rows(resx, resy):
    got = R.coords(resx, resy, resy, resx, 1, 6).reshape(resy, resx, 4)
    assert np.array_equal(got.view(np.uint32), _lattice(resx, resy).view(np.uint32))
    assert np.array_equal(R.source_positions(resx, resx), np.arange(resx, dtype=np.float64))


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("n", [24, 33, 97, 768])
def test_odd_factor_hits_every_lattice_pixel(n, k):
    s = R.source_positions(n, k * n)
    assert np.array_equal(s[(k - 1) // 2::k], np.arange(n, dtype=np.float64))
    got = R.coords(n, 24, 24 * k, n * k, 0, 6).reshape(24 * k, n * k, 4)[(k - 1) // 2::k, (k - 1) // 2::k]
    assert np.array_equal(got.view(np.uint32), _lattice(n, 24, 0).view(np.uint32))


@pytest.mark.parametrize("src,dst", [(40, 67), (24, 41), (40, 120), (40, 20), (768, 1920), (432, 2160), (40, 1), (1, 7), (768, 16384)])
def test_clamped_and_monotone(src, dst):
    s = R.source_positions(src, dst)
    assert s.min() >= 0.0 and s.max() <= src - 1.0 and (np.diff(s) >= 0).all()
    if dst > src:          # up-scaling: half a source pixel hangs over each border and is clamped onto the border pixel
        assert s[0] == 0.0 and s[-1] == src - 1.0
    x = R.coords(src, 3, 2, dst, 0, 6).reshape(2, dst, 4)[0, :, 0]
    assert (np.diff(x) >= 0).all() and x[0] >= -1.0
    free = (s > 0.0) & (s < src - 1.0)      # away from the clamp the rule is cv2.resize's (d + 0.5) * scale - 0.5
    d = np.arange(dst, dtype=np.float64)
    assert np.array_equal(s[free], ((d + 0.5) * (float(src) / dst) - 0.5)[free])


def test_twin_positions_are_the_unrounded_ones():
    a, b = R.coords(40, 24, 41, 67, 3, 6), R.coords64(40, 24, 41, 67, 3, 6)
    assert a.dtype == np.float32 and b.dtype == np.float64 and a.shape == (41 * 67, 4) and b.shape == (41 * 67, 3)
    # three fp32 roundings: the position (relative 2^-24 of a quotient below 2), the quotient (half an ulp below 2) and the difference
    assert np.abs(a[:, :3] - b).max() <= 2.0 ** -23 + 2.0 ** -24 + 2.0 ** -25 and (a[:, 3] == 0).all()


# ---- orchestration ---------------------------------------------------------------------------------------------------------------
class _AtAtlas(_StubAtlas):
    """The stub handle of test_deflicker_host.py, logging its render calls, with the new one."""

    def render_frame_device(self, f, want_float=True, want_u8=True):
        self.log.append(("render", f, want_float, want_u8))
        rgb, u8, sse = super().render_frame_device(f, want_float=want_float, want_u8=True)
        return rgb, (u8 if want_u8 else None), sse

    def render_frame_at_device(self, f, oh, ow, want_float=True, want_u8=True, ref=None):
        self.log.append(("render_at", f, oh, ow, want_float, want_u8, int(np.asarray(ref)[0, 0, 0]), np.asarray(ref).shape))
        rgb = np.full((oh, ow, 3), self.frames[f] / 255.0, np.float32)
        return (rgb if want_float else None), np.full(rgb.shape, self.frames[f], np.uint8), 0.01 * rgb.size


class _AtEngines(_StubEngines):
    def open_atlas(self, resx, resy, n, config):
        import aiod_amd
        self.log.append(("atlas_open", resx, resy, n))
        return _AtAtlas(self.log, aiod_amd.default_config(resx, resy, n, config))


@pytest.mark.parametrize("overlap,windows", [(0, [(0, 5), (5, 9)]), (1, [(0, 5), (4, 9)])])
def test_full_run_renders_every_frame_at_the_clip_size(overlap, windows):
    import aiod_amd
    E = _AtEngines()
    d = aiod_amd.Deflicker(None, None, None, config=SMALL, down=4, seed=7, window_overlap=overlap, engines=E, style_size="full")
    res = d.run(_frames(9), keep=("final", "stage1"))
    assert res["windows"] == windows and res["style_size"] == "full"
    assert res["stage1"].shape == (9, 8, 12, 3) and res["final"].shape == (9, 8, 12, 3)      # the kept styles have the clip's size
    want = []
    for a, b in windows:
        for f in range(b - a):       # per frame: the small render for its error sum alone, then the full-size one against the device frame
            want += [("render", f, False, False), ("render_at", f, 8, 12, overlap > 0, True, a + f, (8, 12, 3))]
    assert [e for e in E.log if e[0] in ("render", "render_at")] == want
    assert len(res["psnr"]) == 2 and res["psnr"] == pytest.approx([10 * np.log10(1 / 0.25)] * 2)      # still the stage-1-size figure
    assert res["psnr_full"] == pytest.approx([10 * np.log10(1 / 0.01)] * 2)
    assert [e[1:] for e in E.log if e[0] == "filter"] == [(i, i) for i in range(9)]
    assert [int(f[0, 0, 0]) for f in res["stage1"]] == list(range(9))


def test_stage1_run_makes_none_of_the_new_calls():
    import aiod_amd
    for kw in ({}, {"style_size": "stage1"}):
        E = _AtEngines()
        res = aiod_amd.Deflicker(None, None, None, config=SMALL, down=4, seed=7, engines=E, **kw).run(_frames(9), keep=("final", "stage1"))
        assert [e[0] for e in E.log if e[0].startswith("render")] == ["render"] * 9
        assert all(e[2:] == (False, True) for e in E.log if e[0] == "render")
        assert res["stage1"].shape == (9, 2, 3, 3) and res["style_size"] == "stage1" and res["psnr_full"] is None
    with pytest.raises(ValueError, match="style_size must be one of stage1, full"):
        aiod_amd.Deflicker(None, None, None, config=SMALL, engines=_AtEngines(), style_size="big")


def test_cross_fade_blends_the_full_size_renders():
    import aiod_amd
    E = _AtEngines()
    res = aiod_amd.Deflicker(None, None, None, config=SMALL, down=4, seed=7, window_overlap=1, engines=E, style_size="full").run(
        _frames(9), keep=("final", "stage1", "renders"))
    assert [r.shape for r in res["renders"]] == [(5, 8, 12, 3), (5, 8, 12, 3)]
    blend = E.lerp(res["renders"][0][4], res["renders"][1][0], 0.5)
    assert np.array_equal(res["stage1"][4], E.quantise_render(blend))


# ---- flags and records -----------------------------------------------------------------------------------------------------------
def test_deflicker_flag_and_record(monkeypatch, tmp_path):
    import torch
    from PIL import Image
    from aiod_amd import deflicker
    assert deflicker.parse_args(["--frames_dir", "x"]).style_size == "stage1"
    assert deflicker.parse_args(["--frames_dir", "x", "--style_size", "full"]).style_size == "full"
    with pytest.raises(SystemExit):
        deflicker.parse_args(["--frames_dir", "x", "--style_size", "half"])
    clip = tmp_path / "clip"
    clip.mkdir()
    for i, f in enumerate(_frames(3)):
        Image.fromarray(f).save(str(clip / ("%05d.png" % i)))
    (tmp_path / "cfg.json").write_text(json.dumps(SMALL))
    E = _AtEngines()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(deflicker, "load_checkpoints", lambda opts: (None, None, None))
    monkeypatch.setattr(deflicker, "DeviceEngines", lambda *a, **k: E)
    argv = ["--frames_dir", str(clip), "--out", str(tmp_path / "out"), "--config", str(tmp_path / "cfg.json"), "--seed", "7"]
    assert deflicker.main(argv + ["--style_size", "full"]) == 0
    rec = json.load(open(tmp_path / "out" / "deflicker.json"))
    assert rec["style_size"] == "full" and len(rec["psnr_full"]) == 1 and len(rec["psnr"]) == 1
    assert [e[2:4] for e in E.log if e[0] == "render_at"] == [(8, 12)] * 3
    assert deflicker.main(argv) == 0
    rec = json.load(open(tmp_path / "out" / "deflicker.json"))
    assert rec["style_size"] == "stage1" and rec["psnr_full"] is None


def test_stage1_flags_reach_main(monkeypatch, tmp_path):
    from aiod_amd import stage1, stage1_seg
    seen = []
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "0")      # _cli sets both: restored when the test ends
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0")
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(stage1, "main", lambda config, args, two_layer=False: seen.append((args.style_size, two_layer)))
    stage1._cli(["--vid_name", "clip", "--skip_preprocess"])
    stage1._cli(["--vid_name", "clip", "--skip_preprocess", "--style_size", "full"])
    stage1_seg._cli(["--vid_name", "clip", "--skip_preprocess", "--style_size", "full"])
    assert seen == [("stage1", False), ("full", False), ("full", True)]
    with pytest.raises(SystemExit):
        stage1._cli(["--vid_name", "clip", "--skip_preprocess", "--style_size", "4k"])


class _EvalAtlas:
    two_layer = False

    def __init__(self):
        self.calls = []

    def render_frame(self, f):
        self.calls.append(("render", f))
        return np.full((2, 3, 3), 0.5, np.float32), 0.25 * 18

    def render_frame_u8(self, f, want_float=True, want_u8=True):
        self.calls.append(("render_u8", f, want_float, want_u8))
        return None, None, 0.25 * 18

    def render_frame_at_u8(self, f, oh, ow, want_float=True, want_u8=True, ref=None):
        self.calls.append(("render_at", f, oh, ow, want_float, want_u8))
        return None, np.full((oh, ow, 3), 10 + f, np.uint8), None


def test_stage1_evaluation_writes_full_size_frames(tmp_path):
    from PIL import Image
    from aiod_amd import stage1
    video = np.zeros((2, 3, 3, 2), np.float32)
    af = _EvalAtlas()
    p = stage1.evaluate_model_single(af, video, tmp_path / "full", 30, save_checkpoint_file=False, style_hw=(8, 12))
    assert af.calls == [("render_u8", 0, False, False), ("render_at", 0, 8, 12, False, True), ("render_u8", 1, False, False), ("render_at", 1, 8, 12, False, True)]
    for f in range(2):
        im = np.array(Image.open(str(tmp_path / "full" / "output" / ("%05d.png" % f))))
        assert im.shape == (8, 12, 3) and (im == 10 + f).all()
    af0 = _EvalAtlas()
    p0 = stage1.evaluate_model_single(af0, video, tmp_path / "small", 30, save_checkpoint_file=False)
    assert af0.calls == [("render", 0), ("render", 1)]
    assert np.array(Image.open(str(tmp_path / "small" / "output" / "00000.png"))).shape == (2, 3, 3)
    assert p == p0 and os.listdir(tmp_path / "full" / "000030") == os.listdir(tmp_path / "small" / "000030")      # the PSNR file is the stage-1-size one


def test_run_pipeline_passes_the_flag_on():
    Rp = _load("af_run_pipeline_at", os.path.join(PKG, "run_pipeline.py"))
    base = dict(video_name="data/test/clip.mp4", video_frame_folder=None, fps=10, gpu=0, class_name=None)
    off = Rp.build_commands(argparse.Namespace(**base))
    assert Rp.build_commands(argparse.Namespace(style_size="stage1", **base)) == off
    on = Rp.build_commands(argparse.Namespace(style_size="full", **base))
    assert on[2] == (off[2][0], off[2][1] + " --style_size full") and on[:2] == off[:2] and on[3:] == off[3:]
    both = Rp.build_commands(argparse.Namespace(style_size="full", native_flow=True, native_stage2=True, **base))
    assert both[2][1].endswith(" --native_flow --style_size full") and "--style_size" not in both[3][1]
    seg = Rp.build_commands(argparse.Namespace(style_size="full", **dict(base, class_name="portrait")))
    assert "stage1_seg.py" in seg[2][1] and seg[2][1].endswith(" --style_size full")
    ip_off = Rp.build_commands(argparse.Namespace(in_process=True, **base))
    ip = Rp.build_commands(argparse.Namespace(in_process=True, style_size="full", **base))
    assert ip[-1] == (ip_off[-1][0], ip_off[-1][1] + " --style_size full") and len(ip) == len(ip_off)


def test_symbol_and_wrappers_exist():
    import re
    import aiod_amd
    hdr = open(os.path.join(ROOT, "include", "atlasfit.h")).read()
    assert "af_render_frame_at" in set(re.findall(r"\b(af_[a-z_0-9]+)\s*\(", hdr)) and "af_render_frame_at" in aiod_amd.atlasfit.ABI_SYMBOLS
    for name in ("render_frame_at", "render_frame_at_u8", "render_frame_at_device"):
        assert hasattr(aiod_amd.AtlasFit, name)
