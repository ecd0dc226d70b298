"""Host-side checks of the one-process pipeline (no GPU): the window planner, the cross-fade weights, the order of work of
Deflicker.run with stub engines, the CLI's defaults, run_pipeline's --in_process switch and the exported af_render_frame_u8."""
import argparse
import importlib.util
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "all-in-one-deflicker_amd")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- plan_windows --------------------------------------------------------------------------------------------------------------
def _check_plan(n, m, o):
    from aiod_amd import plan_windows
    w = plan_windows(n, m, o)
    if n <= m:
        assert w == [(0, n)], (n, m, o, w)
        return
    k = math.ceil((n - o) / (m - o))
    assert len(w) == k, (n, m, o, w)
    assert w[0][0] == 0 and w[-1][1] == n
    lengths = [b - a for a, b in w]
    assert max(lengths) <= m and max(lengths) - min(lengths) <= 1 and min(lengths) > o, (n, m, o, w)
    for (a0, b0), (a1, b1) in zip(w, w[1:]):
        assert b0 - a1 == o and a1 > a0 and b1 > b0, (n, m, o, w)       # exactly `overlap` shared frames, strictly advancing


def test_plan_windows_properties():
    for m in (2, 3, 5, 8, 200):
        for o in sorted({0, 1, 2, m // 2, m - 1}):
            if o >= m:
                continue
            for n in sorted({1, 2, m - 1, m, m + 1, m + 2, 2 * m - o, 2 * m - o + 1, 3 * m, 3 * m + 1, 7 * m + 3}):
                if n >= 1:
                    _check_plan(n, m, o)


def test_plan_windows_examples_and_rejections():
    from aiod_amd import plan_windows
    assert plan_windows(9, 5, 0) == [(0, 5), (5, 9)]
    assert plan_windows(9, 5, 1) == [(0, 5), (4, 9)]
    assert plan_windows(200, 200, 0) == [(0, 200)]
    assert plan_windows(201, 200, 0) == [(0, 101), (101, 201)]
    assert plan_windows(201, 200, 199) == [(0, 200), (1, 201)]
    assert plan_windows(7, 5, 4) == [(0, 5), (1, 6), (2, 7)]
    for bad in (-1, 5, 6):
        with pytest.raises(ValueError, match="overlap"):
            plan_windows(9, 5, bad)


def test_cross_fade_weights_and_seams():
    from aiod_amd.deflicker import cross_fade_weights, seam_pairs
    for K in range(0, 9):
        np.testing.assert_array_equal(np.array(cross_fade_weights(K)), (np.arange(K) + 1.0) / (K + 1.0))
    assert cross_fade_weights(1) == [0.5]
    assert seam_pairs([(0, 5), (5, 9)], 9) == [4]
    assert seam_pairs([(0, 5), (4, 9)], 9) == [3, 4]
    assert seam_pairs([(0, 9)], 9) == []


# ---- orchestration with stub engines -------------------------------------------------------------------------------------------
def _ident(img):
    return int(np.asarray(img)[0, 0, 0])


class _StubFlow:
    def __init__(self, log, h, w):
        self.log, self.h, self.w, self.capacity, self.slots = log, h, w, 2, {}

    def encode(self, slot, img):
        assert img.dtype == np.uint8 and img.shape == (self.h, self.w, 3)
        self.log.append(("encode", _ident(img)))
        self.slots[slot] = _ident(img)

    def flow_slots(self, pairs, on_device=False):
        assert on_device
        self.log.append(("flow", [(self.slots[a], self.slots[b]) for a, b in pairs]))
        return np.stack([np.full((self.h, self.w, 2), 100 * self.slots[a] + self.slots[b], np.float32) for a, b in pairs])

    def close(self):
        self.log.append(("raft_close",))


class _StubAtlas:
    def __init__(self, log, cfg):
        self.log, self.cfg, self.arithmetic, self.frames = log, cfg, {"mlp_mode": 3, "dw_mode": 1, "overrides": []}, None

    def load_state_dict(self, net, sd):
        pass

    def pre_train_mapping(self, iters, seed=0, net=0):
        self.log.append(("pretrain", int(seed)))

    def upload_video(self, video_frames, flows, flows_rev, flows_mask, flows_rev_mask, mask_frames=None):
        self.frames = video_frames
        self.log.append(("upload", list(video_frames), list(flows), list(flows_rev)))

    def train_steps(self, first, count, inds, seed=0, return_losses=True):
        self.log.append(("train", first, count, int(seed)))

    def render_frame_device(self, f, want_float=True, want_u8=True):
        rgb = np.full((self.cfg.resy, self.cfg.resx, 3), self.frames[f] / 255.0, np.float32)
        return (rgb if want_float else None), np.full(rgb.shape, self.frames[f], np.uint8), 0.25 * rgb.size

    def close(self):
        self.log.append(("atlas_close",))


class _StubFilter:
    def __init__(self, log):
        self.log = log

    def reset(self):
        self.log.append(("reset",))

    def frame(self, content, style):
        self.log.append(("filter", int(round(float(content[0, 0, 0]) * 255)), int(round(float(style[0, 0, 0]) * 255))))
        return content, style

    def activation(self, name):
        raise AssertionError("no intermediates were asked for")

    def close(self):
        self.log.append(("filter_close",))


class _StubEngines:
    def __init__(self):
        self.log = []

    def frame(self, x):
        return np.asarray(x)

    def open_flow(self, h, w):
        self.log.append(("raft_open", h, w))
        return _StubFlow(self.log, h, w)

    def resize_flow(self, f, h, w):
        return ("small", int(f[0, 0, 0]), h, w)

    def open_atlas(self, resx, resy, n, config):
        import aiod_amd
        self.log.append(("atlas_open", resx, resy, n))
        return _StubAtlas(self.log, aiod_amd.default_config(resx, resy, n, config))

    def inputs(self, frames, flows12, flows21, resy, resx):
        return (None, [_ident(f) for f in frames], None, [f[1] for f in flows21], [f[1] for f in flows12])

    def open_filter(self, h, w):
        self.log.append(("filter_open", h, w))
        return _StubFilter(self.log)

    def resize(self, img, h, w):
        img = np.asarray(img)
        return np.full((h, w, 3), img[0, 0, 0] / 255.0 if img.dtype == np.uint8 else img[0, 0, 0], np.float32)

    def quantise(self, img):
        return (np.clip(img, 0, 1) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)      # rounds: the stub's idents survive x / 255 * 255

    def quantise_render(self, img):
        return (img.astype(np.float64) * 255 + 0.5).astype(np.uint8)

    def lerp(self, a, b, w):
        return a + np.float32(w) * (b - a)

    def stack(self, imgs):
        return np.stack(imgs)

    def to_host(self, t):
        return np.asarray(t)

    def sync(self):
        pass


SMALL = {"maximum_number_of_frames": 5, "iters_num": 61, "evaluate_every": 30, "pretrain_iter_number": 2, "samples_batch": 64,
         "number_of_channels_atlas": 16, "number_of_channels_mapping1": 16}


def _frames(n, h=8, w=12):
    return [np.full((h, w, 3), i, np.uint8) for i in range(n)]


@pytest.mark.parametrize("overlap,windows", [(0, [(0, 5), (5, 9)]), (1, [(0, 5), (4, 9)])])
def test_order_of_work_with_stub_engines(overlap, windows):
    import aiod_amd
    E = _StubEngines()
    d = aiod_amd.Deflicker(None, None, None, config=SMALL, down=4, seed=7, window_overlap=overlap, engines=E)
    res = d.run(_frames(9), keep=("final", "stage1"))
    log = E.log
    assert res["windows"] == windows and len(res["psnr"]) == 2 and res["seed"] == 7
    assert res["final"].shape == (9, 8, 12, 3) and res["stage1"].shape == (9, 2, 3, 3)
    assert set(res["seconds"]) == {"decode + flow", "stage 1", "stage 2", "total"}
    # RAFT: one handle, every frame encoded exactly once and in order, both directions of every pair in one launch, in order
    assert [e for e in log if e[0] == "raft_open"] == [("raft_open", 8, 12)]
    assert [e[1] for e in log if e[0] == "encode"] == list(range(9))
    assert [e[1] for e in log if e[0] == "flow"] == [[(i, i + 1), (i + 1, i)] for i in range(8)]
    # ... and closed before stage 1 trains (before its handle exists, even)
    names = [e[0] for e in log]
    assert names.index("raft_close") < names.index("atlas_open") < names.index("train")
    # stage 1: each window gets exactly its frames and its internal pairs, its own handle and seed, the CLI's schedule, and is closed
    opens = [e for e in log if e[0] == "atlas_open"]
    assert opens == [("atlas_open", 3, 2, b - a) for a, b in windows]
    uploads = [e for e in log if e[0] == "upload"]
    for (a, b), up in zip(windows, uploads):
        assert up[1] == list(range(a, b))
        assert up[2] == [100 * i + i + 1 for i in range(a, b - 1)] and up[3] == [100 * (i + 1) + i for i in range(a, b - 1)]
    trains = [e for e in log if e[0] == "train"]
    assert [t[1:3] for t in trains] == [(0, 31), (31, 30)] * 2
    assert trains[0][3] == trains[1][3] and trains[2][3] == trains[3][3] and trains[0][3] != trains[2][3]      # one sampler seed per window
    assert len([e for e in log if e[0] == "pretrain"]) == 2 and names.count("atlas_close") == 2
    for w in range(2):                                   # pre-train and upload of a window come before its first train_steps
        seg = names[names.index("atlas_open", names.index("atlas_open") + w):]
        assert seg.index("pretrain") < seg.index("train") and seg.index("upload") < seg.index("train")
    # stage 2: one handle, one reset, every frame once and in order, content i with style i, after the last window's fit
    assert names.count("filter_open") == 1 and names.count("reset") == 1 and names.count("filter_close") == 1
    assert names.index("filter_open") > len(names) - 1 - names[::-1].index("atlas_close")
    assert names.index("reset") < names.index("filter")
    assert [e[1:] for e in log if e[0] == "filter"] == [(i, i) for i in range(9)]
    assert [int(f[0, 0, 0]) for f in res["final"]] == list(range(9))
    assert res["seam_pairs"] == ([4] if overlap == 0 else [3, 4])


def test_same_seed_same_draws_and_window_seed_is_seed_plus_k():
    import aiod_amd
    seeds = []
    for clip, seed in ((_frames(9), 7), (_frames(9)[5:], 8)):
        E = _StubEngines()
        aiod_amd.Deflicker(None, None, None, config=SMALL, seed=seed, engines=E).run(clip)
        seeds.append([(e[1] if e[0] == "pretrain" else e[3]) for e in E.log if e[0] in ("pretrain", "train")])
    assert seeds[0][3:] == seeds[1]                     # window 1 of the long clip draws what a stand-alone run with seed + 1 draws


def test_errors_close_the_handles():
    import aiod_amd
    E = _StubEngines()
    d = aiod_amd.Deflicker(None, None, None, config=SMALL, seed=1, engines=E)
    with pytest.raises(ValueError, match="at least 2 frames"):
        d.run(_frames(1))
    bad = _frames(4)
    bad[2] = np.zeros((8, 13, 3), np.uint8)
    with pytest.raises(ValueError, match="frame 2 is 13x8, the first frame 12x8"):
        d.run(bad)
    names = [e[0] for e in E.log]
    assert names.count("raft_open") == names.count("raft_close") and "atlas_open" not in names
    with pytest.raises(ValueError, match="overlap"):
        aiod_amd.Deflicker(None, None, None, config=SMALL, window_overlap=5, engines=E)
    with pytest.raises(ValueError, match="reaches no evaluation"):
        aiod_amd.Deflicker(None, None, None, config=dict(SMALL, iters_num=10), engines=E)
    with pytest.raises(ValueError, match="unknown"):
        d.run(_frames(3), keep=("final", "nonsense"))
    assert d.run(_frames(3))["final"].shape == (3, 8, 12, 3)      # and the object still works


# ---- CLI, driver, ABI ----------------------------------------------------------------------------------------------------------
def test_cli_defaults(tmp_path):
    from aiod_amd import deflicker
    o = deflicker.parse_args(["--frames_dir", "data/test/clip/"])
    assert o.out == os.path.join("results", "clip") and o.config is None and o.down == 4 and o.seed is None and o.gpu == 0
    assert o.model == "pretrained_weights/raft-things.pth" and o.ckpt_filter == "./pretrained_weights/neural_filter.pth"
    assert o.ckpt_local == "./pretrained_weights/local_refinement_net.pth" and o.window_overlap == 0
    assert not o.keep_intermediates and not o.warp_error and o.warp_error_geometry == "exact"
    o = deflicker.parse_args(["--frames_dir", "x", "--out", "y", "--window_overlap", "3", "--warp_error", "--warp_error_geometry", "reference"])
    assert o.out == "y" and o.window_overlap == 3 and o.warp_error and o.warp_error_geometry == "reference"
    with pytest.raises(SystemExit, match="nowhere.pth not found \\(--model\\)"):
        deflicker.load_checkpoints(argparse.Namespace(model="nowhere.pth", ckpt_filter="a", ckpt_local="b"))
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(PKG, "deflicker.py"), "--help"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0 and "--window_overlap" in r.stdout and "--keep_intermediates" in r.stdout


def test_run_pipeline_in_process_switch():
    R = _load("af_run_pipeline_ip", os.path.join(PKG, "run_pipeline.py"))
    base = dict(video_name="data/test/clip.mp4", video_frame_folder=None, fps=10, gpu=2, class_name=None)
    py = sys.executable or "python"
    off = R.build_commands(argparse.Namespace(**base))
    assert off == [("mkdir", "./data/test/clip"),
                   ("sh", "ffmpeg -i data/test/clip.mp4 -vf fps=10 -start_number 0 ./data/test/clip/%05d.png"),
                   ("sh", "%s %s --vid_name clip --gpu 2" % (py, os.path.join(PKG, "stage1.py"))),
                   ("sh", "python src/neural_filter_and_refinement.py --video_name clip --fps 10")]
    assert R.build_commands(argparse.Namespace(in_process=False, **base)) == off
    on = R.build_commands(argparse.Namespace(in_process=True, ckpt_filter="f.pth", ckpt_local="l.pth", **base))
    assert on[:2] == off[:2] and len(on) == 3
    assert on[2] == ("sh", "%s %s --frames_dir ./data/test/clip --out ./results/clip --gpu 2 --ckpt_filter f.pth --ckpt_local l.pth"
                     % (py, os.path.join(PKG, "deflicker.py")))
    with pytest.raises(ValueError, match="single-atlas"):
        R.build_commands(argparse.Namespace(in_process=True, **dict(base, class_name="portrait")))


def test_render_frame_u8_is_exported():
    import re
    import __graft_entry__ as ge
    ge.build()
    import aiod_amd
    lib = aiod_amd.load_library()
    hdr = open(os.path.join(ROOT, "include", "atlasfit.h")).read()
    assert "af_render_frame_u8" in set(re.findall(r"\b(af_[a-z_0-9]+)\s*\(", hdr))
    assert "af_render_frame_u8" in aiod_amd.atlasfit.ABI_SYMBOLS and hasattr(lib, "af_render_frame_u8")
    assert hasattr(aiod_amd.AtlasFit, "render_frame_device")
