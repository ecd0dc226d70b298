"""Host-side checks of the fg/bg two-layer route of the one-process pipeline (no GPU): `Deflicker.run(frames, masks=...)` with stub
engines of this file's own, and the `--masks_dir` side of the CLI.  Two stubs: `_TodayEngines` has the engine signatures as they were
before the two-layer route existed, so a `masks=None` run that passed one argument more would be a TypeError; `_SegEngines` adds the
mask upload and the two optional arguments."""
import json
import os
import re

import numpy as np
import pytest

H, W = 8, 12
SMALL = {"maximum_number_of_frames": 5, "iters_num": 61, "evaluate_every": 30, "pretrain_iter_number": 2, "samples_batch": 64,
         "number_of_channels_atlas": 16, "number_of_channels_mapping1": 16, "number_of_channels_mapping2": 16, "number_of_channels_alpha": 16}


def _ident(img):
    return int(np.asarray(img).reshape(-1)[0])


class _Flow:
    def __init__(self, log, h, w):
        self.log, self.h, self.w, self.slots = log, h, w, {}

    def encode(self, slot, img):
        self.slots[slot] = _ident(img)

    def flow_slots(self, pairs, on_device=False):
        return np.stack([np.full((self.h, self.w, 2), 100 * self.slots[a] + self.slots[b], np.float32) for a, b in pairs])

    def close(self):
        self.log.append(("raft_close",))


class _Atlas:
    def __init__(self, log, cfg):
        self.log, self.cfg, self.arithmetic, self.frames = log, cfg, {"mlp_mode": 3, "dw_mode": 1, "overrides": []}, None

    def load_state_dict(self, net, sd):
        self.log.append(("load", int(net)))

    def pre_train_mapping(self, iters, seed=0, net=0):
        self.log.append(("pretrain", int(net), int(seed)))

    def upload_video(self, *args):
        self.frames = args[0]
        self.log.append(("upload",) + tuple(None if a is None else list(a) for a in args))

    def train_steps(self, first, count, inds, seed=0, return_losses=True):
        self.log.append(("train", first, count, int(seed)))

    def render_frame_device(self, f, want_float=True, want_u8=True):
        rgb = np.full((self.cfg.resy, self.cfg.resx, 3), self.frames[f] / 255.0, np.float32)
        return (rgb if want_float else None), np.full(rgb.shape, self.frames[f], np.uint8), 0.25 * rgb.size

    def close(self):
        self.log.append(("atlas_close",))


class _Filter:
    def __init__(self, log):
        self.log = log

    def reset(self):
        pass

    def frame(self, content, style):
        return content, style

    def close(self):
        self.log.append(("filter_close",))


class _TodayEngines:
    """The engine methods a single-atlas run uses, with the signatures they had before this route: `calls` records every one."""

    def __init__(self):
        self.log, self.calls = [], []

    def frame(self, x):
        self.calls.append(("frame", _ident(x)))
        return np.asarray(x)

    def open_flow(self, h, w):
        self.calls.append(("open_flow", h, w))
        return _Flow(self.log, h, w)

    def resize_flow(self, f, h, w):
        self.calls.append(("resize_flow", int(f[0, 0, 0]), h, w))
        return ("small", int(f[0, 0, 0]))

    def open_atlas(self, resx, resy, n, config):
        import aiod_amd
        self.calls.append(("open_atlas", resx, resy, n))
        self.log.append(("atlas_open", n, False))
        return _Atlas(self.log, aiod_amd.default_config(resx, resy, n, config))

    def inputs(self, frames, flows12, flows21, resy, resx):
        self.calls.append(("inputs", [_ident(f) for f in frames], [f[1] for f in flows12], [f[1] for f in flows21], resy, resx))
        return (None, [_ident(f) for f in frames], None, [f[1] for f in flows21], [f[1] for f in flows12])

    def open_filter(self, h, w):
        self.calls.append(("open_filter", h, w))
        return _Filter(self.log)

    def resize(self, img, h, w):
        self.calls.append(("resize", h, w))
        img = np.asarray(img)
        return np.full((h, w, 3), img[0, 0, 0] / 255.0 if img.dtype == np.uint8 else img[0, 0, 0], np.float32)

    def quantise(self, img):
        self.calls.append(("quantise",))
        return (np.clip(img, 0, 1) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)

    def quantise_render(self, img):
        self.calls.append(("quantise_render",))
        return (img.astype(np.float64) * 255 + 0.5).astype(np.uint8)

    def lerp(self, a, b, w):
        self.calls.append(("lerp", w))
        return a + np.float32(w) * (b - a)

    def stack(self, imgs):
        self.calls.append(("stack", len(imgs)))
        return np.stack(imgs)

    def to_host(self, t):
        self.calls.append(("to_host",))
        return np.asarray(t)

    def sync(self):
        self.calls.append(("sync",))


class _SegEngines(_TodayEngines):
    def mask(self, x):
        self.calls.append(("mask", _ident(x), tuple(np.asarray(x).shape)))
        return np.asarray(x)

    def open_atlas(self, resx, resy, n, config, two_layer=False):
        import aiod_amd
        self.calls.append(("open_atlas", resx, resy, n, two_layer))
        self.log.append(("atlas_open", n, two_layer))
        return _Atlas(self.log, aiod_amd.default_config(resx, resy, n, config, two_layer=two_layer))

    def inputs(self, frames, flows12, flows21, resy, resx, masks=None):
        self.calls.append(("inputs", [_ident(f) for f in frames], None if masks is None else [_ident(m) for m in masks]))
        t = (None, [_ident(f) for f in frames], None, [f[1] for f in flows21], [f[1] for f in flows12])
        return t if masks is None else t + ([_ident(m) for m in masks],)


def _frames(n):
    return [np.full((H, W, 3), i, np.uint8) for i in range(n)]


def _masks(n, h=5, w=7):
    return [np.full((h, w), 100 + i, np.uint8) for i in range(n)]


def _deflicker(E, **kw):
    import aiod_amd
    return aiod_amd.Deflicker(None, None, None, config=SMALL, down=4, seed=7, engines=E, **kw)


# ---- a masks=None run: exactly the engine calls of before ---------------------------------------------------------------------
def test_single_atlas_run_makes_exactly_the_engine_calls_it_made():
    import aiod_amd
    E = _TodayEngines()
    res = _deflicker(E).run(_frames(3))
    per_frame = [("resize", H, W), ("resize", H, W), ("resize", H, W), ("quantise",)]      # content, style, `final` back to (h, w), its u8
    assert E.calls == [
        ("frame", 0), ("open_flow", H, W),
        ("frame", 1), ("resize_flow", 1, 2, 3), ("resize_flow", 100, 2, 3),
        ("frame", 2), ("resize_flow", 102, 2, 3), ("resize_flow", 201, 2, 3),
        ("sync",),
        ("open_atlas", 3, 2, 3),
        ("inputs", [0, 1, 2], [1, 102], [100, 201], 2, 3),
        ("sync",),
        ("open_filter", H, W)] + per_frame * 3 + [
        ("sync",),
        ("to_host",), ("to_host",), ("to_host",)]
    uploads = [e for e in E.log if e[0] == "upload"]
    assert len(uploads) == 1 and len(uploads[0]) == 1 + 5                  # upload_video with its five tensors, no mask_frames
    assert [e[1] for e in E.log if e[0] == "load"] == [aiod_amd.NET_MAPPING1, aiod_amd.NET_ATLAS]
    assert len([e for e in E.log if e[0] == "pretrain"]) == 1
    assert res["two_layer"] is False and res["final"].shape == (3, H, W, 3)


def test_single_atlas_windows_with_overlap_on_todays_signatures():
    E = _TodayEngines()
    res = _deflicker(E, window_overlap=1).run(_frames(9), keep=("final", "stage1"))
    assert res["windows"] == [(0, 5), (4, 9)] and res["two_layer"] is False
    assert [c for c in E.calls if c[0] == "open_atlas"] == [("open_atlas", 3, 2, 5)] * 2


# ---- masks given: sliced per window, the two-layer arguments reach the engines ------------------------------------------------
@pytest.mark.parametrize("overlap,windows", [(0, [(0, 5), (5, 9)]), (1, [(0, 5), (4, 9)])])
def test_masks_are_sliced_per_window_like_the_frames(overlap, windows):
    import aiod_amd
    E = _SegEngines()
    res = _deflicker(E, window_overlap=overlap).run(_frames(9), masks=_masks(9), keep=("final", "stage1"))
    assert res["windows"] == windows and res["two_layer"] is True and res["final"].shape == (9, H, W, 3)
    # every mask uploaded once, in order, before the first frame, at its own size
    assert [c for c in E.calls if c[0] in ("mask", "frame")][:10] == [("mask", 100 + i, (5, 7)) for i in range(9)] + [("frame", 0)]
    assert [c for c in E.calls if c[0] == "open_atlas"] == [("open_atlas", 3, 2, b - a, True) for a, b in windows]
    assert [c for c in E.calls if c[0] == "inputs"] == [("inputs", list(range(a, b)), list(range(100 + a, 100 + b))) for a, b in windows]
    uploads = [e for e in E.log if e[0] == "upload"]
    for (a, b), up in zip(windows, uploads):
        assert len(up) == 1 + 6 and up[1] == list(range(a, b)) and up[6] == list(range(100 + a, 100 + b))      # mask_frames is the sixth tensor
    # the two-layer start: four nets in the reference's construction order, both pre-train jobs, per window
    assert [e[1] for e in E.log if e[0] == "load"] == [aiod_amd.NET_MAPPING1, aiod_amd.NET_MAPPING2, aiod_amd.NET_ATLAS, aiod_amd.NET_ALPHA] * 2
    assert [e[1] for e in E.log if e[0] == "pretrain"] == [aiod_amd.NET_MAPPING1, aiod_amd.NET_MAPPING2] * 2
    names = [e[0] for e in E.log]
    assert names.count("atlas_close") == 2 and names.count("filter_close") == 1
    # stage 2 never sees the masks: frame i is styled by frame i
    assert [int(f[0, 0, 0]) for f in res["final"]] == list(range(9))


def test_window_k_draws_what_a_stand_alone_two_layer_run_with_seed_plus_k_draws():
    import aiod_amd
    draws = []
    for lo, seed in ((0, 7), (5, 8)):
        E = _SegEngines()
        aiod_amd.Deflicker(None, None, None, config=SMALL, seed=seed, engines=E).run(_frames(9)[lo:], masks=_masks(9)[lo:])
        draws.append([e[-1] for e in E.log if e[0] in ("pretrain", "train")])
    assert len(draws[0]) == 2 * (2 + 2) and draws[0][4:] == draws[1]


def test_mask_forms_iterator_array_and_channels():
    E = _SegEngines()
    d = _deflicker(E)
    want = [("inputs", [0, 1, 2], [100, 101, 102])]
    for masks in (iter(_masks(3)), np.stack(_masks(3)), np.stack(_masks(3))[..., None].repeat(3, -1), [m[:, :, None] for m in _masks(3)]):
        del E.calls[:]
        assert d.run(iter(_frames(3)), masks=masks)["two_layer"] is True
        assert [c for c in E.calls if c[0] == "inputs"] == want


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_mask_errors_name_the_cause_before_any_fit():
    E = _SegEngines()
    d = _deflicker(E)
    with pytest.raises(ValueError, match="3 masks for 4 frames"):
        d.run(_frames(4), masks=_masks(3))
    assert E.calls == []                                                   # both lengths known: refused before any work
    with pytest.raises(ValueError, match="3 masks for 4 frames"):
        d.run(iter(_frames(4)), masks=iter(_masks(3)))                    # lengths unknown until read: refused after RAFT, before stage 1
    with pytest.raises(ValueError, match="5 masks for 4 frames"):
        d.run(iter(_frames(4)), masks=iter(_masks(5)))
    bad = _masks(4)
    bad[1] = bad[1].astype(np.float32)
    with pytest.raises(ValueError, match="mask 1 must be uint8, got float32"):
        d.run(_frames(4), masks=bad)
    with pytest.raises(ValueError, match="masks must be uint8, got float32"):
        d.run(_frames(4), masks=np.stack(_masks(4)).astype(np.float32))
    with pytest.raises(ValueError, match=r"masks must be \(N, Hm, Wm\) or \(N, Hm, Wm, C\) uint8, got \(4, 5\)"):
        d.run(_frames(4), masks=np.zeros((4, 5), np.uint8))
    with pytest.raises(ValueError, match=r"masks must be \(N, Hm, Wm\) or \(N, Hm, Wm, C\) uint8, got \(4, 5, 7, 1, 1\)"):
        d.run(_frames(4), masks=np.zeros((4, 5, 7, 1, 1), np.uint8))
    with pytest.raises(ValueError, match=r"mask 2 must be \(Hm, Wm\) or \(Hm, Wm, C\), got \(7,\)"):
        d.run(_frames(4), masks=_masks(2) + [np.zeros(7, np.uint8), _masks(1)[0]])
    names = [e[0] for e in E.log]
    assert "atlas_open" not in names and names.count("raft_close") == 2    # no fit was started; every RAFT handle that was opened is closed
    assert d.run(_frames(4), masks=_masks(4))["final"].shape == (4, H, W, 3)


# ---- CLI ------------------------------------------------------------------------------------------------------------------------
def test_masks_dir_listing_and_decoding(tmp_path):
    from PIL import Image
    from aiod_amd import deflicker
    d = tmp_path / "clip_seg"
    d.mkdir()
    for name in ("00003.jpg", "00000.png", "00002.png", "00001.jpg", "00004.png"):
        Image.fromarray(np.full((5, 7), 200, np.uint8)).save(str(d / name))
    (d / "notes.txt").write_text("not a mask")
    assert [p.name for p in deflicker.list_masks(str(d), 4)] == ["00000.png", "00001.jpg", "00002.png", "00003.jpg"]      # sorted together, the first N
    with pytest.raises(SystemExit) as e:
        deflicker.list_masks(str(d), 6)
    assert "5 masks" in str(e.value) and "6 frames" in str(e.value) and str(d) in str(e.value)
    Image.fromarray(np.dstack([np.full((5, 7), v, np.uint8) for v in (9, 50, 90)])).save(str(d / "rgb.png"))
    m = deflicker.decode_mask(d / "rgb.png")
    assert m.dtype == np.uint8 and m.shape == (5, 7, 1) and (m == 9).all()                                                 # channel 0
    assert deflicker.decode_mask(d / "00000.png").shape == (5, 7, 1)
    Image.fromarray(np.full((5, 7), 40000, np.uint16)).save(str(d / "deep.png"))
    with pytest.raises(SystemExit, match="deep.png: only 8-bit masks are handled"):
        deflicker.decode_mask(d / "deep.png")


def test_cli_flag_and_help(capsys):
    from aiod_amd import deflicker
    assert deflicker.parse_args(["--frames_dir", "x"]).masks_dir is None
    assert deflicker.parse_args(["--frames_dir", "x", "--masks_dir", "x_seg"]).masks_dir == "x_seg"
    with pytest.raises(SystemExit):
        deflicker.parse_args(["--help"])
    text = re.sub(r"\s+", " ", capsys.readouterr().out)
    assert "--masks_dir" in text and "<frames_dir>_seg" in text and "mask preprocessors" in text and "does not run" in text


def _cli(monkeypatch, tmp_path, engines, n_frames=3, n_masks=3):
    """deflicker.main on a PNG clip with the device replaced by stub engines."""
    import torch
    from PIL import Image
    from aiod_amd import deflicker
    clip, seg = tmp_path / "clip", tmp_path / "clip_seg"
    clip.mkdir(exist_ok=True), seg.mkdir(exist_ok=True)
    for i, f in enumerate(_frames(n_frames)):
        Image.fromarray(f).save(str(clip / ("%05d.png" % i)))
    for i, m in enumerate(_masks(n_masks)):
        Image.fromarray(m).save(str(seg / ("%05d.png" % i)))
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps(SMALL))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(deflicker, "load_checkpoints", lambda opts: (None, None, None))
    monkeypatch.setattr(deflicker, "DeviceEngines", lambda *a, **k: engines)
    return ["--frames_dir", str(clip), "--out", str(tmp_path / "out"), "--config", str(cfg), "--seed", "7"], seg


def test_cli_record_and_wiring(monkeypatch, tmp_path):
    from aiod_amd import deflicker
    E = _SegEngines()
    argv, seg = _cli(monkeypatch, tmp_path, E)
    assert deflicker.main(argv + ["--masks_dir", str(seg)]) == 0
    rec = json.load(open(tmp_path / "out" / "deflicker.json"))
    assert rec["two_layer"] is True and rec["masks_dir"] == str(seg) and rec["frames"] == 3 and rec["windows"] == [[0, 3]]
    assert [c for c in E.calls if c[0] == "mask"] == [("mask", 100 + i, (5, 7, 1)) for i in range(3)]
    assert sorted(os.listdir(tmp_path / "out" / "final" / "output")) == ["%05d.png" % i for i in range(3)]
    E1 = _TodayEngines()
    monkeypatch.setattr(deflicker, "DeviceEngines", lambda *a, **k: E1)
    assert deflicker.main(argv) == 0                                       # without the flag: one atlas, today's engine signatures
    rec = json.load(open(tmp_path / "out" / "deflicker.json"))
    assert rec["two_layer"] is False and rec["masks_dir"] is None


def test_cli_mask_errors(monkeypatch, tmp_path):
    from PIL import Image
    from aiod_amd import deflicker
    E = _SegEngines()
    argv, seg = _cli(monkeypatch, tmp_path, E, n_frames=4, n_masks=3)
    with pytest.raises(SystemExit) as e:
        deflicker.main(argv + ["--masks_dir", str(seg)])
    assert "3 masks" in str(e.value) and "4 frames" in str(e.value) and str(seg) in str(e.value)
    assert E.calls == []
    Image.fromarray(np.full((5, 7), 40000, np.uint16)).save(str(seg / "00001.png"))
    Image.fromarray(np.full((5, 7), 1, np.uint8)).save(str(seg / "00003.png"))
    with pytest.raises(SystemExit, match="00001.png: only 8-bit masks are handled"):
        deflicker.main(argv + ["--masks_dir", str(seg)])
    assert "atlas_open" not in [e[0] for e in E.log]
