"""Host-side checks of the key-mask route (no GPU): the planner of masks.py, the properties of the numpy restatement of the kernels
(tests/maskprop_ref.py) that the GPU tests hold the kernels to, `Deflicker.run(frames, mask_keys=...)` with stub engines in the style of
tests/test_deflicker_seg_host.py (whose stubs are imported, not changed), the CLI flags and the exports."""
import json
import os
import re

import numpy as np
import pytest

import maskprop_ref as R
import test_deflicker_seg_host as SH

H, W = SH.H, SH.W
F = np.float32


# ---- the planner ---------------------------------------------------------------------------------------------------------------
def test_plan_one_key_is_two_one_sided_chains():
    from aiod_amd import plan_mask_propagation
    assert plan_mask_propagation(5, [2]) == [[("key", 2), ("step", 2, 1), ("step", 1, 0), ("step", 2, 3), ("step", 3, 4)]]
    assert plan_mask_propagation(3, {0: None}) == [[("key", 0), ("step", 0, 1), ("step", 1, 2)]]
    assert plan_mask_propagation(1, [0]) == [[("key", 0)]]


def test_plan_keys_at_both_ends_walks_the_interval_once_each_way():
    from aiod_amd import plan_mask_propagation
    assert plan_mask_propagation(5, [4, 0]) == [[
        ("key", 0), ("key", 4),
        ("step", 0, 1), ("step", 1, 2), ("step", 2, 3),
        ("step", 4, 3), ("step", 3, 2), ("step", 2, 1),
        ("blend", 0, 1, 4), ("blend", 0, 2, 4), ("blend", 0, 3, 4)]]
    steps = plan_mask_propagation(101, [0, 100])[0]
    assert len([s for s in steps if s[0] == "step"]) == 2 * 99      # once per key interval and direction, not once per frame
    assert plan_mask_propagation(2, [0, 1]) == [[("key", 0), ("key", 1)]]      # a key on every frame: no step at all


def test_plan_interior_key():
    from aiod_amd import plan_mask_propagation
    assert plan_mask_propagation(6, [1, 3]) == [[
        ("key", 1), ("key", 3),
        ("step", 1, 0),
        ("step", 1, 2), ("step", 3, 2), ("blend", 1, 2, 3),
        ("step", 3, 4), ("step", 4, 5)]]


def test_plan_two_shots_never_cross_the_cut():
    from aiod_amd import plan_mask_propagation
    plans = plan_mask_propagation(7, [1, 6], shots=[(0, 4), (4, 7)])
    assert plans == [[("key", 1), ("step", 1, 0), ("step", 1, 2), ("step", 2, 3)],
                     [("key", 6), ("step", 6, 5), ("step", 5, 4)]]
    pairs = {frozenset(s[1:3]) for p in plans for s in p if s[0] == "step"}
    assert frozenset((3, 4)) not in pairs


def test_plan_refusals_name_the_cause():
    from aiod_amd import plan_mask_propagation
    with pytest.raises(ValueError, match="no key masks"):
        plan_mask_propagation(5, [])
    with pytest.raises(ValueError, match=r"key 5 is outside 0\.\.4 \(the clip has 5 frames\)"):
        plan_mask_propagation(5, [0, 5])
    with pytest.raises(ValueError, match=r"key -1 is outside 0\.\.4"):
        plan_mask_propagation(5, [-1])
    with pytest.raises(ValueError, match=r"shot 1 \(frames 4\.\.6\) holds no key mask"):
        plan_mask_propagation(7, [1], shots=[(0, 4), (4, 7)])


# ---- the restatement's properties ------------------------------------------------------------------------------------------------
def _blob(h, w, cx, cy):
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.clip(1.5 - np.hypot(xs - cx, ys - cy) / 4.0, 0, 1).astype(F)


@pytest.mark.parametrize("dx,dy", [(2, -1), (-3, 2), (0, 0)])
def test_integer_translation_is_reproduced_exactly(dx, dy):
    """Frame t is frame s moved by (dx, dy): flow t -> s is (-dx, -dy) everywhere, flow s -> t is (dx, dy).  Where the source pixel lies
    in the frame the value arrives exactly with confidence 1; elsewhere the source's value at the target's own position is held, c = 0."""
    h, w = 13, 17
    m_s = _blob(h, w, 8, 6)
    f_ts = np.tile(np.array([-dx, -dy], F), (h, w, 1))
    f_st = np.tile(np.array([dx, dy], F), (h, w, 1))
    m_t, c_t = R.step(m_s, np.ones((h, w), F), f_ts, f_st)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    sx, sy = xs - dx, ys - dy
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    want = np.where(inside, m_s[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)], m_s)
    assert np.array_equal(m_t, want) and np.array_equal(c_t, inside.astype(F))
    assert inside.all() == (dx == 0 and dy == 0)


def test_constant_mask_stays_constant_and_blend_of_equals_is_that_input():
    rng = np.random.default_rng(0)
    h, w = 9, 11
    f_ts, f_st = (rng.uniform(-3, 3, (h, w, 2)).astype(F) for _ in range(2))
    for v in (0.0, 1.0, 0.25):      # 0.25 (1 - a) + 0.25 a is exact only for some a: constants 0 and 1 exactly, 0.25 to a rounding
        m_t, c_t = R.step(np.full((h, w), v, F), rng.random((h, w)).astype(F), f_ts, f_st)
        assert np.abs(m_t - F(v)).max() <= (0 if v in (0.0, 1.0) else 2 ** -24)
    m, cf, cb = rng.random((h, w)).astype(F), rng.random((h, w)).astype(F), rng.random((h, w)).astype(F)
    cf[0], cb[0] = 0, 0                                      # a row where neither chain has confidence: the distance-weighted mean
    out = R.blend(m, cf, m, cb, 2, 5, 9)
    assert np.abs(out - m).max() <= 2 ** -23                 # (wf m + wb m) / (wf + wb): three roundings of a value <= 1
    assert np.array_equal(R.blend(m, np.ones_like(m), m, np.zeros_like(m), 0, 1, 2), m)      # one-sided confidence, unit weights: exact


def test_restatement_is_within_its_rounding_of_the_fp64_twin():
    """Derived, not measured: a bil is 3 lerps of 3 roundings each on values <= 1, the blend at most 7 more: fewer than 16 roundings of
    2^-24 relative each on values <= 1, so < 16 * 2^-24 < 1e-6.  The round-trip test may fall the other way only within its own rounding
    of the bound: such pixels (|norm^2 - thresh^2| < 1e-4 in fp64) are left out of the comparison, and there must be few."""
    rng = np.random.default_rng(1)
    h, w = 40, 56
    m_s, c_s = rng.random((h, w)).astype(F), rng.random((h, w)).astype(F)
    f_ts = rng.uniform(-2, 2, (h, w, 2)).astype(F)
    f_st = (-f_ts + rng.uniform(-0.9, 0.9, (h, w, 2))).astype(F)
    m32, c32 = R.step(m_s, c_s, f_ts, f_st)
    m64, c64, ok64, margin = R.step64(m_s, c_s, f_ts, f_st)
    sure = margin >= 1e-4
    assert sure.mean() > 0.99 and 0.2 < ok64.mean() < 0.9 and 0.02 < (c32 == 0).mean() < 0.8      # both branches are exercised
    assert np.abs(m32 - m64)[sure].max() < 1e-6 and np.abs(c32 - c64)[sure].max() < 1e-6
    b32 = R.blend(m32, c32, m_s, c_s, 3, 4, 9)
    assert np.abs(b32 - R.blend64(m32, c32, m_s, c_s, 3, 4, 9)).max() < 1e-6
    assert b32.min() >= 0 and b32.max() <= 1


def test_restatement_holds_out_of_frame_and_non_finite_pixels():
    h, w = 5, 6
    rng = np.random.default_rng(2)
    m_s = rng.random((h, w)).astype(F)
    f_ts, f_st = np.zeros((h, w, 2), F), np.zeros((h, w, 2), F)
    f_ts[0, 0] = (np.nan, 0); f_ts[0, 1] = (np.inf, 0); f_ts[0, 2] = (0, -np.inf); f_ts[1, 0] = (-0.5, 0); f_ts[4, 5] = (0, 0.25)
    f_ts[2, 2] = (3, 0)                                      # lands exactly on w - 1: inside, x1 clamped
    f_st[2, 5] = (-3, 0)
    f_st[3, 3] = (np.nan, 0)                                 # the round trip is NaN: not consistent
    m_t, c_t = R.step(m_s, np.ones((h, w), F), f_ts, f_st)
    held = np.zeros((h, w), bool)
    held[0, 0] = held[0, 1] = held[0, 2] = held[1, 0] = held[4, 5] = held[3, 3] = True
    held[3, 2] = held[2, 3] = True                           # (3, 3) is their x1 / y1 tap: NaN times a zero weight is NaN
    held[2, 5] = True                                        # its own round trip is 3 pixels long
    assert np.array_equal(c_t, (~held).astype(F)) and np.array_equal(m_t[held], m_s[held])
    moved = np.zeros((h, w), bool)
    moved[2, 2] = True
    assert m_t[2, 2] == m_s[2, 5] and np.array_equal(m_t[~held & ~moved], m_s[~held & ~moved])      # zero flow elsewhere: the pixel itself


def test_propagate_restatement_on_a_translating_clip():
    """Keys at both ends of a clip that moves one pixel per frame: inside the frame every propagated mask is the moved blob."""
    n, h, w = 5, 12, 20
    masks = [_blob(h, w, 6 + t, 6) for t in range(n)]
    f12 = [np.tile(np.array([1, 0], F), (h, w, 1)) for _ in range(n - 1)]
    f21 = [np.tile(np.array([-1, 0], F), (h, w, 1)) for _ in range(n - 1)]
    out = R.propagate({0: masks[0], 4: masks[4]}, f12, f21)
    assert out.shape == (n, h, w) and np.array_equal(out[0], masks[0]) and np.array_equal(out[4], masks[4])
    for t in range(1, 4):
        assert np.abs(out[t] - masks[t])[:, 4:w - 4].max() <= 2 ** -23
    one = R.propagate({2: masks[2]}, f12, f21)
    assert np.array_equal(one[2], masks[2]) and np.array_equal(one[4][:, 2:], masks[4][:, 2:]) and np.array_equal(one[0][:, :w - 2], masks[0][:, :w - 2])


# ---- Deflicker with stub engines ----------------------------------------------------------------------------------------------
class _KeyEngines(SH._SegEngines):
    """_SegEngines plus the two engine methods and the one argument of the key-mask route."""

    def resize_mask(self, mask, h, w):
        self.calls.append(("resize_mask", SH._ident(mask), tuple(np.asarray(mask).shape), h, w))
        return np.full((h, w), SH._ident(mask), F)

    def propagate_masks(self, keys, flows12, flows21, shots, thresh=1.0):
        self.calls.append(("propagate_masks", {k: (int(v[0, 0]), v.shape) for k, v in keys.items()}, [f and f[1] for f in flows12],
                           [f and f[1] for f in flows21], list(shots), thresh))
        n = len(flows12) + 1
        h, w = next(iter(keys.values())).shape
        return np.stack([np.full((h, w), (200 + i) / 255.0, F) for i in range(n)])

    def inputs(self, frames, flows12, flows21, resy, resx, masks=None, mask_frames=None):
        if mask_frames is None:
            return super().inputs(frames, flows12, flows21, resy, resx, masks=masks)
        assert masks is None
        planes = [int(round(float(m[0, 0]) * 255)) for m in mask_frames]
        self.calls.append(("inputs", [SH._ident(f) for f in frames], ("mask_frames", planes)))
        return (None, [SH._ident(f) for f in frames], None, [f[1] for f in flows21], [f[1] for f in flows12], planes)


def _keys(*idx):
    return {i: np.full((5, 7), 100 + i, np.uint8) for i in idx}


def test_mask_keys_make_one_propagation_call_and_every_window_gets_its_slice():
    import aiod_amd
    E = _KeyEngines()
    res = SH._deflicker(E).run(SH._frames(9), mask_keys=_keys(8, 0, 4), keep=("final", "masks"))
    windows = [(0, 5), (5, 9)]
    assert res["windows"] == windows and res["two_layer"] is True and res["mask_keys"] == [0, 4, 8] and res["mask_thresh"] == 1.0
    # the keys are uploaded before the first frame, in index order, at their own size; resized after the flows; one propagation call
    assert [c for c in E.calls if c[0] in ("mask", "frame")][:4] == [("mask", 100, (5, 7)), ("mask", 104, (5, 7)), ("mask", 108, (5, 7)), ("frame", 0)]
    names = [c[0] for c in E.calls]
    assert names.count("propagate_masks") == 1 and names.count("resize_mask") == 3
    assert max(i for i, c in enumerate(names) if c == "resize_flow") < names.index("resize_mask") < names.index("propagate_masks") < names.index("open_atlas")
    assert [c for c in E.calls if c[0] == "resize_mask"] == [("resize_mask", 100 + i, (5, 7), 2, 3) for i in (0, 4, 8)]
    call = [c for c in E.calls if c[0] == "propagate_masks"][0]
    assert call[1] == {i: (100 + i, (2, 3)) for i in (0, 4, 8)} and call[4] == [(0, 9)] and call[5] == 1.0
    assert call[2] == [100 * i + i + 1 for i in range(8)] and call[3] == [100 * (i + 1) + i for i in range(8)]      # the stage-1-size flows, both directions
    assert [c for c in E.calls if c[0] == "inputs"] == [("inputs", list(range(a, b)), ("mask_frames", list(range(200 + a, 200 + b)))) for a, b in windows]
    assert [c for c in E.calls if c[0] == "open_atlas"] == [("open_atlas", 3, 2, b - a, True) for a, b in windows]
    uploads = [e for e in E.log if e[0] == "upload"]
    for (a, b), up in zip(windows, uploads):
        assert len(up) == 1 + 6 and up[6] == list(range(200 + a, 200 + b))      # mask_frames is the sixth tensor
    assert [e[1] for e in E.log if e[0] == "load"] == [aiod_amd.NET_MAPPING1, aiod_amd.NET_MAPPING2, aiod_amd.NET_ATLAS, aiod_amd.NET_ALPHA] * 2
    assert res["masks"].shape == (9, 2, 3) and res["masks"].dtype == F and np.array_equal(res["masks"][:, 0, 0], (np.arange(200, 209) / 255.0).astype(F))
    assert "masks" in res["seconds"] and res["final"].shape == (9, H, W, 3)


def test_mask_keys_with_cuts_pass_the_shots_and_a_non_default_thresh():
    E = _KeyEngines()
    res = SH._deflicker(E, cuts=[4], mask_thresh=0.5).run(SH._frames(7), mask_keys=_keys(1, 6))
    call = [c for c in E.calls if c[0] == "propagate_masks"][0]
    assert call[4] == [(0, 4), (4, 7)] and call[5] == 0.5 and call[2][3] is None and call[3][3] is None
    assert res["shots"] == [(0, 4), (4, 7)] and res["mask_keys"] == [1, 6] and res["mask_thresh"] == 0.5
    assert [c[2] for c in E.calls if c[0] == "inputs"] == [("mask_frames", [200, 201, 202, 203]), ("mask_frames", [204, 205, 206])]


def test_masks_only_stops_after_the_propagation():
    E = _KeyEngines()
    res = SH._deflicker(E).run(SH._frames(4), mask_keys=_keys(0), masks_only=True)
    assert res["masks"].shape == (4, 2, 3) and res["mask_keys"] == [0] and "final" not in res and set(res["seconds"]) == {"decode + flow", "masks", "total"}
    names = [c[0] for c in E.calls]
    assert "open_atlas" not in names and "open_filter" not in names and names.count("propagate_masks") == 1


def test_key_route_refusals_come_before_any_fit():
    import aiod_amd
    E = _KeyEngines()
    d = SH._deflicker(E)
    with pytest.raises(ValueError, match="masks and mask_keys are mutually exclusive"):
        d.run(SH._frames(4), masks=SH._masks(4), mask_keys=_keys(0))
    with pytest.raises(ValueError, match="no key masks"):
        d.run(SH._frames(4), mask_keys={})
    with pytest.raises(ValueError, match=r"key 4 is outside 0\.\.3"):
        d.run(SH._frames(4), mask_keys=_keys(0, 4))
    with pytest.raises(ValueError, match="mask 2 must be uint8, got float32"):
        d.run(SH._frames(4), mask_keys={2: np.zeros((5, 7), F)})
    with pytest.raises(ValueError, match=r"mask 1 must be \(Hm, Wm\) or \(Hm, Wm, C\), got \(7,\)"):
        d.run(SH._frames(4), mask_keys={1: np.zeros(7, np.uint8)})
    with pytest.raises(ValueError, match="frame index 'a' is not an integer"):
        d.run(SH._frames(4), mask_keys={"a": np.zeros((5, 7), np.uint8)})
    with pytest.raises(ValueError, match="mask_keys must be a .* mapping, got list"):
        d.run(SH._frames(4), mask_keys=[np.zeros((5, 7), np.uint8)])
    with pytest.raises(ValueError, match=r"shot 1 \(frames 4\.\.6\) holds no key mask"):
        SH._deflicker(E, cuts=[4]).run(SH._frames(7), mask_keys=_keys(1))
    with pytest.raises(ValueError, match="keep \"masks\" and masks_only belong to the key-mask route"):
        d.run(SH._frames(4), keep=("final", "masks"))
    assert E.calls == []                                                   # the clip has a length: all of it before the first upload
    with pytest.raises(ValueError, match=r"key 4 is outside 0\.\.3"):
        d.run(iter(SH._frames(4)), mask_keys=_keys(0, 4))                 # an iterator: after the decode, still before any fit
    with pytest.raises(ValueError, match="Deflicker: mask_thresh: .*finite and > 0"):
        SH._deflicker(E, mask_thresh=0.0)
    with pytest.raises(ValueError, match="mask_keys needs an engine with propagate_masks; _SegEngines has none"):
        SH._deflicker(SH._SegEngines()).run(SH._frames(4), mask_keys=_keys(0))
    names = [e[0] for e in E.log]
    assert "atlas_open" not in names and "propagate_masks" not in [c[0] for c in E.calls]
    assert aiod_amd.Deflicker(None, None, None, config=SH.SMALL, engines=E).run(SH._frames(4), mask_keys=_keys(0))["final"].shape == (4, H, W, 3)


def test_stubs_without_the_new_method_run_the_old_routes_with_their_old_calls():
    """The single-atlas and the masks= routes on engines from before this route: the call lists a _KeyEngines run of the same route makes,
    minus nothing — no resize_mask, no propagate_masks, no mask_frames argument."""
    old, new = SH._TodayEngines(), _KeyEngines()
    r_old, r_new = SH._deflicker(old).run(SH._frames(3)), SH._deflicker(new).run(SH._frames(3))
    assert r_old["mask_keys"] is None and r_old["two_layer"] is False and np.array_equal(r_old["final"], r_new["final"])
    assert [c[0] for c in old.calls] == [c[0] for c in new.calls]
    assert old.calls[:3] == [("frame", 0), ("open_flow", H, W), ("frame", 1)] and ("inputs", [0, 1, 2], [1, 102], [100, 201], 2, 3) in old.calls
    seg, key = SH._SegEngines(), _KeyEngines()
    r_seg = SH._deflicker(seg).run(SH._frames(9), masks=SH._masks(9))
    SH._deflicker(key).run(SH._frames(9), masks=SH._masks(9))
    assert seg.calls == key.calls and r_seg["two_layer"] is True and r_seg["mask_keys"] is None
    assert not {"resize_mask", "propagate_masks"} & {c[0] for c in key.calls}


# ---- CLI -----------------------------------------------------------------------------------------------------------------------
def _write_keys(folder, names):
    from PIL import Image
    folder.mkdir(exist_ok=True)
    for name, v in names.items():
        Image.fromarray(np.full((5, 7), v, np.uint8)).save(str(folder / name))


def test_cli_stems_record_and_mask_files(monkeypatch, tmp_path):
    from aiod_amd import deflicker
    E = _KeyEngines()
    argv, _ = SH._cli(monkeypatch, tmp_path, E, n_frames=4)
    _write_keys(tmp_path / "keys", {"00003.jpg": 103, "00000.png": 100})
    assert deflicker.main(argv + ["--mask_keys_dir", str(tmp_path / "keys"), "--mask_thresh", "2"]) == 0
    rec = json.load(open(tmp_path / "out" / "deflicker.json"))
    assert rec["two_layer"] is True and rec["mask_keys"] == [0, 3] and rec["mask_thresh"] == 2.0 and rec["masks_dir"] is None
    assert rec["mask_keys_dir"] == str(tmp_path / "keys") and rec["masks_only"] is False and rec["frames"] == 4
    assert [c[:3] for c in E.calls if c[0] == "mask"] == [("mask", 100, (5, 7, 1)), ("mask", 103, (5, 7, 1))]      # a key belongs to the frame with its stem
    assert [c[5] for c in E.calls if c[0] == "propagate_masks"] == [2.0]
    assert not (tmp_path / "out" / "masks").exists()                      # masks/ comes with --keep_intermediates or --masks_only
    assert sorted(os.listdir(tmp_path / "out" / "final" / "output")) == ["%05d.png" % i for i in range(4)]


def test_cli_unmatched_stem_and_flag_errors(monkeypatch, tmp_path, capsys):
    from aiod_amd import deflicker
    E = _KeyEngines()
    argv, seg = SH._cli(monkeypatch, tmp_path, E, n_frames=4)
    _write_keys(tmp_path / "keys", {"00001.png": 101, "frame7.png": 1})
    with pytest.raises(SystemExit) as e:
        deflicker.main(argv + ["--mask_keys_dir", str(tmp_path / "keys")])
    assert "frame7.png" in str(e.value) and "no frame is named frame7.png" in str(e.value)
    (tmp_path / "empty").mkdir()
    with pytest.raises(SystemExit, match="no key masks"):
        deflicker.main(argv + ["--mask_keys_dir", str(tmp_path / "empty")])
    _write_keys(tmp_path / "two", {"00001.png": 1, "00001.jpg": 2})
    with pytest.raises(SystemExit, match="both key masks of frame 1"):
        deflicker.main(argv + ["--mask_keys_dir", str(tmp_path / "two")])
    assert E.calls == []
    for extra, text in ((["--mask_keys_dir", "k", "--masks_dir", str(seg)], "mutually exclusive"), (["--masks_only"], "options of --mask_keys_dir"),
                        (["--mask_thresh", "1"], "options of --mask_keys_dir")):
        with pytest.raises(SystemExit):
            deflicker.parse_args(["--frames_dir", "x"] + extra)
        assert text in capsys.readouterr().err
    # with --video the stem is the decimal frame index
    _write_keys(tmp_path / "keys2", {"7.png": 1, "00012.png": 2})
    keys = deflicker.list_mask_keys(str(tmp_path / "keys2"))
    assert sorted(keys) == [7, 12] and keys[12].name == "00012.png"
    with pytest.raises(SystemExit, match="the stem of a key mask is the decimal frame index, got 'frame7'"):
        deflicker.list_mask_keys(str(tmp_path / "keys"))


def test_cli_masks_only_needs_the_flow_checkpoint_alone(monkeypatch, tmp_path):
    import torch
    from PIL import Image
    from aiod_amd import deflicker
    E = _KeyEngines()
    argv, _ = SH._cli(monkeypatch, tmp_path, E, n_frames=3)
    _write_keys(tmp_path / "keys", {"00001.png": 101})
    assert deflicker.main(argv + ["--mask_keys_dir", str(tmp_path / "keys"), "--masks_only"]) == 0
    out = tmp_path / "out"
    assert sorted(os.listdir(out / "masks")) == ["%05d.png" % i for i in range(3)] and not (out / "final").exists()
    assert (np.asarray(Image.open(out / "masks" / "00002.png")) == 202).all()
    rec = json.load(open(out / "deflicker.json"))
    assert rec["masks_only"] is True and rec["mask_keys"] == [1] and rec["frames"] == 3 and "windows" not in rec and "psnr" not in rec
    assert "open_atlas" not in [c[0] for c in E.calls] and "open_filter" not in [c[0] for c in E.calls]
    torch.save({"w": torch.zeros(1)}, str(tmp_path / "raft.pth"))
    opts = deflicker.parse_args(["--frames_dir", "x", "--mask_keys_dir", "k", "--masks_only", "--model", str(tmp_path / "raft.pth"),
                                 "--ckpt_filter", str(tmp_path / "absent1.pth"), "--ckpt_local", str(tmp_path / "absent2.pth")])
    monkeypatch.undo()
    sds = deflicker.load_checkpoints(opts)
    assert list(sds[0]) == ["w"] and sds[1] is None and sds[2] is None
    opts.masks_only = False
    with pytest.raises(SystemExit, match="absent1.pth not found"):
        deflicker.load_checkpoints(opts)


def test_run_pipeline_passes_the_key_flags_on_and_refuses_them_without_in_process(capsys):
    from aiod_amd import run_pipeline as RP
    opts = RP.parse_opts(["--video_name", "data/test/X.mp4", "--in_process", "--mask_keys_dir", "data/test/X_keys", "--mask_thresh", "1.5"])
    cmd = RP.build_commands(opts)[-1][1]
    assert "deflicker.py" in cmd and cmd.endswith(" --mask_keys_dir data/test/X_keys --mask_thresh 1.5")
    plain = RP.build_commands(RP.parse_opts(["--video_name", "data/test/X.mp4", "--in_process"]))[-1][1]
    assert "mask" not in plain
    for argv, text in ((["--video_name", "data/test/X.mp4", "--mask_keys_dir", "k"], "they need --in_process"),
                       (["--video_name", "data/test/X.mp4", "--in_process", "--mask_thresh", "2"], "--mask_thresh is an option of --mask_keys_dir"),
                       (["--video_name", "data/test/X.mp4", "--in_process", "--mask_keys_dir", "a b"], "expected a plain file name")):
        with pytest.raises(SystemExit):
            RP.parse_opts(argv)
        assert text in capsys.readouterr().err
    opts.in_process = False
    with pytest.raises(ValueError, match="they need --in_process"):
        RP.build_commands(opts)


# ---- exports ----------------------------------------------------------------------------------------------------------------------
def test_exports_and_abi_names():
    import aiod_amd
    from aiod_amd import masks
    assert {"af_mask_step", "af_mask_blend"} <= set(aiod_amd.atlasfit.ABI_SYMBOLS)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "atlasfit.h")).read()
    assert re.search(r"\bint af_mask_step\(int device_ordinal, const float\* m_s,", hdr) and re.search(r"\bint af_mask_blend\(int device_ordinal, const float\* m_f,", hdr)
    assert aiod_amd.plan_mask_propagation is masks.plan_mask_propagation and aiod_amd.propagate_masks is masks.propagate_masks
    assert aiod_amd.propagate_masks_device is masks.propagate_masks_device
    assert "masks" in aiod_amd.deflicker.KEEP and hasattr(aiod_amd.deflicker.DeviceEngines, "propagate_masks")
