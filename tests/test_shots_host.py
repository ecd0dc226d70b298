"""Host-side checks of the shot-aware pipeline (no GPU): the score, the cut rule and the shot planner of shots.py against written-out
cases, and the order of work of Deflicker.run with cuts, on stub engines (those of tests/test_deflicker_host.py, restated here with
the RAFT slots in the log)."""
import argparse
import importlib.util
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


# ---- cut_scores ----------------------------------------------------------------------------------------------------------------
def _score_loops(sums, counts):
    """The score written out: two passes over the cells per pair, plain Python floats (fp64)."""
    n, gh, gw = sums.shape
    out = []
    for t in range(n - 1):
        a = [[float(sums[t, i, j]) / (256.0 * float(counts[i, j])) for j in range(gw)] for i in range(gh)]
        b = [[float(sums[t + 1, i, j]) / (256.0 * float(counts[i, j])) for j in range(gw)] for i in range(gh)]
        ma = mb = 0.0
        for i in range(gh):
            for j in range(gw):
                ma += a[i][j]
                mb += b[i][j]
        ma, mb = ma / (gh * gw), mb / (gh * gw)
        sab = saa = sbb = 0.0
        for i in range(gh):
            for j in range(gw):
                sab += (a[i][j] - ma) * (b[i][j] - mb)
                saa += (a[i][j] - ma) ** 2
                sbb += (b[i][j] - mb) ** 2
        if saa == 0.0 and sbb == 0.0:
            out.append(1.0)
        elif saa == 0.0 or sbb == 0.0:
            out.append(0.0)
        else:
            out.append(sab / (saa * sbb) ** 0.5)
    return np.array(out)


def test_cut_scores_against_a_double_loop():
    from aiod_amd import cut_scores
    from aiod_amd.shots import cell_counts
    rng = np.random.default_rng(0)
    for (h, w), grid in (((130, 197), (16, 16)), ((33, 70), (64, 64)), ((48, 64), (1, 3)), ((7, 5), (16, 16))):
        counts = cell_counts(h, w, grid)
        assert counts.shape == (min(grid[0], h), min(grid[1], w)) and counts.sum() == h * w and counts.min() >= 1
        sums = rng.integers(0, 65280, (6,) + counts.shape) * counts[None]
        got = cut_scores(sums, counts)
        assert got.dtype == np.float64 and got.shape == (5,)
        assert np.abs(got - _score_loops(sums, counts)).max() <= 1e-12
        assert (np.abs(got) <= 1.0 + 1e-12).all()
    assert cut_scores(sums[:1], counts).shape == (0,)
    with pytest.raises(ValueError, match="cut_scores"):
        cut_scores(sums[0], counts)


def test_cut_scores_ignore_gain_and_offset():
    """What flicker is: a frame-wide gain c and offset d.  Grids a and c * a + d score 1."""
    from aiod_amd import cut_scores
    rng = np.random.default_rng(1)
    counts = np.full((16, 16), 96, np.int64)
    a = rng.integers(2000, 20000, (16, 16)).astype(np.int64)
    for c, d in ((1, 0), (2, 0), (3, 1234), (1, 40000), (5, 7)):
        sums = np.stack([a * counts, (c * a + d) * counts])
        assert abs(cut_scores(sums, counts)[0] - 1.0) <= 1e-12, (c, d)
    other = rng.integers(2000, 20000, (16, 16)).astype(np.int64)
    assert abs(cut_scores(np.stack([a * counts, other * counts]), counts)[0]) < 0.3      # unrelated content does not


def test_cut_scores_flat_frames():
    from aiod_amd import cut_scores
    from aiod_amd.shots import cell_counts
    counts = cell_counts(130, 197, (16, 16))                 # ragged cells: a flat frame's sums differ per cell, its means do not
    rng = np.random.default_rng(2)
    flat_a, flat_b = 256 * 255 * counts, 77 * 3 * counts
    tex = rng.integers(0, 65280, counts.shape) * counts
    s = cut_scores(np.stack([flat_a, flat_b, tex, flat_a, flat_a]), counts)
    assert s.tolist() == [1.0, 0.0, 0.0, 1.0]


# ---- detect_cuts ---------------------------------------------------------------------------------------------------------------
def test_detect_cuts_on_written_out_scores():
    from aiod_amd import detect_cuts
    assert detect_cuts([0.93, 0.94, 0.92, 0.94, 0.04, 0.93, 0.94, 0.92, 0.93, 0.94, 0.93]) == [5]                 # one clear cut
    assert detect_cuts([-0.3] * 11) == []                                        # sustained motion: every pair is low, none stands out
    assert detect_cuts([0.6] * 5 + [0.45] + [0.6] * 5) == []                     # below the threshold but not by the margin
    assert detect_cuts([0.9] * 5 + [0.55] + [0.9] * 5) == []                     # by the margin but not below the threshold
    assert detect_cuts([0.94] * 5 + [0, 0] + [0.94] * 4, min_shot_frames=2) == [6]      # a flash frame: one cut, the second would leave 1 frame
    assert detect_cuts([0.94] * 5 + [0, 0] + [0.94] * 4) == [6]                  # ... and with the default 5 the same, 6 | 6 frames
    # two cuts closer than min_shot_frames: the stronger (lower score) stays
    s = [0.9] * 6 + [0.2] + [0.9] * 2 + [0.1] + [0.9] * 6
    assert detect_cuts(s) == [10] and detect_cuts(s, min_shot_frames=3) == [7, 10]
    # the tie order: equal scores are taken by ascending t, so the earlier pair wins the conflict
    s = [0.9] * 6 + [0.1] + [0.9] * 2 + [0.1] + [0.9] * 6
    assert detect_cuts(s) == [7]
    assert detect_cuts([0.9] * 3 + [0.1] + [0.9] * 8, min_shot_frames=5) == []   # would leave 4 frames at the clip's start
    assert detect_cuts([0.9] * 3 + [0.1] + [0.9] * 8, min_shot_frames=4) == [4]
    assert detect_cuts([0.0]) == [] and detect_cuts([]) == []                    # a pair with no neighbour is never a candidate
    assert detect_cuts([0.9, 0.0, 0.9], min_shot_frames=2, radius=1) == [2]
    # the neighbours are clipped to the clip: pair 1 of 5 has pairs 0, 2, 3, 4 with radius 4
    assert detect_cuts([0.9, 0.1, 0.9, 0.9, 0.9], min_shot_frames=2) == [2]
    with pytest.raises(ValueError, match="min_shot_frames must be at least 2"):
        detect_cuts([0.9, 0.0, 0.9], min_shot_frames=1)
    assert detect_cuts(np.array([0.93, 0.94, 0.92, 0.94, 0.04, 0.93, 0.94, 0.92, 0.93]), threshold=0.5, margin=0.25, radius=4, min_shot_frames=4) == [5]


# ---- plan_shots ----------------------------------------------------------------------------------------------------------------
def test_plan_shots_and_its_messages():
    from aiod_amd import plan_shots
    assert plan_shots(9, []) == [(0, 9)] and plan_shots(9, [5]) == [(0, 5), (5, 9)] and plan_shots(12, (7,)) == [(0, 7), (7, 12)]
    assert plan_shots(9, [2, 4, 7]) == [(0, 2), (2, 4), (4, 7), (7, 9)] and plan_shots(9, np.array([5])) == [(0, 5), (5, 9)]
    with pytest.raises(ValueError, match=r"cut 0 at frame 9 is outside 1\.\.8 \(a clip of 9 frames\)"):
        plan_shots(9, [9])
    with pytest.raises(ValueError, match=r"cut 0 at frame 0 is outside 1\.\.8"):
        plan_shots(9, [0])
    with pytest.raises(ValueError, match="cut 1 at frame 3 does not follow cut 0 at frame 5: cuts must be strictly increasing"):
        plan_shots(9, [5, 3])
    with pytest.raises(ValueError, match="cut 1 at frame 5 does not follow cut 0 at frame 5"):
        plan_shots(9, [5, 5])
    with pytest.raises(ValueError, match=r"cut 0 at frame 1 leaves shot 0 \(frames 0\.\.0\) with 1 frame: a shot needs at least 2"):
        plan_shots(9, [1])
    with pytest.raises(ValueError, match=r"cut 1 at frame 6 leaves shot 1 \(frames 5\.\.5\) with 1 frame"):
        plan_shots(9, [5, 6])
    with pytest.raises(ValueError, match=r"cut 0 at frame 8 leaves shot 1 \(frames 8\.\.8\) with 1 frame"):
        plan_shots(9, [8])
    with pytest.raises(ValueError, match="cut 0 is 2.5: cuts are integer"):
        plan_shots(9, [2.5])
    with pytest.raises(ValueError, match="cut 0 is '5'"):
        plan_shots(9, ["5"])
    with pytest.raises(ValueError, match="at least 2 frames, got 1"):
        plan_shots(1, [])


# ---- orchestration with stub engines -------------------------------------------------------------------------------------------
def _ident(img):
    return int(np.asarray(img)[0, 0, 0])


class _StubFlow:
    def __init__(self, log, h, w):
        self.log, self.h, self.w, self.capacity, self.slots = log, h, w, 2, {}

    def encode(self, slot, img):
        assert img.dtype == np.uint8 and img.shape == (self.h, self.w, 3)
        self.log.append(("encode", slot, _ident(img)))
        self.slots[slot] = _ident(img)

    def flow_slots(self, pairs, on_device=False):
        assert on_device
        self.log.append(("flow", list(pairs), [(self.slots[a], self.slots[b]) for a, b in pairs]))
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
    """No luma_grids: the engines of a user who wrote a stub before shots existed."""

    def __init__(self):
        self.log = []

    def frame(self, x):
        self.log.append(("frame", _ident(x)))
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
        return (np.clip(img, 0, 1) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)

    def quantise_render(self, img):
        return (img.astype(np.float64) * 255 + 0.5).astype(np.uint8)

    def lerp(self, a, b, w):
        return a + np.float32(w) * (b - a)

    def stack(self, imgs):
        return np.stack(imgs)

    def to_host(self, t):
        return np.asarray(t)

    def warp_error(self, img1, img2, f12, f21, align_corners):
        assert f12[0] == "small" and f12[1] == 100 * _ident(img1) + _ident(img2) and f21[1] == 100 * _ident(img2) + _ident(img1)
        self.log.append(("warp_error", _ident(img1), _ident(img2)))
        return float(2 ** _ident(img1))                      # every subset of pairs has a mean of its own

    def sync(self):
        pass


class _AutoEngines(_StubEngines):
    """With luma_grids: frames below `cut` show one pattern under a per-frame gain and offset (flicker), the others another."""

    def __init__(self, cut):
        super().__init__()
        self.cut = cut

    def luma_grids(self, dev_frames, gh, gw):
        self.log.append(("luma_grids", [_ident(f) for f in dev_frames], gh, gw))
        rng = np.random.default_rng(3)
        pat = rng.integers(1000, 30000, (2, gh, gw)).astype(np.int64)
        counts = np.full((gh, gw), 6, np.int64)
        sums = np.stack([((1 + i % 3) * pat[int(_ident(f) >= self.cut)] + 100 * i) * counts for i, f in enumerate(dev_frames)])
        return sums, counts


SMALL = {"maximum_number_of_frames": 5, "iters_num": 61, "evaluate_every": 30, "pretrain_iter_number": 2, "samples_batch": 64,
         "number_of_channels_atlas": 16, "number_of_channels_mapping1": 16}
S = 7


def _frames(n, h=8, w=12):
    return [np.full((h, w, 3), i, np.uint8) for i in range(n)]


def _seeds(log):
    """Per fitted window, what it drew from its generator: (pre-train seed, sampler seed)."""
    out = []
    for e in log:
        if e[0] == "pretrain":
            out.append([e[1]])
        elif e[0] == "train" and len(out[-1]) == 1:
            out[-1].append(e[3])
    return [tuple(s) for s in out]


def _standalone_seeds(seed, n):
    import aiod_amd
    E = _StubEngines()
    aiod_amd.Deflicker(None, None, None, config=SMALL, seed=seed, engines=E).run(_frames(n))
    return _seeds(E.log)[0]


def _device_log(log):
    """The calls whose order and arguments the contract fixes, seeds left out (they are compared on their own)."""
    keep = {"encode", "flow", "raft_open", "raft_close", "atlas_open", "upload", "atlas_close", "filter_open", "reset", "filter", "filter_close"}
    return [e for e in log if e[0] in keep]


def test_call_list_with_one_cut():
    import aiod_amd
    E = _StubEngines()
    d = aiod_amd.Deflicker(None, None, None, config=SMALL, down=4, seed=S, engines=E, cuts=[5])
    res = d.run(_frames(9), keep=("final", "stage1", "flows"), warp_error=True)
    enc = lambda slot, i: ("encode", slot, i)                                      # noqa: E731
    flow = lambda a, b, i: ("flow", [(a, b), (b, a)], [(i, i + 1), (i + 1, i)])      # noqa: E731
    up = lambda a, b: ("upload", list(range(a, b)), [100 * i + i + 1 for i in range(a, b - 1)], [100 * (i + 1) + i for i in range(a, b - 1)])      # noqa: E731
    assert _device_log(E.log) == [
        ("raft_open", 8, 12),
        enc(0, 0), enc(1, 1), flow(0, 1, 0), enc(0, 2), flow(1, 0, 1), enc(1, 3), flow(0, 1, 2), enc(0, 4), flow(1, 0, 3),
        enc(0, 5),                                                                 # no flow for pair (4, 5); the slots start again at 0
        enc(1, 6), flow(0, 1, 5), enc(0, 7), flow(1, 0, 6), enc(1, 8), flow(0, 1, 7),
        ("raft_close",),
        ("atlas_open", 3, 2, 5), up(0, 5), ("atlas_close",),
        ("atlas_open", 3, 2, 4), up(5, 9), ("atlas_close",),
        ("filter_open", 8, 12),
        ("reset",), ("filter", 0, 0), ("filter", 1, 1), ("filter", 2, 2), ("filter", 3, 3), ("filter", 4, 4),
        ("reset",), ("filter", 5, 5), ("filter", 6, 6), ("filter", 7, 7), ("filter", 8, 8),
        ("filter_close",)]
    # a shot's RAFT calls are those of its stand-alone run
    alone = _StubEngines()
    aiod_amd.Deflicker(None, None, None, config=SMALL, seed=S + 1, engines=alone).run(_frames(9)[5:])
    raft = lambda log: [e for e in log if e[0] in ("encode", "flow")]              # noqa: E731
    assert raft(E.log)[9:] == raft(alone.log)
    # seeds S and S + 1
    assert _seeds(E.log) == [_standalone_seeds(S, 5), _standalone_seeds(S + 1, 4)] and len(set(_seeds(E.log))) == 2
    assert res["shots"] == [(0, 5), (5, 9)] and res["windows"] == [(0, 5), (5, 9)] and res["cut_pairs"] == [4] and res["seam_pairs"] == []
    assert res["cuts"] == [5] and res["cut_scores"] is None and set(res["seconds"]) == {"decode + flow", "stage 1", "stage 2", "warp error", "total"}
    assert len(res["flows"]) == 8 and res["flows"][4] is None and all(f is not None for i, f in enumerate(res["flows"]) if i != 4)
    assert [int(f[0, 0, 0]) for f in res["final"]] == list(range(9))
    # E_warp: no call for the cut pair, None in per_pair, every mean over the others
    assert [e[1:] for e in E.log if e[0] == "warp_error"] == [(i, i + 1) for i in (0, 1, 2, 3, 5, 6, 7)] * 2
    we = res["warp_error"]
    others = [2.0 ** i for i in (0, 1, 2, 3, 5, 6, 7)]
    for name in ("input", "final"):
        assert we[name]["per_pair"] == [1.0, 2.0, 4.0, 8.0, None, 32.0, 64.0, 128.0]
        assert we[name]["mean"] == np.mean(others) == we[name]["mean_other_pairs"] and we[name]["mean_seam_pairs"] is None
    assert we["cut_pairs"] == [4] and we["seam_pairs"] == []


def test_windows_inside_shots():
    """7 + 5 frames, at most 5 per window: shot A is cut into (0, 4), (4, 7), shot B is (7, 12); windows are numbered in clip order."""
    import aiod_amd
    E = _StubEngines()
    res = aiod_amd.Deflicker(None, None, None, config=SMALL, seed=S, engines=E, cuts=[7]).run(_frames(12), warp_error=False)
    assert res["shots"] == [(0, 7), (7, 12)] and res["windows"] == [(0, 4), (4, 7), (7, 12)]
    assert res["seam_pairs"] == [3] and res["cut_pairs"] == [6] and len(res["psnr"]) == 3
    assert _seeds(E.log) == [_standalone_seeds(S, 4), _standalone_seeds(S + 1, 3), _standalone_seeds(S + 2, 5)]
    ups = [e for e in E.log if e[0] == "upload"]
    assert [u[1] for u in ups] == [list(range(0, 4)), list(range(4, 7)), list(range(7, 12))]
    assert ups[2][2] == [100 * i + i + 1 for i in range(7, 11)]                  # window 2 gets the pairs of its own frames
    assert [e[0] for e in E.log if e[0] in ("reset", "filter")] == ["reset"] + ["filter"] * 7 + ["reset"] + ["filter"] * 5
    we = res["warp_error"]
    assert we["seam_pairs"] == [3] and we["cut_pairs"] == [6] and we["final"]["per_pair"][6] is None
    assert we["final"]["mean_seam_pairs"] == 8.0 and we["final"]["mean_other_pairs"] == np.mean([2.0 ** i for i in (0, 1, 2, 4, 5, 7, 8, 9, 10)])
    # window overlap applies inside shots only: no frame of shot B is blended with shot A
    E2 = _StubEngines()
    r2 = aiod_amd.Deflicker(None, None, None, config=SMALL, seed=S, engines=E2, cuts=[7], window_overlap=1).run(_frames(12))
    assert r2["windows"] == [(0, 4), (3, 7), (7, 12)] and r2["seam_pairs"] == [2, 3] and r2["cut_pairs"] == [6]


def test_default_run_is_todays():
    """cuts=None: the engine calls of the pipeline as it was - one handle, one parity, one reset - on engines without luma_grids."""
    import aiod_amd
    E = _StubEngines()
    assert not hasattr(E, "luma_grids")
    res = aiod_amd.Deflicker(None, None, None, config=SMALL, down=4, seed=S, engines=E).run(_frames(9), keep=("final", "flows"))
    up = lambda a, b: ("upload", list(range(a, b)), [100 * i + i + 1 for i in range(a, b - 1)], [100 * (i + 1) + i for i in range(a, b - 1)])      # noqa: E731
    expect = [("raft_open", 8, 12), ("encode", 0, 0)]
    for i in range(1, 9):
        cur, prev = i & 1, (i - 1) & 1
        expect += [("encode", cur, i), ("flow", [(prev, cur), (cur, prev)], [(i - 1, i), (i, i - 1)])]
    expect += [("raft_close",), ("atlas_open", 3, 2, 5), up(0, 5), ("atlas_close",), ("atlas_open", 3, 2, 4), up(5, 9), ("atlas_close",),
               ("filter_open", 8, 12), ("reset",)] + [("filter", i, i) for i in range(9)] + [("filter_close",)]
    assert _device_log(E.log) == expect
    assert [e[1] for e in E.log if e[0] == "frame"] == list(range(9))
    assert res["shots"] == [(0, 9)] and res["cut_pairs"] == [] and res["cuts"] is None and res["cut_scores"] is None
    assert res["windows"] == [(0, 5), (5, 9)] and res["seam_pairs"] == [4] and all(f is not None for f in res["flows"])
    assert set(res["seconds"]) == {"decode + flow", "stage 1", "stage 2", "total"}
    # an empty list of cuts is the same run
    E2 = _StubEngines()
    r2 = aiod_amd.Deflicker(None, None, None, config=SMALL, down=4, seed=S, engines=E2, cuts=[]).run(_frames(9))
    assert E2.log == E.log and r2["shots"] == [(0, 9)] and r2["cuts"] == []


def test_auto_scores_first_and_runs_raft_afterwards():
    import aiod_amd
    E = _AutoEngines(cut=5)
    res = aiod_amd.Deflicker(None, None, None, config=SMALL, seed=S, engines=E, cuts="auto", min_shot_frames=4).run(_frames(9), keep=("final", "flows"))
    names = [e[0] for e in E.log]
    assert names[:10] == ["frame"] * 9 + ["luma_grids"] and names.count("frame") == 9 and names.count("luma_grids") == 1
    assert E.log[9] == ("luma_grids", list(range(9)), 16, 16) and names[10] == "raft_open"
    assert res["shots"] == [(0, 5), (5, 9)] and res["cut_pairs"] == [4] and res["cuts"] == "auto" and res["flows"][4] is None
    assert len(res["cut_scores"]) == 8 and res["cut_scores"][4] < 0.3 and all(abs(v - 1) < 1e-12 for i, v in enumerate(res["cut_scores"]) if i != 4)
    assert set(res["seconds"]) == {"decode + cuts", "flow", "stage 1", "stage 2", "total"}
    # from RAFT on, the run with the detected cut is the run with the same cut given
    G = _StubEngines()
    aiod_amd.Deflicker(None, None, None, config=SMALL, seed=S, engines=G, cuts=[5]).run(_frames(9))
    assert _device_log(E.log) == _device_log(G.log) and _seeds(E.log) == _seeds(G.log)
    # with the default min_shot_frames = 5 the 4-frame shot is refused and the clip stays one shot
    E5 = _AutoEngines(cut=5)
    assert aiod_amd.Deflicker(None, None, None, config=SMALL, seed=S, engines=E5, cuts="auto").run(_frames(9))["shots"] == [(0, 9)]


def test_errors_come_before_any_fit_and_leave_the_object_usable():
    import aiod_amd
    E = _StubEngines()
    mk = lambda **kw: aiod_amd.Deflicker(None, None, None, config=SMALL, seed=S, engines=E, **kw)      # noqa: E731
    for bad in ("yes", 5, 2.5, {"a": 1}):
        with pytest.raises(ValueError, match="cuts must be None, \"auto\" or a sequence"):
            mk(cuts=bad)
    with pytest.raises(ValueError, match="cuts: plan_shots: cut 1 at frame 3 does not follow cut 0 at frame 5"):
        mk(cuts=[5, 3])
    with pytest.raises(ValueError, match="cuts: plan_shots: cut 0 is 2.5"):
        mk(cuts=[2.5])
    with pytest.raises(ValueError, match="cuts=\"auto\" needs an engine with luma_grids.*_StubEngines has none"):
        mk(cuts="auto")
    with pytest.raises(ValueError, match="min_shot_frames must be at least 2"):
        aiod_amd.Deflicker(None, None, None, config=SMALL, engines=_AutoEngines(5), cuts="auto", min_shot_frames=1)
    d = mk(cuts=[5])
    with pytest.raises(ValueError, match=r"cut 0 at frame 5 is outside 1\.\.3 \(a clip of 4 frames\)"):
        d.run(_frames(4))
    assert E.log == []                                   # a clip of known length: refused before the first upload
    with pytest.raises(ValueError, match=r"cut 0 at frame 5 leaves shot 1 \(frames 5\.\.5\) with 1 frame"):
        d.run(iter(_frames(6)))                          # an iterator: known once it is decoded, still before any fit
    names = [e[0] for e in E.log]
    assert "atlas_open" not in names and names.count("raft_open") == names.count("raft_close") == 1
    assert d.run(_frames(9))["shots"] == [(0, 5), (5, 9)]      # and the object still works


# ---- CLIs ----------------------------------------------------------------------------------------------------------------------
def test_cli_flags(tmp_path, capsys):
    from aiod_amd import deflicker, shots
    o = deflicker.parse_args(["--frames_dir", "x"])
    assert o.cuts is None and (o.cut_threshold, o.cut_margin, o.cut_radius, o.min_shot_frames) == (0.5, 0.25, 4, 5)
    assert deflicker.parse_args(["--frames_dir", "x", "--cuts", "none"]).cuts is None
    assert deflicker.parse_args(["--frames_dir", "x", "--cuts", "auto"]).cuts == "auto"
    o = deflicker.parse_args(["--frames_dir", "x", "--cuts", "5,12,40", "--cut_threshold", "0.4", "--cut_margin", "0.3", "--cut_radius", "2", "--min_shot_frames", "3"])
    assert o.cuts == [5, 12, 40] and (o.cut_threshold, o.cut_margin, o.cut_radius, o.min_shot_frames) == (0.4, 0.3, 2, 3)
    with pytest.raises(SystemExit):
        deflicker.parse_args(["--frames_dir", "x", "--cuts", "sometimes"])
    assert "expected none, auto or comma-separated" in capsys.readouterr().err
    o = shots.parse_args(["--frames_dir", "x"])
    assert o.grid == (16, 16) and (o.cut_threshold, o.cut_margin, o.cut_radius, o.min_shot_frames, o.gpu) == (0.5, 0.25, 4, 5, 0)
    o = shots.parse_args(["--frames_dir", "x", "--grid", "8x12", "--cut_threshold", "0.4", "--cut_margin", "0.1", "--cut_radius", "3", "--min_shot_frames", "2", "--gpu", "1"])
    assert o.grid == (8, 12) and (o.cut_threshold, o.cut_margin, o.cut_radius, o.min_shot_frames, o.gpu) == (0.4, 0.1, 3, 2, 1)
    for bad in ("65x4", "0x4", "16", "axb"):
        with pytest.raises(SystemExit):
            shots.parse_args(["--frames_dir", "x", "--grid", bad])
    import subprocess
    for script, flags in (("deflicker.py", ("--cuts", "--cut_threshold", "--cut_margin", "--cut_radius", "--min_shot_frames")),
                          ("shots.py", ("--frames_dir", "--grid", "--cut_threshold", "--cut_margin", "--cut_radius", "--min_shot_frames", "--gpu"))):
        r = subprocess.run([sys.executable, os.path.join(PKG, script), "--help"], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 0 and all(f in r.stdout for f in flags), (script, r.stdout, r.stderr)


def test_run_pipeline_forwards_the_cut_flags(capsys):
    R = _load("af_run_pipeline_shots", os.path.join(PKG, "run_pipeline.py"))
    py = sys.executable or "python"
    base = "%s %s --frames_dir ./data/test/clip --out ./results/clip --gpu 0 --ckpt_filter ./pretrained_weights/neural_filter.pth --ckpt_local ./pretrained_weights/local_refinement_net.pth" \
           % (py, os.path.join(PKG, "deflicker.py"))
    o = R.parse_opts(["--video_frame_folder", "clip", "--in_process"])
    assert o.cuts == "none" and R.build_commands(o)[-1] == ("sh", base)              # nothing given, nothing forwarded
    o = R.parse_opts(["--video_frame_folder", "clip", "--in_process", "--cuts", "auto", "--min_shot_frames", "4", "--cut_threshold", "0.4"])
    assert R.build_commands(o)[-1] == ("sh", base + " --cuts auto --cut_threshold 0.4 --min_shot_frames 4")
    o = R.parse_opts(["--video_frame_folder", "clip", "--in_process", "--cuts", "5,12", "--cut_margin", "0.3", "--cut_radius", "2"])
    assert R.build_commands(o)[-1] == ("sh", base + " --cuts 5,12 --cut_margin 0.3 --cut_radius 2")
    for bad in ("5;ls", "auto x", "$(id)", "5,", "-3"):
        with pytest.raises(SystemExit):
            R.parse_opts(["--video_frame_folder", "clip", "--in_process", "--cuts=" + bad])      # the text goes into a shell command
        assert "expected none, auto or comma-separated" in capsys.readouterr().err
    for extra in (["--cuts", "auto"], ["--cuts", "5"], ["--cut_threshold", "0.4"], ["--min_shot_frames", "4"], ["--native_stage2", "--cut_radius", "2"]):
        with pytest.raises(SystemExit):
            R.parse_opts(["--video_frame_folder", "clip"] + extra)
        assert "need --in_process" in capsys.readouterr().err
    assert R.build_commands(argparse.Namespace(video_name=None, video_frame_folder="clip", fps=10, gpu=0, class_name=None, in_process=True))[-1] == ("sh", base)


def test_exports():
    import aiod_amd
    for name in ("luma_grids", "cut_scores", "detect_cuts", "plan_shots"):
        assert getattr(aiod_amd, name) is getattr(aiod_amd.shots, name)
    import inspect
    sig = inspect.signature(aiod_amd.Deflicker.__init__).parameters
    assert all(k in sig for k in ("cuts", "cut_threshold", "cut_margin", "cut_radius", "min_shot_frames")) and sig["cuts"].default is None
    assert hasattr(aiod_amd.deflicker.DeviceEngines, "luma_grids")
    assert "af_luma_grid" in aiod_amd.atlasfit.ABI_SYMBOLS
