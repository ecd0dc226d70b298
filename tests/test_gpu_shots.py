"""Shot-aware deflicker on the GPU: k_luma_grid (af_luma_grid, csrc/shots.hip) and Deflicker(cuts=...).

Every comparison of device results here is exact.  The kernel sums integers, so its grids must EQUAL numpy's int64 sums whatever the
order of summation.  The pipeline's contract is derived, not measured: a shot is fitted, filtered and given its flows by the entry
points a stand-alone run of its frames calls, on the same values in the same order (window k with seed S + k), so shot j equals
Deflicker(seed=S + k_j).run(frames[a_j:b_j]) with tolerance zero.  The only float tolerance, 1e-12, is between two fp64 evaluations of
the score (numpy's pairwise sums against plain loops over 256 cells of values below 256: relative rounding of a few 1e-16 each).

Clip: shot A = synthetic_clip(5 or 7, H, W, seed=5), shot B = the frames of synthetic_clip(4 or 5, W, H, seed=9, motion=(-2, 1)),
each transposed to (H, W, 3).  On a 16 x 16 grid the numpy twin scores the pairs inside a shot 0.924 - 0.942 and the pair across the
cut 0.040 (asserted below, on the host values)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pipeline_bench as PB  # noqa: E402

H, W, DOWN, SEED = 130, 197, 4, 11                         # those of tests/test_gpu_deflicker.py, and its SHORT config
SHORT = {"samples_batch": 1024, "iters_num": 31, "evaluate_every": 30, "pretrain_iter_number": 3, "stop_global_rigidity": 15}
PKG = os.path.join(ROOT, "all-in-one-deflicker_amd")


# ---- the numpy twins -----------------------------------------------------------------------------------------------------------
def grids_numpy(frames, gh, gw):
    """af_luma_grid's contract in numpy int64: (sums (n, GH, GW), counts (GH, GW))."""
    frames = np.asarray(frames)
    n, h, w = frames.shape[:3]
    gh, gw = min(gh, h), min(gw, w)
    luma = (frames.astype(np.int64) * np.array([77, 150, 29], np.int64)).sum(axis=3)
    sums, counts = np.zeros((n, gh, gw), np.int64), np.zeros((gh, gw), np.int64)
    for i in range(gh):
        r0, r1 = i * h // gh, (i + 1) * h // gh
        for j in range(gw):
            c0, c1 = j * w // gw, (j + 1) * w // gw
            sums[:, i, j] = luma[:, r0:r1, c0:c1].sum(axis=(1, 2))
            counts[i, j] = (r1 - r0) * (c1 - c0)
    return sums, counts


def scores_numpy(sums, counts):
    """The score with plain loops over the cells (fp64)."""
    out = []
    for t in range(len(sums) - 1):
        a = [float(s) / (256.0 * float(c)) for s, c in zip(sums[t].ravel(), counts.ravel())]
        b = [float(s) / (256.0 * float(c)) for s, c in zip(sums[t + 1].ravel(), counts.ravel())]
        ma, mb = sum(a) / len(a), sum(b) / len(b)
        sab = sum((x - ma) * (y - mb) for x, y in zip(a, b))
        saa, sbb = sum((x - ma) ** 2 for x in a), sum((y - mb) ** 2 for y in b)
        out.append(1.0 if saa == 0.0 and sbb == 0.0 else 0.0 if saa == 0.0 or sbb == 0.0 else sab / (saa * sbb) ** 0.5)
    return np.array(out)


def shot_b(n):
    return [np.ascontiguousarray(f.transpose(1, 0, 2)) for f in PB.synthetic_clip(n, W, H, seed=9, motion=(-2.0, 1.0))]


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


# ---- kernel: exact equality with numpy -----------------------------------------------------------------------------------------
def _case(name):
    rng = np.random.default_rng(7)
    if name == "white":
        return np.full((1, 300, 300, 3), 255, np.uint8)
    n, h, w = {"ragged": (1, 130, 197), "clamped": (1, 7, 5), "one cell": (1, 64, 48), "fine": (1, 33, 70), "three frames": (3, 37, 41),
               "two strips": (3, 150, 90)}[name]
    return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("name,grid", [("ragged", (16, 16)),          # 130 x 197: cells of 8/9 x 12/13 pixels, rows of 591 bytes
                                       ("clamped", (16, 16)),         # 7 x 5: the grid clamps to the image, one pixel per cell
                                       ("one cell", (1, 1)),          # 64 x 48
                                       ("white", (1, 1)),             # 300 x 300 of 255: 5 875 200 000 > 2^32, and a cell cut into strips
                                       ("fine", (64, 64)),            # 33 x 70: clamps to 33 x 64, cells of 1 x 1/2
                                       ("three frames", (16, 16)),    # 37 x 41 x 3 bytes per frame: the frame stride is no multiple of 16
                                       ("three frames", (1, 1)),
                                       ("two strips", (1, 2)),        # 150 x 45 cells: two strips of 92 and 58 rows, in each of three frames
                                       ("ragged", (3, 64))])
def test_luma_grid_equals_numpy(name, grid):
    import aiod_amd
    frames = _case(name)
    sums, counts = grids_numpy(frames, *grid)
    if name == "white":
        assert sums.tolist() == [[[5875200000]]] and sums[0, 0, 0] > 2 ** 32
    host = aiod_amd.luma_grids(frames, grid)                                             # one call, host pointer
    dev = aiod_amd.luma_grids(torch.from_numpy(frames).cuda(), grid)                     # one call, device pointer
    per_frame = aiod_amd.luma_grids([torch.from_numpy(f).cuda() for f in frames], grid)  # a call per frame
    mixed = aiod_amd.luma_grids(list(frames), grid)
    for got in (host, dev, per_frame, mixed):
        assert got[0].dtype == np.int64 and got[0].shape == sums.shape and got[1].dtype == np.int64
        assert np.array_equal(got[0], sums), (name, grid, np.argwhere(got[0] != sums)[:4])
        assert np.array_equal(got[1], counts)
    assert np.array_equal(aiod_amd.luma_grids(frames, grid)[0], sums)                    # and a second run


def test_luma_grid_refusals_name_the_cause():
    import aiod_amd
    lib = aiod_amd.load_library()
    src = np.zeros((2, 6, 8, 3), np.uint8)
    out = np.zeros(2 * 6 * 8, np.uint64)
    s, o = src.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    cases = [((None, 2, 6, 8, 4, 4, o), "null pointer"), ((s, 2, 6, 8, 4, 4, None), "null pointer"),
             ((s, 0, 6, 8, 4, 4, o), "n < 1"), ((s, 2, 0, 8, 4, 4, o), "h < 1"), ((s, 2, 6, -1, 4, 4, o), "w < 1"),
             ((s, 2, 6, 8, 0, 4, o), "gh must be 1..64"), ((s, 2, 6, 8, 65, 4, o), "gh must be 1..64"),
             ((s, 2, 6, 8, 4, 0, o), "gw must be 1..64"), ((s, 2, 6, 8, 4, 65, o), "gw must be 1..64"),
             ((s, 2, (1 << 24) + 1, 8, 4, 4, o), "image too large"), ((s, 2, 6, (1 << 24) + 1, 4, 4, o), "image too large")]      # refused before a byte is read
    for args, msg in cases:
        rc = lib.af_luma_grid(0, *args, 0)
        text = lib.af_last_error(None).decode()
        assert rc == -1 and text == "af_luma_grid: " + msg, (args[1:6], rc, text)      # AF_EINVAL
    with pytest.raises(aiod_amd.AtlasFitError, match="af_luma_grid: gh must be 1..64"):
        aiod_amd.luma_grids(src, (0, 4))
    with pytest.raises(ValueError, match="frames must be \\(H, W, 3\\) uint8"):
        aiod_amd.luma_grids(src.astype(np.float32))
    with pytest.raises(ValueError, match="frame 1 is 8x7, the first frame 8x6"):
        aiod_amd.luma_grids([src[0], np.zeros((7, 8, 3), np.uint8)])
    got = aiod_amd.luma_grids(src + 3, (4, 4))                                           # and the library still works
    assert np.array_equal(got[0], grids_numpy(src + 3, 4, 4)[0])


# ---- pipeline ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    d = tmp_path_factory.mktemp("shots_assets")
    weights = PB.synthetic_weights()
    paths = PB.write_weights(str(d / "weights"), weights)
    cfgs = {}
    for name, extra in (("short", {}), ("win5", {"maximum_number_of_frames": 5})):
        cfgs[name] = dict(REFERENCE_CONFIG, **SHORT, **extra)
        with open(d / (name + ".json"), "w") as f:
            json.dump(cfgs[name], f)
    a7, b5 = PB.synthetic_clip(7, H, W, seed=5), shot_b(5)
    a5 = PB.synthetic_clip(5, H, W, seed=5)
    assert all(np.array_equal(x, y) for x, y in zip(a5, a7)) and all(np.array_equal(x, y) for x, y in zip(shot_b(4), b5))      # longer clips extend shorter ones
    mb = [np.ascontiguousarray(m.T) for m in PB.synthetic_masks(4, W, H, motion=(-2.0, 1.0))]
    return {"dir": d, "weights": weights, "paths": paths, "cfg": cfgs, "cfg_path": {k: str(d / (k + ".json")) for k in cfgs},
            "clip9": a5 + b5[:4], "clip12": a7 + b5, "masks9": PB.synthetic_masks(5, H, W) + mb}


KEEP = ("final", "stage1", "filtered", "flows")


@pytest.fixture(scope="module")
def api(assets):
    """run(clip name, lo, hi, ...) through the Python API, cached: the tests compare against the same runs.  The results are read, never changed."""
    import aiod_amd
    cache = {}

    def run(clip, lo, hi, cfg="short", seed=SEED, masks=False, **kw):
        key = (clip, lo, hi, cfg, seed, masks, tuple(sorted((k, str(v)) for k, v in kw.items())))
        if key not in cache:
            d = aiod_amd.Deflicker(*assets["weights"], config=assets["cfg"][cfg], down=DOWN, seed=seed, **kw)
            cache[key] = d.run(assets[clip][lo:hi], masks=assets["masks9"][lo:hi] if masks else None, keep=KEEP)
        return cache[key]
    return run


def _same_flows(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g is not None and torch.equal(g[0], w[0]) and torch.equal(g[1], w[1])


def _assert_shot_is_standalone(whole, a, b, alone, window):
    """Frames a .. b - 1 of `whole` are the run `alone` of those frames, bit for bit; psnr of `window` is that run's."""
    for name in ("final", "stage1", "filtered"):
        assert np.array_equal(whole[name][a:b], alone[name]), "%s differs in %d values" % (name, int((whole[name][a:b] != alone[name]).sum()))
    _same_flows(whole["flows"][a:b - 1], alone["flows"])
    assert whole["psnr"][window] == alone["psnr"][0]


def test_host_scores_of_the_clips(assets):
    """The figures the pipeline tests rest on, from the numpy twins alone."""
    from aiod_amd import detect_cuts
    s9 = scores_numpy(*grids_numpy(assets["clip9"], 16, 16))
    inside = np.delete(s9, 4)
    assert (round(float(inside.min()), 3), round(float(inside.max()), 3), round(float(s9[4]), 3)) == (0.924, 0.942, 0.040), s9
    assert detect_cuts(s9, min_shot_frames=4) == [5] and detect_cuts(s9) == []
    assert detect_cuts(scores_numpy(*grids_numpy(assets["clip12"], 16, 16))) == [7]


def test_explicit_cut_equals_the_two_standalone_runs(assets, api):
    cut = api("clip9", 0, 9, cuts=[5])
    first, second = api("clip9", 0, 5), api("clip9", 5, 9, seed=SEED + 1)
    assert cut["shots"] == [(0, 5), (5, 9)] and cut["windows"] == [(0, 5), (5, 9)] and cut["cut_pairs"] == [4] and cut["seam_pairs"] == []
    assert cut["cuts"] == [5] and cut["cut_scores"] is None and len(cut["flows"]) == 8 and cut["flows"][4] is None
    _assert_shot_is_standalone(cut, 0, 5, first, 0)
    _assert_shot_is_standalone(cut, 5, 9, second, 1)
    assert first["shots"] == [(0, 5)] and first["cut_pairs"] == [] and first["cuts"] is None and first["cut_scores"] is None
    # without the cut the clip is one window across two scenes: frame 5 gets another style and the state of frame 4
    one = api("clip9", 0, 9)
    assert one["windows"] == [(0, 9)] and one["flows"][4] is not None
    assert not np.array_equal(cut["final"][5], one["final"][5]) and not np.array_equal(cut["stage1"][5], one["stage1"][5])


def test_auto_finds_the_cut_and_gives_the_same_run(assets, api):
    import aiod_amd
    auto = api("clip9", 0, 9, cuts="auto", min_shot_frames=4)
    cut = api("clip9", 0, 9, cuts=[5])
    assert auto["shots"] == [(0, 5), (5, 9)] and auto["cuts"] == "auto" and auto["cut_pairs"] == [4] and auto["windows"] == cut["windows"]
    for name in ("final", "stage1", "filtered"):
        assert np.array_equal(auto[name], cut[name]), name
    assert auto["flows"][4] is None and auto["psnr"] == cut["psnr"]
    _same_flows([f for f in auto["flows"] if f is not None], [f for f in cut["flows"] if f is not None])
    assert set(auto["seconds"]) == {"decode + cuts", "flow", "stage 1", "stage 2", "total"}
    sums, counts = aiod_amd.luma_grids(assets["clip9"])
    assert auto["cut_scores"] == aiod_amd.cut_scores(sums, counts).tolist()                      # exactly
    twin = grids_numpy(assets["clip9"], 16, 16)
    assert np.array_equal(sums, twin[0]) and np.array_equal(counts, twin[1])
    assert np.abs(np.array(auto["cut_scores"]) - scores_numpy(*twin)).max() <= 1e-12


def test_windows_inside_shots(assets, api):
    r = api("clip12", 0, 12, cfg="win5", cuts=[7])
    assert r["shots"] == [(0, 7), (7, 12)] and r["windows"] == [(0, 4), (4, 7), (7, 12)] and r["seam_pairs"] == [3] and r["cut_pairs"] == [6]
    assert len(r["psnr"]) == 3 and r["flows"][6] is None
    _assert_shot_is_standalone(r, 7, 12, api("clip12", 7, 12, cfg="win5", seed=SEED + 2), 2)      # window 2 is fitted with S + 2


def test_two_layer_shots(assets, api):
    r = api("clip9", 0, 9, masks=True, cuts=[5])
    assert r["two_layer"] and r["shots"] == [(0, 5), (5, 9)]
    _assert_shot_is_standalone(r, 5, 9, api("clip9", 5, 9, seed=SEED + 1, masks=True), 1)
    assert not np.array_equal(r["stage1"][5:9], api("clip9", 0, 9, cuts=[5])["stage1"][5:9])      # the masks reached the fit


@pytest.fixture(scope="module")
def clip_dir(assets):
    PB.write_clip(str(assets["dir"] / "clip9"), assets["clip9"])
    return assets["dir"] / "clip9"


def test_cli_auto(assets, api, clip_dir, tmp_path):
    out = tmp_path / "res"
    cmd = PB.in_process_command(str(clip_dir), str(out), assets["cfg_path"]["short"], DOWN, SEED, assets["paths"],
                                extra=["--cuts", "auto", "--min_shot_frames", "4", "--keep_intermediates", "--warp_error"])
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rec = json.load(open(out / "deflicker.json"))
    assert rec["shots"] == [[0, 5], [5, 9]] and rec["cut_pairs"] == [4] and rec["cuts"] == "auto" and rec["seam_pairs"] == [] and rec["windows"] == [[0, 5], [5, 9]]
    assert (rec["cut_threshold"], rec["cut_margin"], rec["cut_radius"], rec["min_shot_frames"]) == (0.5, 0.25, 4, 4)
    assert set(rec["seconds"]) == {"decode + cuts", "flow", "stage 1", "stage 2", "warp error", "total"}
    auto = api("clip9", 0, 9, cuts="auto", min_shot_frames=4)
    assert rec["cut_scores"] == auto["cut_scores"] and rec["psnr"] == auto["psnr"]
    names = sorted(os.listdir(str(clip_dir) + "_flow"))
    assert len(names) == 2 * 7 and not any("00004.png_00005.png" in n or "00005.png_00004.png" in n for n in names)
    we = rec["warp_error"]
    assert we["cut_pairs"] == [4] and we["seam_pairs"] == []
    for name in ("input", "final"):
        per = we[name]["per_pair"]
        assert len(per) == 8 and per[4] is None and all(isinstance(v, float) for i, v in enumerate(per) if i != 4)
        assert we[name]["mean"] == float(np.mean([v for v in per if v is not None])) == we[name]["mean_other_pairs"]
    final = np.stack([_png(out / "final" / "output" / ("%05d.png" % i)) for i in range(9)])
    assert np.array_equal(final, auto["final"])


def test_shots_cli_prints_the_same_scores(assets, api, clip_dir, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(PKG, "shots.py"), "--frames_dir", str(clip_dir), "--min_shot_frames", "4"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["scores"] == api("clip9", 0, 9, cuts="auto", min_shot_frames=4)["cut_scores"]
    assert rec["cuts"] == [5] and rec["shots"] == [[0, 5], [5, 9]] and rec["frames"] == 9 and rec["grid"] == [16, 16]
    assert (rec["cut_threshold"], rec["cut_margin"], rec["cut_radius"], rec["min_shot_frames"]) == (0.5, 0.25, 4, 4)


def test_errors_name_the_cause_and_leave_the_process_usable(assets, api):
    import aiod_amd
    from aiod_amd import deflicker
    mk = lambda **kw: aiod_amd.Deflicker(*assets["weights"], config=assets["cfg"]["short"], down=DOWN, seed=SEED, **kw)      # noqa: E731
    with pytest.raises(ValueError, match="cuts must be None, \"auto\" or a sequence"):
        mk(cuts="always")
    with pytest.raises(ValueError, match="cut 1 at frame 3 does not follow cut 0 at frame 5"):
        mk(cuts=[5, 3])
    with pytest.raises(ValueError, match=r"cut 0 at frame 8 leaves shot 1 \(frames 8\.\.8\) with 1 frame"):
        mk(cuts=[8]).run(assets["clip9"])
    with pytest.raises(ValueError, match=r"cut 0 at frame 9 is outside 1\.\.8"):
        mk(cuts=[9]).run(torch.from_numpy(np.stack(assets["clip9"])).cuda())

    class NoGrids(deflicker.DeviceEngines):
        luma_grids = property()                              # hasattr is False: an engine from before shots existed

    with pytest.raises(ValueError, match="cuts=\"auto\" needs an engine with luma_grids"):
        mk(cuts="auto", engines=NoGrids(*assets["weights"]))
    with pytest.raises(ValueError, match="min_shot_frames must be at least 2"):
        mk(cuts="auto", min_shot_frames=1)
    with pytest.raises(SystemExit, match=r"cut 0 at frame 40 is outside"):
        deflicker.main(_argv(assets, "40"))                  # the CLI refuses before a frame is decoded
    # after every refusal the process computes what it computed before
    again = mk(cuts=[5]).run(assets["clip9"], keep=KEEP)
    cut = api("clip9", 0, 9, cuts=[5])
    assert np.array_equal(again["final"], cut["final"]) and np.array_equal(again["stage1"], cut["stage1"]) and again["psnr"] == cut["psnr"]


def _argv(assets, cuts):
    PB.write_clip(str(assets["dir"] / "clip3"), assets["clip9"][:3])
    return ["--frames_dir", str(assets["dir"] / "clip3"), "--out", str(assets["dir"] / "out3"), "--config", assets["cfg_path"]["short"], "--seed", str(SEED),
            "--model", assets["paths"][0], "--ckpt_filter", assets["paths"][1], "--ckpt_local", assets["paths"][2], "--cuts", cuts]
