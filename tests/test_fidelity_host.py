"""Host-side checks of the fidelity report (no GPU): the numpy restatement of af_fidelity (tests/fidelity_ref.py) that the GPU tests hold
the kernel to, against its fp64 twin (the skimage algorithm stated with scipy.ndimage.uniform_filter) and its definition; the Python
helpers, the refusals that need no device, the CLIs, and `Deflicker.run(fidelity=...)` with stub engines defined here on top of those of
tests/test_deflicker_host.py (imported, not edited).

The bound against the twin, 1e-12, is the issue's: both compute the same real-valued S, each with a few dozen fp64 roundings of values
near 1 (the twin's box means carry up to 225 additions); S and its partial derivatives are O(1) because c1 and c2 keep both
denominators away from 0."""
import json
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fidelity_ref as R  # noqa: E402
import test_deflicker_host as TD  # noqa: E402      (the stub engines of the one-process pipeline)

TWIN_BOUND = 1e-12


# ---- the restatement against its twin and its definition ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "structured"])
@pytest.mark.parametrize("win", [3, 7, 15])
def test_restatement_is_within_1e12_of_the_skimage_algorithm(win, kind):
    a, b = R.make_pair(37, 53, 10 * win + len(kind), kind)
    s, t = R.ssim_map(a, b, win), R.ssim_twin(a, b, win)
    assert s.shape == t.shape == (37 - win + 1, 53 - win + 1, 3) and s.dtype == np.float64
    worst = np.abs(s - t).max()
    print("win %d %s: max |S - twin| = %.3e" % (win, kind, worst))
    assert worst <= TWIN_BOUND
    assert np.abs(s).max() <= 1.0


@pytest.mark.parametrize("win", [3, 7, 15])
def test_identical_frames_give_exactly_one(win):
    a, _ = R.make_pair(20, 23, win, "random")
    s = R.ssim_map(a, a.copy(), win)
    assert np.array_equal(s, np.ones_like(s))
    assert not R.sse(a, a).any() and R.psnr(R.sse(a, a), 20 * 23) == math.inf


@pytest.mark.parametrize("win", [3, 7, 15])
def test_constant_frames(win):
    """The variance terms are 0: S = (2 x y + C1) / (x^2 + y^2 + C1) * (C2 / C2)."""
    a, b = np.full((17, 19, 3), 100, np.uint8), np.full((17, 19, 3), 50, np.uint8)
    same = R.ssim_map(a, a, win)
    assert np.array_equal(same, np.ones_like(same))
    s = R.ssim_map(a, b, win)
    c1 = (0.01 * 255) ** 2
    assert np.abs(s - (2 * 100 * 50 + c1) / (100 ** 2 + 50 ** 2 + c1)).max() <= TWIN_BOUND
    assert np.abs(s - R.ssim_twin(a, b, win)).max() <= TWIN_BOUND
    assert np.array_equal(R.sse(a, b), np.full(3, 17 * 19 * 2500, np.uint64))


def test_white_against_black():
    a, b = np.full((16, 16, 3), 255, np.uint8), np.zeros((16, 16, 3), np.uint8)
    s = R.ssim_map(a, b, 7)
    c1 = (0.01 * 255) ** 2
    assert np.abs(s - c1 / (255.0 ** 2 + c1)).max() <= TWIN_BOUND and abs(float(s[0, 0, 0]) - 9.999e-05) < 1e-8
    assert np.array_equal(R.sse(a, b), np.full(3, 256 * 65025, np.uint64))
    assert abs(R.psnr(R.sse(a, b), 256)) < 1e-12           # the largest error there is: 0 dB


def test_the_largest_integers_stay_exact():
    """win = 15: N Sxx reaches 225 * 225 * 255^2 = 3 291 890 625 > 2^31 (the int64 of the issue) and stays far below 2^53."""
    assert 225 * 225 * 255 ** 2 > 2 ** 31 and 2 * 225 * 225 * 255 ** 2 < 2 ** 53
    a = np.full((15, 15, 3), 255, np.uint8)
    assert R.box_sums(a.astype(np.int64) ** 2, 15).max() == 225 * 255 ** 2
    assert np.array_equal(R.ssim_map(a, a, 15), np.ones((1, 1, 3)))


# ---- the python helpers ------------------------------------------------------------------------------------------------------------
def test_psnr_from_sse_and_summarise():
    import aiod_amd
    from aiod_amd import fidelity as F
    assert F.DEFAULT_WINDOW == aiod_amd.DEFAULT_WINDOW == 7
    for name in ("frame_fidelity", "frame_fidelity_device", "psnr_from_sse", "summarise"):
        assert getattr(aiod_amd, name) is getattr(F, name)
    assert F.psnr_from_sse([0, 0, 0], 100) == math.inf
    assert F.psnr_from_sse(np.array([10, 20, 30], np.uint64), 100) == 10.0 * math.log10(255.0 * 255.0 * 3.0 * 100.0 / 60.0)
    assert F.psnr_from_sse([3 * 65025, 0, 0], 1) == 0.0
    big = np.array([2 ** 63, 2 ** 63, 5], np.uint64)         # the sum passes 2^64: taken in Python integers
    assert F.psnr_from_sse(big, 16384 ** 2) == 10.0 * math.log10(255.0 * 255.0 * 3.0 * float(16384 ** 2) / float(2 ** 64 + 5))
    sse = np.array([[10, 20, 30], [0, 0, 0], [1, 1, 1]], np.uint64)
    ssim = np.array([[0.5, 0.25, 0.75], [1.0, 1.0, 1.0], [0.0, 0.3, 0.6]])
    rec = F.summarise(sse, ssim, 10, 10)
    assert set(rec) == {"psnr", "ssim"} and rec["psnr"]["identical_frames"] == 1
    assert rec["psnr"]["per_frame"] == [F.psnr_from_sse(sse[0], 100), math.inf, F.psnr_from_sse(sse[2], 100)]
    assert rec["psnr"]["mean"] == float(np.mean([rec["psnr"]["per_frame"][0], rec["psnr"]["per_frame"][2]]))
    assert rec["ssim"]["per_frame"] == [(0.5 + 0.25 + 0.75) / 3.0, 1.0, (0.0 + 0.3 + 0.6) / 3.0]
    assert rec["ssim"]["mean"] == float(np.mean(rec["ssim"]["per_frame"]))
    json.dumps(rec)
    alone = F.summarise(sse[1:2], ssim[1:2], 10, 10)
    assert alone["psnr"]["mean"] is None and alone["psnr"]["identical_frames"] == 1 and alone["ssim"]["mean"] == 1.0


def test_python_refusals():
    from aiod_amd import fidelity as F, flicker as K, guided as G
    img = np.zeros((8, 9, 3), np.uint8)
    for bad in (2, 8, 1, 17, 7.0, True, "7"):
        with pytest.raises(ValueError, match=r"frame_fidelity: win must be an odd integer in 3\.\.15"):
            F.frame_fidelity(img, img, win=bad)
    with pytest.raises(ValueError, match=r"frame_fidelity: a must be \(H, W, 3\) or \(N, H, W, 3\) uint8"):
        F.frame_fidelity(img.astype(np.float32), img)
    with pytest.raises(ValueError, match=r"frame_fidelity: b must be \(H, W, 3\) or \(N, H, W, 3\) uint8"):
        F.frame_fidelity(img, img[:, :, :2])
    with pytest.raises(ValueError, match=r"frame_fidelity: a is \(8, 9, 3\), b \(8, 8, 3\)"):
        F.frame_fidelity(img, img[:, :8])
    with pytest.raises(ValueError, match=r"frame_fidelity: the height must be in win\.\.16384 \(win 9\), got 8"):
        F.frame_fidelity(img, img, win=9)
    with pytest.raises(ValueError, match=r"frame_fidelity: the width must be in win\.\.16384 \(win 7\), got 6"):
        F.frame_fidelity(img[:, :6], img[:, :6])
    with pytest.raises(ValueError, match="want_map needs want_ssim"):
        F.frame_fidelity(img, img, want_map=True, want_ssim=False)
    with pytest.raises(ValueError, match="must be CUDA tensors"):
        F.frame_fidelity_device(img, img)
    planes = np.zeros((2, 2, 3), np.float32)
    with pytest.raises(ValueError, match=r"guided_apply: a must be \(h, w, 3\) float32"):
        G.guided_apply(img, planes.astype(np.float64), planes)
    with pytest.raises(ValueError, match=r"guided_apply: a is 2x2, b 1x2"):
        G.guided_apply(img, planes, planes[:, :1])
    with pytest.raises(ValueError, match=r"guided_apply: the proxy \(9x9\) is larger than the full frame \(9x8\)"):
        G.guided_apply(img, np.zeros((9, 9, 3), np.float32), np.zeros((9, 9, 3), np.float32))
    with pytest.raises(ValueError, match="must be CUDA tensors"):
        G.guided_apply_device(img, planes, planes)
    with pytest.raises(ValueError, match="kind must be one of global, local"):
        K.synth_flicker([img], kind="wavy")
    for bad in (-0.1, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="strength must be"):
            K.synth_flicker([img], strength=bad)
    for bad in ((0, 4), (4, 65), (4,), 4):
        with pytest.raises(ValueError, match="grid must be two integers"):
            K.synth_flicker([img], kind="local", grid=bad)
    with pytest.raises(ValueError, match=r"frame 0 \(9x8\) is smaller than the grid \(16x16\)"):
        K.synth_flicker([img], kind="local", grid=(16, 16))
    with pytest.raises(ValueError, match="no frames"):
        K.synth_flicker([])


def test_flicker_planes_follow_the_documented_draws():
    from aiod_amd import flicker as K
    for kind, shape in (("global", (1, 1, 3)), ("local", (3, 5, 3))):
        mine, ref = K.draw_planes(4, kind, 0.2, (3, 5), seed=9), R.flicker_planes(4, kind, 0.2, (3, 5), 9)
        assert len(mine) == 4
        for (a, b), (ra, rb) in zip(mine, ref):
            assert a.shape == b.shape == shape and a.dtype == b.dtype == np.float32
            assert np.array_equal(a, ra) and np.array_equal(b, rb)
            assert np.abs(a).max() <= 0.2 and np.abs(b).max() <= 64 * 0.2
    assert not np.array_equal(K.draw_planes(1, "global", 0.2, (4, 4), 0)[0][0], K.draw_planes(1, "global", 0.2, (4, 4), 1)[0][0])
    zero, _ = R.flicker([np.full((5, 6, 3), 77, np.uint8)], strength=0.0)
    assert np.array_equal(zero[0], np.full((5, 6, 3), 77, np.uint8))


# ---- the C refusals: before the device is touched ----------------------------------------------------------------------------------
def test_abi_refusals_come_before_the_device():
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    import aiod_amd
    lib = aiod_amd.load_library()
    u8 = np.zeros((2, 9, 10, 3), np.uint8)
    sse, ssim, smap = np.full((2, 3), 7, np.uint64), np.full((2, 3), 7.0), np.full((2, 3, 4, 3), 7.0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None      # noqa: E731

    def call(a=u8, b=u8, n=2, h=9, w=10, win=7, s=sse, m=ssim, mp=smap):
        return lib.af_fidelity(0, ptr(a), ptr(b), n, h, w, win, ptr(s), ptr(m), ptr(mp), 0)

    for fn, msg in ((lambda: call(a=None), "null pointer"), (lambda: call(b=None), "null pointer"),
                    (lambda: call(s=None, m=None, mp=None), "no output asked for"),
                    (lambda: call(m=None), "ssim_map needs ssim_out"),
                    (lambda: call(n=0), "n < 1"),
                    (lambda: call(win=6), "win must be odd and 3..15"), (lambda: call(win=1), "win must be odd and 3..15"),
                    (lambda: call(win=17), "win must be odd and 3..15"),
                    (lambda: call(h=6), "h must be win..16384"), (lambda: call(h=16385), "h must be win..16384"),
                    (lambda: call(w=6), "w must be win..16384"), (lambda: call(w=16385), "w must be win..16384")):
        assert fn() == -1, msg                                                      # AF_EINVAL
        assert lib.af_last_error(None).decode() == "af_fidelity: " + msg
    assert (sse == 7).all() and (ssim == 7.0).all() and (smap == 7.0).all()         # the outputs are untouched
    import torch
    if not torch.cuda.is_available():                         # a valid call needs the device: nothing is computed on the host
        assert call() == -2 and lib.af_last_error(None).decode().startswith("hipSetDevice: ")


# ---- the pipeline with stub engines ------------------------------------------------------------------------------------------------
class _Engines(TD._StubEngines):
    """The host stubs plus the proxy route's two calls and the fidelity call, which records the sizes it was given."""

    def shrink(self, frame, h, w):
        return np.full((h, w, 3), TD._ident(frame), np.uint8)

    def guided_transfer(self, full, proxy_in, proxy_out, radius, eps):
        return np.full(full.shape, TD._ident(full) + 100, np.uint8)

    def warp_error(self, img1, img2, f12, f21, align_corners):
        return 0.5

    def fidelity(self, a, b, win):
        assert len(a) == len(b)
        self.log.append(("fidelity", [TD._ident(x) for x in a], [tuple(x.shape) for x in a], [TD._ident(x) for x in b], [tuple(x.shape) for x in b], win))
        n = len(a)
        return np.full((n, 3), 12, np.uint64), np.full((n, 3), 0.5)


def _run(frames, engines=None, run_kw=None, **kw):
    import aiod_amd
    E = engines if engines is not None else _Engines()
    res = aiod_amd.Deflicker(None, None, None, config=TD.SMALL, down=4, seed=7, engines=E, **kw).run(frames, **(run_kw or {}))
    return E, res


def test_fidelity_none_adds_no_call_and_no_key():
    logs, results = [], []
    for run_kw in ({}, {"fidelity": None}, {"fidelity": False}):
        E, res = _run(TD._frames(4, 16, 40), run_kw=run_kw)
        logs.append(E.log)
        results.append(res)
    assert logs[0] == logs[1] == logs[2] and "fidelity" not in [e[0] for e in logs[0]]
    for res in results:
        assert "fidelity" not in res and set(res["seconds"]) == {"decode + flow", "stage 1", "stage 2", "total"}
    # an engine without the call serves the default as before, and is refused by name when the report is asked for
    E, res = _run(TD._frames(3), engines=TD._StubEngines())
    assert "fidelity" not in res
    with pytest.raises(ValueError, match="fidelity needs an engine with fidelity; _StubEngines has none"):
        _run(TD._frames(3), engines=TD._StubEngines(), run_kw={"fidelity": True})


def test_fidelity_true_makes_one_call_per_comparison():
    from aiod_amd import fidelity as F
    frames = TD._frames(4, 16, 40)
    plain_E, plain = _run(frames)
    E, res = _run(frames, run_kw={"fidelity": True})
    calls = [e for e in E.log if e[0] == "fidelity"]
    assert [e for e in E.log if e[0] != "fidelity"] == plain_E.log and np.array_equal(res["final"], plain["final"])
    assert calls == [("fidelity", [0, 1, 2, 3], [(16, 40, 3)] * 4, [0, 1, 2, 3], [(16, 40, 3)] * 4, 7)]
    assert E.log[-1][0] == "fidelity"                        # after the last stage
    expect = F.summarise(np.full((4, 3), 12, np.uint64), np.full((4, 3), 0.5), 16, 40)
    assert res["fidelity"] == {"window": 7, "size": [16, 40], "final_vs_input": expect}
    assert list(res["seconds"])[-2:] == ["fidelity", "total"]
    # a window of the caller's; a reference: three comparisons, the final first
    ref = [f + 50 for f in frames]
    E, res = _run(frames, run_kw={"fidelity": 11, "reference": ref, "warp_error": True})
    calls = [e for e in E.log if e[0] == "fidelity"]
    assert [(c[1], c[3], c[5]) for c in calls] == [([0, 1, 2, 3], [0, 1, 2, 3], 11), ([0, 1, 2, 3], [50, 51, 52, 53], 11), ([0, 1, 2, 3], [50, 51, 52, 53], 11)]
    assert set(res["fidelity"]) == {"window", "size", "final_vs_input", "input_vs_reference", "final_vs_reference"} and res["fidelity"]["window"] == 11
    assert {"warp error", "fidelity"} <= set(res["seconds"])


def test_fidelity_on_the_proxy_route_sees_full_size_frames():
    frames = TD._frames(4, 16, 40)
    ref = [f + 50 for f in frames]
    E, res = _run(iter(frames), run_kw={"fidelity": True, "reference": ref}, proxy_long_edge=20)
    assert res["proxy"]["size"] == [8, 20] and res["final"].shape == (4, 16, 40, 3)
    calls = [e for e in E.log if e[0] == "fidelity"]
    full = [(16, 40, 3)] * 4
    assert calls == [("fidelity", [100, 101, 102, 103], full, [0, 1, 2, 3], full, 7),            # the full-size final against the full-size input
                     ("fidelity", [0, 1, 2, 3], full, [50, 51, 52, 53], full, 7),
                     ("fidelity", [100, 101, 102, 103], full, [50, 51, 52, 53], full, 7)]
    assert res["fidelity"]["size"] == [16, 40]
    assert list(res["seconds"])[-2:] == ["fidelity", "total"] and "transfer" in res["seconds"]


def test_reference_refusals_come_before_any_work():
    frames = TD._frames(4, 16, 40)
    E = _Engines()
    for run_kw, msg in (({"reference": frames}, "reference belongs to the fidelity report: it needs fidelity"),
                        ({"fidelity": True, "reference": frames[:3]}, "3 reference frames for 4 frames"),
                        ({"fidelity": True, "reference": [f[:, :39] for f in frames]}, "reference frame 0 is 39x16, the clip 40x16"),
                        ({"fidelity": True, "reference": frames[:3] + [frames[3].astype(np.float32)]}, r"reference frame 3 must be \(H, W, 3\) uint8"),
                        ({"fidelity": True, "reference": iter(frames)}, "reference must be a sequence"),
                        ({"fidelity": 8}, r"fidelity: win must be an odd integer in 3\.\.15"),
                        ({"fidelity": 2.5}, r"fidelity: win must be an odd integer in 3\.\.15")):
        with pytest.raises(ValueError, match=msg):
            _run(frames, engines=E, run_kw=run_kw)
    assert E.log == []
    # the clip's length is not known before the decode: refused as soon as it is, before stage 1
    with pytest.raises(ValueError, match="3 reference frames for 4 frames"):
        _run(iter(frames), engines=E, run_kw={"fidelity": True, "reference": frames[:3]})
    assert "atlas_open" not in [e[0] for e in E.log] and "fidelity" not in [e[0] for e in E.log]
    E2 = _Engines()
    with pytest.raises(ValueError, match="reference frame 0 is 20x8, the clip 40x16"):      # the proxy's size is not the clip's
        _run(iter(frames), engines=E2, run_kw={"fidelity": True, "reference": [f[:8, :20] for f in frames]}, proxy_long_edge=20)
    assert "atlas_open" not in [e[0] for e in E2.log]


# ---- the CLIs ----------------------------------------------------------------------------------------------------------------------
def test_cli_flags():
    from aiod_amd import deflicker, fidelity as F, flicker as K
    o = deflicker.parse_args(["--frames_dir", "x"])
    assert o.fidelity is False and o.reference_dir is None and o.ssim_window is None
    o = deflicker.parse_args(["--frames_dir", "x", "--fidelity", "--reference_dir", "clean", "--ssim_window", "11"])
    assert o.fidelity and o.reference_dir == "clean" and o.ssim_window == 11
    for argv in (["--reference_dir", "clean"], ["--ssim_window", "7"], ["--fidelity", "--ssim_window", "8"], ["--fidelity", "--ssim_window", "17"]):
        with pytest.raises(SystemExit):
            deflicker.parse_args(["--frames_dir", "x"] + argv)
    R2 = TD._load("af_run_pipeline_fidelity", os.path.join(TD.PKG, "run_pipeline.py"))
    base = ["--video_frame_folder", "data/test/clip"]
    cmds = R2.build_commands(R2.parse_opts(base + ["--in_process", "--fidelity", "--reference_dir", "data/clean", "--ssim_window", "9"]))
    assert cmds[-1][1].endswith(" --fidelity --reference_dir data/clean --ssim_window 9")
    plain = R2.build_commands(R2.parse_opts(base + ["--in_process"]))
    assert "fidelity" not in plain[-1][1] and cmds[-1][1].startswith(plain[-1][1])
    for argv in (["--fidelity"], ["--in_process", "--ssim_window", "9"], ["--in_process", "--reference_dir", "d"]):
        with pytest.raises(SystemExit):
            R2.parse_opts(base + argv)
    a = F.parse_args(["--vid_name", "clip"])
    assert (a.root, a.results, a.reference_dir, a.ssim_window, a.gpu) == ("data/test/", "results", None, 7, 0)
    a = F.parse_args(["--vid_name", "clip", "--reference_dir", "c", "--ssim_window", "5", "--gpu", "1"])
    assert (a.reference_dir, a.ssim_window, a.gpu) == ("c", 5, 1)
    k = K.parse_args(["--frames_dir", "d", "--out", "o"])
    assert (k.kind, k.strength, k.grid, k.seed) == ("global", 0.1, (4, 4), 0)
    k = K.parse_args(["--frames_dir", "d", "--out", "o", "--kind", "local", "--strength", "0.3", "--grid", "2x6", "--seed", "4"])
    assert (k.kind, k.strength, k.grid, k.seed) == ("local", 0.3, (2, 6), 4)
    with pytest.raises(SystemExit):
        K.parse_args(["--frames_dir", "d", "--out", "o", "--grid", "4"])


def _write_seq(folder, n, h, w, value=0):
    from PIL import Image
    folder.mkdir(parents=True)
    for i in range(n):
        Image.fromarray(np.full((h, w, 3), value + i, np.uint8)).save(str(folder / ("%05d.png" % i)))


def test_report_discovers_the_sequences_and_skips_another_size(tmp_path, capsys):
    from aiod_amd import fidelity as F
    root, results = tmp_path / "data", tmp_path / "results"
    _write_seq(root / "clip", 3, 16, 20)
    _write_seq(results / "clip" / "stage_1" / "output", 3, 4, 5)
    _write_seq(results / "clip" / "neural_filter" / "output", 3, 16, 20, 10)
    _write_seq(results / "clip" / "final" / "output", 3, 16, 20, 20)
    _write_seq(tmp_path / "clean", 3, 16, 20, 30)
    plan, skipped, hw = F.plan_comparisons(root, results, "clip")
    assert hw == (16, 20) and [p[0] for p in plan] == ["neural_filter_vs_input", "final_vs_input"]
    assert [(s["stage"], s["height"], s["width"], s["frames"]) for s in skipped] == [("stage_1", 4, 5, 3)] and "nothing is resized" in skipped[0]["reason"]
    plan, _, _ = F.plan_comparisons(root, results, "clip", tmp_path / "clean")
    assert [p[0] for p in plan] == ["neural_filter_vs_input", "final_vs_input", "input_vs_reference", "neural_filter_vs_reference", "final_vs_reference"]
    assert [f.name for f in plan[2][1]] == ["%05d.png" % i for i in range(3)] and plan[2][2][0].parent == tmp_path / "clean"
    seen = []

    def stub(fa, fb, win, device):
        a, b = F.read_u8(fa[0]), F.read_u8(fb[0])
        seen.append((int(a[0, 0, 0]), int(b[0, 0, 0]), a.shape, win, device))
        return F.summarise(np.full((len(fa), 3), 5, np.uint64), np.full((len(fa), 3), 0.25), *a.shape[:2])

    args = F.parse_args(["--vid_name", "clip", "--root", str(root), "--results", str(results), "--reference_dir", str(tmp_path / "clean"), "--ssim_window", "5"])
    rep = F.run(args, measure_fn=stub)
    assert seen == [(10, 0, (16, 20, 3), 5, 0), (20, 0, (16, 20, 3), 5, 0), (0, 30, (16, 20, 3), 5, 0), (10, 30, (16, 20, 3), 5, 0), (20, 30, (16, 20, 3), 5, 0)]
    assert json.loads((results / "clip" / "fidelity.json").read_text()) == rep
    assert rep["window"] == 5 and rep["size"] == [16, 20] and list(rep["comparisons"]) == [p[0] for p in plan]
    assert rep["comparisons"]["final_vs_input"]["frames"] == 3 and rep["comparisons"]["final_vs_input"]["ssim"]["mean"] == 0.25
    assert [s["stage"] for s in rep["skipped"]] == ["stage_1"]
    text = capsys.readouterr().out
    assert "final_vs_reference" in text and "stage_1" in text and "skipped: 5x4" in text
    # refusals of the tree
    with pytest.raises(SystemExit, match="no input frames under"):
        F.plan_comparisons(root, results, "other")
    with pytest.raises(SystemExit, match="no reference frames"):
        F.plan_comparisons(root, results, "clip", tmp_path / "nowhere")
    _write_seq(tmp_path / "short", 2, 16, 20)
    with pytest.raises(SystemExit, match="2 frames, the input has 3"):
        F.plan_comparisons(root, results, "clip", tmp_path / "short")
    with pytest.raises(SystemExit, match=r"--ssim_window: win must be an odd integer"):
        F.run(F.parse_args(["--vid_name", "clip", "--root", str(root), "--results", str(results), "--ssim_window", "4"]), measure_fn=stub)


def test_deflicker_cli_writes_the_fidelity_record(tmp_path):
    from PIL import Image
    from aiod_amd import deflicker
    clip, clean = tmp_path / "clip", tmp_path / "clean"
    _write_seq(clip, 3, 16, 40)
    _write_seq(clean, 3, 16, 40, 50)
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps(TD.SMALL))
    base = ["--frames_dir", str(clip), "--config", str(cfg), "--seed", "1"]
    for k, (extra, keys) in enumerate(((["--fidelity", "--reference_dir", str(clean), "--ssim_window", "9"], {"window", "size", "final_vs_input", "input_vs_reference", "final_vs_reference"}),
                                       (["--fidelity"], {"window", "size", "final_vs_input"}), ([], None))):
        out = tmp_path / ("out%d" % k)
        E = _Engines()
        assert deflicker.main(base + ["--out", str(out)] + extra, engines=E) == 0
        rec = json.loads((out / "deflicker.json").read_text())
        assert ("fidelity" in rec) == (keys is not None) == ("fidelity" in rec["seconds"]) == ("reference_dir" in rec)
        if keys is not None:
            assert set(rec["fidelity"]) == keys and rec["fidelity"]["window"] == (9 if "--ssim_window" in extra else 7) and rec["fidelity"]["size"] == [16, 40]
            assert rec["fidelity"]["final_vs_input"]["ssim"]["mean"] == 0.5
        if "--reference_dir" in extra:
            assert [e[3] for e in E.log if e[0] == "fidelity"][1] == [50, 51, 52]
        assert len(list((out / "final" / "output").iterdir())) == 3
    _write_seq(tmp_path / "short", 2, 16, 40)
    with pytest.raises(SystemExit, match="2 reference frames under .* for 3 frames"):
        deflicker.main(base + ["--out", str(tmp_path / "o"), "--fidelity", "--reference_dir", str(tmp_path / "short")], engines=_Engines())
    with pytest.raises(SystemExit, match="no reference frames"):
        deflicker.main(base + ["--out", str(tmp_path / "o"), "--fidelity", "--reference_dir", str(tmp_path / "nowhere")], engines=_Engines())


def test_flicker_cli_writes_frames_and_parameters(tmp_path):
    from PIL import Image
    from aiod_amd import flicker as K
    _write_seq(tmp_path / "clip", 3, 8, 9, 40)
    seen = {}

    def stub(frames, **kw):
        seen.update(kw, n=len(frames))
        return np.stack([f + 1 for f in frames]), None

    assert K.main(["--frames_dir", str(tmp_path / "clip"), "--out", str(tmp_path / "o"), "--kind", "local", "--grid", "2x3", "--seed", "5"], apply_fn=stub) == 0
    assert seen == {"kind": "local", "strength": 0.1, "grid": (2, 3), "seed": 5, "device": 0, "n": 3}
    assert [int(np.asarray(Image.open(str(tmp_path / "o" / ("%05d.png" % i))))[0, 0, 0]) for i in range(3)] == [41, 42, 43]
    rec = json.loads((tmp_path / "o" / "flicker.json").read_text())
    assert rec["kind"] == "local" and rec["grid"] == [2, 3] and rec["seed"] == 5 and rec["frames"] == 3 and rec["strength"] == 0.1
    with pytest.raises(SystemExit, match="no frames"):
        K.main(["--frames_dir", str(tmp_path / "none"), "--out", str(tmp_path / "o2")], apply_fn=stub)
