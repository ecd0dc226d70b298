"""The --max_long_edge shrink on the GPU: k_resize_area (af_resize_area) and the routes that use it.

Every comparison of bytes here is exact.  The kernel is held against the numpy restatement of OpenCV 4.x's INTER_AREA arithmetic
(tests/resize_area_ref.py): each output value sees the same fp32 operations in the same order (no contraction), so the tolerance is
zero.  Against the exact fp64 area average the bound is 0.5 (the rounding to uint8) + 1e-3 (generous for the fp32 weights and sums).
The flow CLI and the one-process pipeline run the same kernels on the same values as the routes they are compared with (the
argument of tests/test_gpu_deflicker.py), so those tolerances are zero too.  Parity with OpenCV's own bytes is not tested here:
tests/test_resize_area_cv2.py does that once its fixture exists."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pipeline_bench as PB  # noqa: E402
import resize_area_ref as R  # noqa: E402

CASES = [(s, 3) for s in R.SHAPES] + [((20, 30, 10, 15), 1), ((20, 30, 10, 15), 2)]      # one- and two-channel 2x2: both 2x2 rules
H, W, EDGE, SMALL_HW, PADDED, DOWN, SEED = 200, 288, 192, (133, 192), (136, 192), 4, 11
SHORT = {"samples_batch": 1024, "iters_num": 31, "evaluate_every": 30, "pretrain_iter_number": 3, "stop_global_rigidity": 15}


@pytest.fixture(scope="module")
def expected():
    """(shape, ch) -> [(image, restatement)] for the random, the all-0 and the all-255 image: computed once, shared, never written to."""
    out = {}
    for (sh, sw, dh, dw), ch in CASES:
        out[(sh, sw, dh, dw), ch] = [(img, R.resize_area(img, dh, dw)) for img in R.inputs(sh, sw, ch)]
    return out


# ---- the kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-%dx%d-c%d" % (c[0] + (c[1],)))
def test_kernel_equals_restatement_bitwise(case, expected):
    import aiod_amd
    (sh, sw, dh, dw), ch = case
    for img, want in expected[case]:
        host = aiod_amd.resize_area(img, dh, dw)
        dev = aiod_amd.resize_area_device(torch.from_numpy(img).cuda(), dh, dw)
        assert host.dtype == np.uint8 and host.shape == (dh, dw, ch) and dev.is_cuda and dev.dtype == torch.uint8 and tuple(dev.shape) == (dh, dw, ch)
        diff = int((host != want).sum())
        print("%s c%d: %d of %d values differ from the restatement" % ((sh, sw, dh, dw), ch, diff, want.size))
        assert diff == 0
        assert np.array_equal(dev.cpu().numpy(), host)                                            # device pointers == host pointers
        assert np.array_equal(aiod_amd.resize_area(img, dh, dw), host)                            # and a second run
        assert np.array_equal(aiod_amd.resize_area_device(torch.from_numpy(img).cuda(), dh, dw).cpu().numpy(), host)
    if ch == 1:                                                                                   # the 2-D form of the numpy wrapper
        img = expected[case][0][0]
        assert np.array_equal(aiod_amd.resize_area(img[:, :, 0], dh, dw), expected[case][0][1][:, :, 0])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-%dx%d-c%d" % (c[0] + (c[1],)))
def test_kernel_is_an_area_average(case, expected):
    import aiod_amd
    (sh, sw, dh, dw), ch = case
    img = expected[case][0][0]
    got = aiod_amd.resize_area(img, dh, dw).astype(np.float64)
    err = float(np.abs(got - R.exact_area(img, dh, dw)).max())
    print("%s c%d: max |kernel - exact area average| = %.4f" % ((sh, sw, dh, dw), ch, err))
    assert err <= 0.5 + 1e-3


def test_argument_errors():
    import aiod_amd
    lib = aiod_amd.load_library()
    src = np.zeros((6, 8, 3), np.uint8)
    dst = np.zeros((6, 8, 3), np.uint8)
    ps, pd = src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p)

    def call(s, sh, sw, ch, d, dh, dw):
        rc = lib.af_resize_area(0, s, sh, sw, ch, d, dh, dw, 0)
        return rc, lib.af_last_error(None).decode()
    for args, msg in (((None, 6, 8, 3, pd, 3, 4), "null pointer"), ((ps, 6, 8, 3, None, 3, 4), "null pointer"),
                      ((ps, 6, 8, 3, pd, 0, 4), "dh < 1"), ((ps, 6, 8, 3, pd, 3, 0), "dw < 1"), ((ps, 6, 8, 3, pd, -1, 4), "dh < 1"),
                      ((ps, 6, 8, 3, pd, 7, 4), "dh > sh"), ((ps, 6, 8, 3, pd, 3, 9), "dw > sw"),
                      ((ps, 6, 8, 3, pd, 6, 8), "dh == sh && dw == sw"), ((ps, 6, 8, 5, pd, 3, 4), "ch must be 1..4"),
                      ((ps, 6, 8, 0, pd, 3, 4), "ch must be 1..4")):
        rc, text = call(*args)
        assert rc == -1 and text.startswith("af_resize_area: " + msg), (args[1:4] + args[5:], rc, text)      # AF_EINVAL
    with pytest.raises(aiod_amd.AtlasFitError, match="dh > sh"):
        aiod_amd.resize_area(src, 7, 4)
    with pytest.raises(aiod_amd.AtlasFitError, match="dh == sh && dw == sw"):
        aiod_amd.resize_area_device(torch.from_numpy(src).cuda(), 6, 8)
    with pytest.raises(ValueError, match="uint8"):
        aiod_amd.resize_area(src.astype(np.float32), 3, 4)
    assert np.array_equal(aiod_amd.resize_area(src + 9, 3, 4), np.full((3, 4, 3), 9, np.uint8))       # and the library still works
    assert aiod_amd.resize_area(src, 6, 4).shape == (6, 4, 3) and aiod_amd.resize_area(src, 1, 8).shape == (1, 8, 3)      # one axis may keep its size


# ---- the routes ----------------------------------------------------------------------------------------------------------------
def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _run(cmd, cwd):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, " ".join(str(c) for c in cmd) + "\n" + r.stdout[-2000:] + r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    d = tmp_path_factory.mktemp("resize_area_assets")
    weights = PB.synthetic_weights()
    cfg = dict(REFERENCE_CONFIG, **SHORT)
    with open(d / "short.json", "w") as f:
        json.dump(cfg, f)
    return {"weights": weights, "paths": PB.write_weights(str(d / "weights"), weights), "cfg": cfg, "cfg_path": str(d / "short.json"),
            "frames": PB.synthetic_clip(4, H, W, seed=5)}


def test_flow_cli_shrinks_with_the_kernel(assets, tmp_path):
    import aiod_amd
    from aiod_amd import preprocess_optical_flow as cli
    frames = assets["frames"]
    assert cli.shrink_size(H, W, EDGE) == SMALL_HW
    PB.write_clip(str(tmp_path / "clip"), frames)
    assert cli.main(["--vid-path", str(tmp_path / "clip"), "--max_long_edge", str(EDGE), "--model", assets["paths"][0]]) == 0
    names = ["%05d.png" % i for i in range(len(frames))]
    small = [aiod_amd.resize_area(f, *SMALL_HW) for f in frames]
    assert all(np.array_equal(s, R.resize_area(f, *SMALL_HW)) for s, f in zip(small, frames))
    raft = aiod_amd.RAFT(*SMALL_HW, capacity=2)
    try:
        raft.load_state_dict(assets["weights"][0])
        for i in range(len(frames) - 1):
            raft.encode(0, small[i])
            raft.encode(1, small[i + 1])
            f12, f21 = raft.flow_slots([(0, 1), (1, 0)])
            for want, (a, b) in ((f12, (i, i + 1)), (f21, (i + 1, i))):
                got = np.load(tmp_path / "clip_flow" / ("%s_%s.npy" % (names[a], names[b])))
                assert got.dtype == np.float32 and got.shape == PADDED + (2,)
                assert np.array_equal(got.view(np.uint32), np.asarray(want, np.float32).view(np.uint32)), "flow %d -> %d differs" % (a, b)
    finally:
        raft.close()
    assert len(os.listdir(tmp_path / "clip_flow")) == 2 * (len(frames) - 1)


def test_pipeline_identity_with_the_chained_clis_when_shrinking(assets, tmp_path):
    import aiod_amd
    frames = assets["frames"]
    n = len(frames)
    roots = {arm: tmp_path / arm for arm in ("in_process", "chained")}
    for r in roots.values():
        PB.write_clip(str(r / "data" / "test" / "clip"), frames)
    out = roots["in_process"] / "anywhere" / "clip"
    _run(PB.in_process_command(str(roots["in_process"] / "data" / "test" / "clip"), str(out), assets["cfg_path"], DOWN, SEED, assets["paths"],
                               extra=["--max_long_edge", str(EDGE), "--keep_intermediates", "--warp_error"]), tmp_path)
    for name, cmd in PB.chained_commands("clip", assets["cfg_path"], DOWN, SEED, assets["paths"]):
        _run(cmd + (["--max_long_edge", str(EDGE)] if name == "flow" else []), roots["chained"])
    ref = roots["chained"] / "results" / "clip"
    names = ["%05d.png" % i for i in range(n)]
    # flows: equal arrays of the padded shrunk size
    fa, fb = roots["in_process"] / "data" / "test" / "clip_flow", roots["chained"] / "data" / "test" / "clip_flow"
    flow_names = sorted(os.listdir(fb))
    assert len(flow_names) == 2 * (n - 1) and sorted(os.listdir(fa)) == flow_names
    for fn in flow_names:
        x, y = np.load(fa / fn), np.load(fb / fn)
        assert x.shape == y.shape == PADDED + (2,) and x.dtype == y.dtype == np.float32
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "flow %s differs" % fn
    # stage 1 and the final frames: identical decoded pixels, at the sizes of the full-size frames
    for sub in (("stage_1", "output"), ("final", "output")):
        a, b = out.joinpath(*sub), ref.joinpath(*sub)
        assert sorted(os.listdir(a)) == names == sorted(os.listdir(b)), sub
        for fn in names:
            x, y = _png(a / fn), _png(b / fn)
            assert x.dtype == np.uint8 and x.shape == y.shape and np.array_equal(x, y), "%s/%s differs in %d values" % ("/".join(sub), fn, int((x != y).sum()))
    assert _png(out / "stage_1" / "output" / names[0]).shape == (H // DOWN, W // DOWN, 3)
    assert _png(out / "final" / "output" / names[0]).shape == (H, W, 3)
    rec = json.load(open(out / "deflicker.json"))
    assert rec["flow_size"] == list(SMALL_HW) and rec["max_long_edge"] == EDGE and rec["windows"] == [[0, n]]
    # E_warp rescales the shrunk flows to the frames: the figures warp_error.py measures on the chained route's files
    from aiod_amd import warp_error as WE
    files = WE.list_frames(roots["chained"] / "data" / "test" / "clip")
    pairs = WE.flow_pairs(files, fb)
    assert WE.measure_sequence(files, pairs, True)[1] == rec["warp_error"]["input"]["per_pair"]
    assert WE.measure_sequence(WE.list_frames(ref / "final" / "output"), pairs, True)[1] == rec["warp_error"]["final"]["per_pair"]
    # the API gives the CLI's frames, and its kept flows are the saved ones
    final_files = np.stack([_png(out / "final" / "output" / fn) for fn in names])
    r = aiod_amd.Deflicker(*assets["weights"], config=assets["cfg"], down=DOWN, seed=SEED, max_long_edge=EDGE).run(frames, keep=("final", "flows"))
    assert np.array_equal(r["final"], final_files) and r["flow_size"] == list(SMALL_HW)
    assert np.array_equal(r["flows"][0][0].cpu().numpy(), np.load(fa / ("%s_%s.npy" % (names[0], names[1]))))


def test_pipeline_below_the_limit_is_unchanged(assets, tmp_path):
    """--max_long_edge 2000 on the same clip: no shrink, and the bytes of the call that never mentions the limit (the code path the
    pipeline had before it could shrink)."""
    import aiod_amd
    frames = assets["frames"]
    PB.write_clip(str(tmp_path / "clip"), frames)
    out = tmp_path / "out"
    _run(PB.in_process_command(str(tmp_path / "clip"), str(out), assets["cfg_path"], DOWN, SEED, assets["paths"],
                               extra=["--max_long_edge", "2000", "--keep_intermediates"]), tmp_path)
    names = ["%05d.png" % i for i in range(len(frames))]
    rec = json.load(open(out / "deflicker.json"))
    assert rec["flow_size"] == [H, W] and rec["max_long_edge"] == 2000
    r = aiod_amd.Deflicker(*assets["weights"], config=assets["cfg"], down=DOWN, seed=SEED).run(frames, keep=("final", "stage1", "flows"))
    assert np.array_equal(r["final"], np.stack([_png(out / "final" / "output" / fn) for fn in names]))
    assert np.array_equal(r["stage1"], np.stack([_png(out / "stage_1" / "output" / fn) for fn in names]))
    for i, (f12, f21) in enumerate(r["flows"]):
        assert tuple(f12.shape) == (H, W, 2)                                                      # 200 x 288 needs no padding
        assert np.array_equal(f12.cpu().numpy(), np.load(tmp_path / "clip_flow" / ("%s_%s.npy" % (names[i], names[i + 1]))))
        assert np.array_equal(f21.cpu().numpy(), np.load(tmp_path / "clip_flow" / ("%s_%s.npy" % (names[i + 1], names[i]))))
