"""Host-side checks of the --max_long_edge shrink (no GPU): the size rule, the numpy restatement of cv2.INTER_AREA
(tests/resize_area_ref.py) against an independent exact area average, and the orchestration of the flow CLI and of Deflicker.run with
stub engines.

The bound of the restatement against the exact average is derived: the restatement rounds the area average to the nearest integer
(half to even, or half up on the 2x2 integer path), so it is within 0.5 of the exact value, plus the fp32 error of the weights and of
at most a few dozen accumulations of values <= 255 (a few 1e-5), taken generously as 1e-3."""
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "all-in-one-deflicker_amd")
sys.path.insert(0, HERE)
import resize_area_ref as R  # noqa: E402
import test_deflicker_host as TD  # noqa: E402      (the stub engines of the one-process pipeline)
import test_raft_host as TR  # noqa: E402           (the stub RAFT handle of the flow CLI)

BOUND = 0.5 + 1e-3


def _cli(name="af_pof_area"):
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, "preprocess_optical_flow.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- the size rule -------------------------------------------------------------------------------------------------------------
def test_shrink_size_is_the_references_rule():
    cli = _cli()
    assert cli.shrink_size(2160, 3840, 2000) == (1125, 2000)
    assert cli.shrink_size(1716, 4096, 2000) == (837, 1999)          # float floor division: 4096 // 2.048 is 1999.0
    assert cli.shrink_size(16, 40, 39) == (15, 39)
    assert cli.shrink_size(9, 10, 9) == (8, 8)
    for h, w, m in ((1080, 1920, 2000), (2000, 1500, 2000), (16, 40, 40), (1, 1, 1)):
        assert cli.shrink_size(h, w, m) is None                      # factor <= 1
    with pytest.raises(ValueError, match="00007.png is 4000x1"):     # a zero side is refused, naming the frame
        cli.shrink_size(1, 4000, 2000, name="00007.png")
    with pytest.raises(ValueError, match="max_long_edge"):
        cli.shrink_size(10, 10, 0)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_restatement_is_an_area_average(shape):
    sh, sw, dh, dw = shape
    assert R.is_fast(sh, sw, dh, dw) == (shape not in R.GENERAL)
    rnd, zeros, full = R.inputs(sh, sw)
    got = R.resize_area(rnd, dh, dw)
    assert got.dtype == np.uint8 and got.shape == (dh, dw, 3)
    err = float(np.abs(got.astype(np.float64) - R.exact_area(rnd, dh, dw)).max())
    print("%s: max |u8 - exact| = %.4f" % (shape, err))
    assert err <= BOUND
    assert (R.resize_area(zeros, dh, dw) == 0).all() and (R.resize_area(full, dh, dw) == 255).all()      # a constant image stays constant
    assert (R.resize_area(np.full((sh, sw, 3), 77, np.uint8), dh, dw) == 77).all()


def test_restatement_two_by_two_rules_and_tables():
    # 2x2 with 1, 3 and 4 channels is the integer (s + 2) >> 2 (a half rounds up); with 2 channels it is the float product (half to even)
    img = np.zeros((2, 2, 1), np.uint8)
    img[0, 0] = 2                                                    # block sum 2: 0.5 -> 1 on the integer path, 0 on the float path
    for ch, want in ((1, 1), (2, 0), (3, 1), (4, 1)):
        assert (R.resize_area(np.repeat(img, ch, axis=2), 1, 1) == want).all(), ch
    img[0, 0] = 6                                                    # 1.5 -> 2 on both
    for ch in (1, 2, 3, 4):
        assert (R.resize_area(np.repeat(img, ch, axis=2), 1, 1) == 2).all()
    # the table of 23 -> 11: every destination's weights sum to 1, the last cell is clipped at the source's edge
    tab = R.area_table(23, 11)
    for d in range(11):
        assert abs(sum(float(w) for dd, _, w in tab if dd == d) - 1.0) < 1e-6
    assert max(s for _, s, _ in tab) == 22 and min(s for _, s, _ in tab) == 0
    assert [d for d, _, _ in tab] == sorted(d for d, _, _ in tab)


# ---- the flow CLI with stubs ---------------------------------------------------------------------------------------------------
def test_cli_shrinks_before_raft(tmp_path):
    from PIL import Image
    cli = _cli("af_pof_area2")
    vid = tmp_path / "big"
    vid.mkdir()
    names = ["a.png", "b.png", "c.png"]
    for i, n in enumerate(names):
        Image.fromarray(np.full((16, 40, 3), i, np.uint8)).save(vid / n)
    stubs, shrunk = [], []

    def make(h, w):
        stubs.append(TR._StubFlow(h, w, 2))
        return stubs[-1]

    def shrink(img, h, w):
        assert img.dtype == np.uint8 and img.shape == (16, 40, 3)
        shrunk.append((int(img[0, 0, 0]), h, w))
        return np.full((h, w, 3), img[0, 0, 0], np.uint8)
    args = cli.parse_args(["--vid-path", str(vid), "--max_long_edge", "39"])
    assert cli.preprocess(args, make, shrink) == 2
    assert shrunk == [(0, 15, 39), (1, 15, 39), (2, 15, 39)]                       # every frame once, at the reference's size
    assert len(stubs) == 1 and (stubs[0].h, stubs[0].w) == (15, 39) and stubs[0].encoded == [0, 1, 2]
    f = np.load(tmp_path / "big_flow" / "a.png_b.png.npy")
    assert f.dtype == np.float32 and f.shape == (16, 40, 2) and f[0, 0, 0] == 1.0   # the padded shrunk size
    assert np.load(tmp_path / "big_flow" / "c.png_b.png.npy")[0, 0, 0] == 21.0
    # the frame-size check compares the sizes as decoded
    Image.fromarray(np.zeros((16, 41, 3), np.uint8)).save(vid / "d.png")
    with pytest.raises(SystemExit, match="d.png is 41x16, the first frame 40x16"):
        cli.preprocess(args, make, shrink)
    # below the limit the shrinker is not called
    shrunk.clear()
    os.remove(vid / "d.png")
    for p in (tmp_path / "big_flow").iterdir():
        p.unlink()
    assert cli.preprocess(cli.parse_args(["--vid-path", str(vid), "--max_long_edge", "40"]), make, shrink) == 2
    assert shrunk == [] and (stubs[-1].h, stubs[-1].w) == (16, 40)
    # a shrinker that returns the wrong thing is caught
    for p in (tmp_path / "big_flow").iterdir():
        p.unlink()
    with pytest.raises(SystemExit, match="shrinker returned"):
        cli.preprocess(args, make, lambda img, h, w: img)


# ---- Deflicker.run with stub engines -------------------------------------------------------------------------------------------
class _Engines(TD._StubEngines):
    """The host stubs plus a shrinker; records what the builder and the filter are given."""

    def shrink(self, frame, h, w):
        assert frame.dtype == np.uint8
        self.log.append(("shrink", TD._ident(frame), tuple(frame.shape[:2]), h, w))
        return np.full((h, w, 3), TD._ident(frame), np.uint8)

    def inputs(self, frames, flows12, flows21, resy, resx):
        self.log.append(("inputs", [tuple(f.shape) for f in frames], resy, resx, [f[2:] for f in flows12]))
        return super().inputs(frames, flows12, flows21, resy, resx)

    def resize(self, img, h, w):
        self.log.append(("resize", tuple(np.asarray(img).shape), h, w))
        return super().resize(img, h, w)


def test_deflicker_shrinks_for_raft_only():
    import aiod_amd
    E = _Engines()
    d = aiod_amd.Deflicker(None, None, None, config=TD.SMALL, down=4, seed=7, max_long_edge=39, engines=E)
    res = d.run(TD._frames(4, 16, 40), keep=("final", "flows"))
    log = E.log
    assert [e for e in log if e[0] == "raft_open"] == [("raft_open", 15, 39)]                       # RAFT at the shrunk size
    assert [e for e in log if e[0] == "shrink"] == [("shrink", i, (16, 40), 15, 39) for i in range(4)]      # every frame once, full size in
    assert [e[1] for e in log if e[0] == "encode"] == [0, 1, 2, 3]                                  # (the stub RAFT asserts the 15x39 shape)
    names = [e[0] for e in log]
    assert [n for n in names if n in ("shrink", "encode", "flow")] == ["shrink", "encode"] + ["shrink", "encode", "flow"] * 3
    # the builder gets the full-size frames and flows resized to (resy, resx) of the full-size frames
    (inp,) = [e for e in log if e[0] == "inputs"]
    assert inp[1] == [(16, 40, 3)] * 4 and inp[2:4] == (4, 10) and inp[4] == [(4, 10)] * 3
    assert [e for e in log if e[0] == "atlas_open"] == [("atlas_open", 10, 4, 4)]
    # stage 2 runs at the full size, on the full-size frames
    assert [e for e in log if e[0] == "filter_open"] == [("filter_open", 16, 40)]
    assert [e[1] for e in log if e[0] == "resize"][:1] == [(16, 40, 3)] and all(e[2:] == (16, 40) for e in log if e[0] == "resize")
    assert res["final"].shape == (4, 16, 40, 3)
    assert len(res["flows"]) == 3 and res["flows"][0][0].shape == (15, 39, 2)                       # the kept flows: what RAFT returned
    assert res["flow_size"] == [15, 39] and res["max_long_edge"] == 39


def test_deflicker_below_the_limit_calls_what_it_called_before():
    import aiod_amd
    logs = []
    for engines, mle in ((_Engines(), 2000), (_Engines(), 12), (TD._StubEngines(), 2000)):      # the last: stubs without a shrinker keep working
        d = aiod_amd.Deflicker(None, None, None, config=TD.SMALL, down=4, seed=7, max_long_edge=mle, engines=engines)
        res = d.run(TD._frames(4))
        assert res["flow_size"] == [8, 12] and res["max_long_edge"] == mle
        logs.append([e for e in engines.log if e[0] not in ("inputs", "resize")])
    assert logs[0] == logs[1] == logs[2] and "shrink" not in [e[0] for e in logs[0]]
    # ... and the RAFT stage is the sequence the pipeline has always made: open at the frames' size, one encode per frame, both
    # directions per pair as soon as its second frame is encoded, close
    raft = [e for e in logs[0] if e[0] in ("raft_open", "encode", "flow", "raft_close")]
    want = [("raft_open", 8, 12), ("encode", 0)]
    for i in range(1, 4):
        want += [("encode", i), ("flow", [(i - 1, i), (i, i - 1)])]
    assert raft == want + [("raft_close",)]
    assert logs[0][:len(raft)] == raft                                                             # nothing else in between


def test_deflicker_cli_flag():
    from aiod_amd import deflicker
    assert deflicker.parse_args(["--frames_dir", "x"]).max_long_edge == 2000
    assert deflicker.parse_args(["--frames_dir", "x", "--max_long_edge", "192"]).max_long_edge == 192
    import aiod_amd
    E = _Engines()
    with pytest.raises(ValueError, match="frame 0 is 4000x1"):
        aiod_amd.Deflicker(None, None, None, config=TD.SMALL, seed=1, max_long_edge=2000, engines=E).run([np.zeros((1, 4000, 3), np.uint8)] * 2)
    assert "raft_open" not in [e[0] for e in E.log]


# ---- the ABI without a GPU -----------------------------------------------------------------------------------------------------
def test_argument_errors_need_no_device_and_there_is_no_cpu_path():
    import ctypes as C
    import torch
    import __graft_entry__ as ge
    ge.build()
    import aiod_amd
    lib = aiod_amd.load_library()
    src, dst = np.zeros((6, 8, 3), np.uint8), np.zeros((6, 8, 3), np.uint8)
    ps, pd = src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p)
    for args, msg in (((None, 6, 8, 3, pd, 3, 4), "null pointer"), ((ps, 6, 8, 3, pd, 0, 4), "dh < 1"), ((ps, 6, 8, 3, pd, 3, 0), "dw < 1"),
                      ((ps, 6, 8, 3, pd, 7, 4), "dh > sh"), ((ps, 6, 8, 3, pd, 3, 9), "dw > sw"), ((ps, 6, 8, 3, pd, 6, 8), "dh == sh && dw == sw")):
        assert lib.af_resize_area(0, *args, 0) == -1 and lib.af_last_error(None).decode().startswith("af_resize_area: " + msg)
    if not torch.cuda.is_available():
        with pytest.raises(aiod_amd.AtlasFitError, match="hipSetDevice"):      # a missing device is an error, never a host resize
            aiod_amd.resize_area(src, 3, 4)
