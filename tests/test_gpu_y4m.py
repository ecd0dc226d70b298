"""The YUV4MPEG2 route on the GPU: k_yuv_to_rgb / k_rgb_to_yuv (csrc/yuv.hip, af_yuv_to_rgb / af_rgb_to_yuv) and
deflicker.py --video / --video_out.

Every comparison is exact.  The kernels compute in integers, so they must equal the whole-array numpy restatement (tests/y4m_ref.py,
itself held against an fp64 exact twin and against Pillow in tests/test_y4m_host.py) bit for bit; the pipeline sees, from a stream, the
tensors a folder of PNGs with the same pixels gives it, so its frames must be the same bytes.

Pipeline inputs: the 130x197 synthetic clip (5 frames), the SHORT config and the synthetic weights of tests/test_gpu_deflicker.py."""
import ctypes as C
import io
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
import y4m_ref as R  # noqa: E402
import pipeline_bench as PB  # noqa: E402

PKG = PB.PKG
SIZES = ((1, 1), (2, 2), (3, 2), (3, 3), (1, 8), (8, 1), (7, 5), (130, 9), (197, 130))      # (w, h): odd edges on both axes, single-sample planes, both sitings' border clamps, columns past a workgroup's first 64 blocks, more than one workgroup
H, W, N, DOWN, SEED = 130, 197, 5, 4, 11
SHORT = {"samples_batch": 1024, "iters_num": 31, "evaluate_every": 30, "pretrain_iter_number": 3, "stop_global_rigidity": 15}


# ---- the kernels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_kernels_equal_numpy(layout):
    import aiod_amd
    lib = aiod_amd.load_library()
    for w, h in SIZES:
        assert lib.af_yuv_frame_bytes(h, w, R.LAYOUTS.index(layout)) == R.frame_bytes(h, w, layout) == aiod_amd.y4m.frame_bytes(h, w, layout)
        for matrix in R.MATRICES:
            for full in (False, True):
                for name, payload in R.inputs(h, w, layout):
                    want = R.yuv_to_rgb(payload, h, w, layout, matrix, full)
                    host = aiod_amd.yuv_to_rgb(payload, h, w, layout, matrix, full)                       # host pointers
                    dev = aiod_amd.yuv_to_rgb_device(torch.from_numpy(payload).cuda(), h, w, layout, matrix, full)      # device pointers
                    assert host.shape == (h, w, 3) and dev.is_cuda and dev.dtype == torch.uint8
                    assert np.array_equal(host, want), ("read", w, h, matrix, full, name, int(np.abs(host.astype(int) - want).max()))
                    assert np.array_equal(dev.cpu().numpy(), want), ("read, device", w, h, matrix, full, name)
                    assert np.array_equal(aiod_amd.yuv_to_rgb(payload.tobytes(), h, w, layout, matrix, full), want)      # and a second run
                for name, img in R.rgb_inputs(h, w):
                    want = R.rgb_to_yuv(img, layout, matrix, full)
                    host = aiod_amd.rgb_to_yuv(img, layout, matrix, full)
                    dev = aiod_amd.rgb_to_yuv_device(torch.from_numpy(img).cuda(), layout, matrix, full)
                    assert host.shape == (R.frame_bytes(h, w, layout),) and dev.is_cuda and dev.dtype == torch.uint8
                    assert np.array_equal(host, want), ("write", w, h, matrix, full, name, int(np.abs(host.astype(int) - want).max()))
                    assert np.array_equal(dev.cpu().numpy(), want), ("write, device", w, h, matrix, full, name)
                    assert np.array_equal(aiod_amd.rgb_to_yuv(img, layout, matrix, full), want)


def test_refusals_name_the_cause():
    import aiod_amd
    lib = aiod_amd.load_library()
    buf = np.zeros(16384 * 3 + 64, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    for fn in ("af_yuv_to_rgb", "af_rgb_to_yuv"):
        for args, msg in (((None, 4, 4, 2, 0, 0, p), "null pointer"), ((p, 4, 4, 2, 0, 0, None), "null pointer"),
                          ((p, 0, 4, 2, 0, 0, p), "h must be 1..16384"), ((p, 16385, 1, 2, 0, 0, p), "h must be 1..16384"),
                          ((p, 4, 0, 2, 0, 0, p), "w must be 1..16384"), ((p, 1, 16385, 2, 0, 0, p), "w must be 1..16384"),
                          ((p, 4, 4, 5, 0, 0, p), "unknown layout"), ((p, 4, 4, -1, 0, 0, p), "unknown layout"),
                          ((p, 4, 4, 2, 2, 0, p), "unknown matrix"), ((p, 4, 4, 2, -1, 0, p), "unknown matrix")):
            rc = getattr(lib, fn)(0, *args, 0)
            text = lib.af_last_error(None).decode()
            assert rc == -1 and text == "%s: %s" % (fn, msg), (fn, args[1:6], rc, text)      # AF_EINVAL
    for h, w, layout in ((0, 4, 2), (4, 0, 2), (16385, 4, 2), (4, 4, 5), (4, 4, -1)):
        assert lib.af_yuv_frame_bytes(h, w, layout) == 0
    assert lib.af_yuv_frame_bytes(16384, 16384, 0) == 3 * 16384 * 16384
    with pytest.raises(ValueError, match="expected 24 uint8 bytes for a 4x4 420jpeg frame, got 23"):
        aiod_amd.yuv_to_rgb(np.zeros(23, np.uint8), 4, 4, "420jpeg", "bt601", False)
    with pytest.raises(ValueError, match="expected an \\(H, W, 3\\) uint8 image"):
        aiod_amd.rgb_to_yuv(np.zeros((4, 4), np.uint8), "444", "bt601", False)
    with pytest.raises(ValueError, match="unknown layout '411'"):
        aiod_amd.rgb_to_yuv(np.zeros((4, 4, 3), np.uint8), "411", "bt601", False)
    img = R.rgb_inputs(5, 7)[0][1]
    assert np.array_equal(aiod_amd.rgb_to_yuv(img, "420mpeg2", "bt709", False), R.rgb_to_yuv(img, "420mpeg2", "bt709", False))      # and the library still works


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------
def _run(cmd, cwd, stdin=None):
    r = subprocess.run([str(c) for c in cmd], cwd=str(cwd), input=stdin, capture_output=True, timeout=600)
    assert r.returncode == 0, " ".join(str(c) for c in cmd) + "\n" + r.stderr.decode(errors="replace")[-3000:]
    return r


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(str(path)))


def _parse(data):
    from aiod_amd import Y4MReader
    r = Y4MReader(io.BytesIO(data))
    return r, list(r)


def _video_command(assets, video, video_out, out, extra=()):
    return [sys.executable, os.path.join(PKG, "deflicker.py"), "--video", video, "--video_out", video_out, "--out", out] + assets["common"] + list(extra)


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    """The clip as a stream (y4m_ref's RGB -> YCbCr), the video run (files in, files out) and the PNG run on what y4m.py --to_png makes of
    the stream: computed once, read by every test below."""
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    d = tmp_path_factory.mktemp("y4m_assets")
    paths = PB.write_weights(str(d / "weights"), PB.synthetic_weights())
    with open(d / "short.json", "w") as f:
        json.dump(dict(REFERENCE_CONFIG, **SHORT), f)
    frames = PB.synthetic_clip(N, H, W, seed=5)
    stream = R.y4m_bytes(frames, (30000, 1001), "420jpeg", "bt601", False)
    (d / "clip.y4m").write_bytes(stream)
    a = {"dir": d, "stream": stream, "clip": str(d / "clip.y4m"),
         "common": ["--config", str(d / "short.json"), "--down", str(DOWN), "--seed", str(SEED), "--model", paths[0], "--ckpt_filter", paths[1],
                    "--ckpt_local", paths[2], "--gpu", "0"]}
    _run(_video_command(a, a["clip"], str(d / "out.y4m"), str(d / "video_run")), d)
    _run([sys.executable, os.path.join(PKG, "y4m.py"), "--to_png", a["clip"], str(d / "png")], d)
    _run([sys.executable, os.path.join(PKG, "deflicker.py"), "--frames_dir", str(d / "png"), "--out", str(d / "png_run")] + a["common"], d)
    a["out"] = (d / "out.y4m").read_bytes()
    return a


def test_video_route_equals_the_png_route(assets):
    d = assets["dir"]
    names = ["%05d.png" % i for i in range(N)]
    assert sorted(os.listdir(d / "png")) == names                     # --to_png: the device conversion of every payload
    src, payloads = _parse(assets["stream"])
    for n, p in zip(names, payloads):
        assert np.array_equal(_png(d / "png" / n), R.yuv_to_rgb(p, H, W, "420jpeg", "bt601", False)), n
    # the stream out: the input's W H F I A C and range, one frame per input frame, each the conversion of the PNG route's final frame
    assert assets["out"].startswith(b"YUV4MPEG2 W197 H130 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\nFRAME\n")
    r, got = _parse(assets["out"])
    assert len(got) == N and (r.width, r.height, r.layout, r.full_range, r.fps) == (W, H, "420jpeg", False, src.fps)
    assert len(assets["out"]) == len(b"YUV4MPEG2 W197 H130 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n") + N * (6 + R.frame_bytes(H, W, "420jpeg"))
    assert sorted(os.listdir(d / "png_run" / "final" / "output")) == names
    finals = [_png(d / "png_run" / "final" / "output" / n) for n in names]
    assert finals[0].min() < finals[0].max()
    for i, (p, f) in enumerate(zip(got, finals)):
        assert np.array_equal(p, R.rgb_to_yuv(f, "420jpeg", "bt601", False)), i      # tolerance zero: both routes feed the same tensors
    assert not (d / "video_run" / "final").exists()
    rec = json.load(open(d / "video_run" / "deflicker.json"))
    assert (rec["video"], rec["video_out"], rec["fps"], rec["frames"]) == (assets["clip"], str(d / "out.y4m"), [30000, 1001], N)
    assert (rec["yuv_layout"], rec["yuv_matrix"], rec["yuv_range"]) == ("420jpeg", "bt601", "limited")
    other = json.load(open(d / "png_run" / "deflicker.json"))
    assert all(other[k] is None for k in ("video", "video_out", "fps", "yuv_layout", "yuv_matrix", "yuv_range"))
    assert rec["psnr"] == other["psnr"] and rec["windows"] == other["windows"] == [[0, N]]


def test_pipes_carry_the_same_bytes(assets, tmp_path):
    r = _run(_video_command(assets, "-", "-", str(tmp_path / "res")), tmp_path, stdin=assets["stream"])
    assert r.stdout == assets["out"]                                  # exactly header plus frames
    assert b"wrote %d frames to standard output" % N in r.stderr
    rec = json.load(open(tmp_path / "res" / "deflicker.json"))
    assert rec["video"] == "-" and rec["video_out"] == "-" and rec["frames"] == N


def test_cuts_on_video_input_and_frames_dir_with_video_out(assets, tmp_path):
    from aiod_amd import deflicker
    common = assets["common"]
    assert deflicker.main(["--frames_dir", str(assets["dir"] / "png"), "--video_out", str(tmp_path / "fd.y4m"), "--fps", "30000:1001", "--out", str(tmp_path / "fd")] + common) == 0
    r, got = _parse((tmp_path / "fd.y4m").read_bytes())
    assert (r.layout, r.full_range, r.aspect, r.fps.numerator) == ("420jpeg", False, None, 30000)
    assert all(np.array_equal(a, b) for a, b in zip(got, _parse(assets["out"])[1])) and len(got) == N      # the same tensors again: the video run's payloads
    rec = json.load(open(tmp_path / "fd" / "deflicker.json"))
    assert (rec["video"], rec["yuv_layout"], rec["yuv_matrix"], rec["yuv_range"]) == (None, "420jpeg", "bt601", "limited")
    assert deflicker.main(["--video", assets["clip"], "--video_out", str(tmp_path / "cut.y4m"), "--cuts", "3", "--out", str(tmp_path / "cut"), "--keep_intermediates"] + common) == 0
    rec = json.load(open(tmp_path / "cut" / "deflicker.json"))
    assert rec["shots"] == [[0, 3], [3, N]] and rec["cut_pairs"] == [2] and rec["frames"] == N and rec["windows"] == [[0, 3], [3, N]]
    assert len(_parse((tmp_path / "cut.y4m").read_bytes())[1]) == N
    flows = sorted(os.listdir(tmp_path / "cut" / "flow"))            # frames named as --to_png names them; no pair across the cut
    assert flows == sorted("%05d.png_%05d.png.npy" % p for a in (0, 1, 3) for p in ((a, a + 1), (a + 1, a)))
    assert sorted(os.listdir(tmp_path / "cut" / "stage_1" / "output")) == ["%05d.png" % i for i in range(N)] and not (tmp_path / "cut" / "final").exists()


def test_truncated_stream_ends_the_run_and_the_process_runs_again(assets, tmp_path):
    from aiod_amd import deflicker
    (tmp_path / "cut.y4m").write_bytes(assets["stream"][:-1000])
    nbytes = R.frame_bytes(H, W, "420jpeg")
    with pytest.raises(SystemExit, match="cut.y4m: truncated frame 4: %d of %d bytes" % (nbytes - 1000, nbytes)):
        deflicker.main(["--video", str(tmp_path / "cut.y4m"), "--video_out", str(tmp_path / "o.y4m"), "--out", str(tmp_path / "a")] + assets["common"])
    assert deflicker.main(["--video", assets["clip"], "--video_out", str(tmp_path / "again.y4m"), "--out", str(tmp_path / "b")] + assets["common"]) == 0
    assert (tmp_path / "again.y4m").read_bytes() == assets["out"]
