"""The deep-video route on the GPU: k_yuv_to_rgb16 / k_rgb_to_yuv16 / k_depth_reduce (csrc/yuv16.hip), k_guided_apply16
(csrc/guided.hip) through af_yuv_to_rgb16, af_rgb_to_yuv16, af_depth_reduce and af_guided_apply16, and Deflicker.run(bits=...).

Every comparison is equality.  The conversions and the reduction compute in integers, so they must equal the whole-array numpy
restatement (tests/y4m16_ref.py, held against tests/y4m_ref.py at 8 bits and against an fp64 exact twin in tests/test_deep_video_host.py)
bit for bit.  The deep apply performs single correctly rounded fp32 operations in one documented order with contraction off, and
tests/depth_transfer_ref.py performs the same operations in the same order.  The deep pipeline route runs the code a plain run of the
reduced frames runs (same kernels, same values, same seed) and carries the result to the deep frames with the kernels
aiod_amd.depth_transfer runs, so its frames must be the same samples.

Shapes: 1x1, 2x2, 3x2, 5x3 and 7x5 (clipped 2x2 blocks, replicated chroma edges), 130x9 (columns past a workgroup's first 64 blocks) and
130x66, which crosses the 128x8 footprint of a workgroup on both axes; for the apply ratio 1, a non-integer ratio, a 1x1 plane, widths that
are and are not multiples of 4 (8 and 7 over 3x2 and 1x1 planes among them), more than one workgroup across, and a frame 2 bytes off the
8-byte alignment of the vector path; for the reduction every value and 2047, 2048 and 2049 samples."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import y4m_ref as R8  # noqa: E402
import y4m16_ref as R  # noqa: E402
import guided_transfer_ref as G  # noqa: E402
import depth_transfer_ref as DT  # noqa: E402
import pipeline_bench as PB  # noqa: E402

SIZES = ((1, 1), (2, 2), (3, 2), (5, 3), (7, 5), (130, 9), (130, 66))      # (w, h)
BITS = (8, 9, 10, 12, 16)
DEV = torch.device("cuda", 0)


def dev16(a):
    """A uint16 array on the device: the type is storage only, the bytes travel as int16."""
    return torch.from_numpy(np.array(a).view(np.int16)).to(DEV).view(torch.uint16)      # np.array: a writable copy of a read-only reference


def host16(t):
    assert t.is_cuda and t.dtype == torch.uint16
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


# ---- the conversions -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_conversions_equal_the_restatement(layout):
    import aiod_amd
    for w, h in SIZES:
        for bits in BITS:
            for matrix in R.MATRICES:
                for full in (False, True):
                    for name, payload in R.inputs(h, w, layout, bits, above=bits == 10):
                        want = R.yuv_to_rgb(payload, h, w, layout, matrix, full, bits)
                        host = aiod_amd.yuv_to_rgb16(payload, h, w, layout, matrix, full, bits)
                        dev = aiod_amd.yuv_to_rgb16_device(dev16(payload), h, w, layout, matrix, full, bits)
                        assert host.shape == (h, w, 3) and host.dtype == np.uint16 and dev.dtype == torch.uint16
                        assert np.array_equal(host, want), ("read", w, h, bits, matrix, full, name, int(np.abs(host.astype(int) - want).max()))
                        assert np.array_equal(host16(dev), want), ("read, device", w, h, bits, matrix, full, name)
                    for name, img in R.rgb_inputs(h, w, bits, above=bits == 10):
                        want = R.rgb_to_yuv(img, layout, matrix, full, bits)
                        host = aiod_amd.rgb16_to_yuv(img, layout, matrix, full, bits)
                        dev = aiod_amd.rgb16_to_yuv_device(dev16(img), layout, matrix, full, bits)
                        assert host.shape == (R.frame_samples(h, w, layout),) and host.dtype == np.uint16 and dev.dtype == torch.uint16
                        assert np.array_equal(host, want), ("write", w, h, bits, matrix, full, name, int(np.abs(host.astype(int) - want).max()))
                        assert np.array_equal(host16(dev), want), ("write, device", w, h, bits, matrix, full, name)


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_at_8_bits_the_conversions_are_the_8_bit_kernels(layout):
    import aiod_amd
    for w, h in SIZES:
        for matrix in R.MATRICES:
            for full in (False, True):
                for name, payload in R8.inputs(h, w, layout):
                    got = aiod_amd.yuv_to_rgb16(payload.astype(np.uint16), h, w, layout, matrix, full, 8)
                    assert np.array_equal(got, aiod_amd.yuv_to_rgb(payload, h, w, layout, matrix, full)), ("read", w, h, matrix, full, name)
                for name, img in R8.rgb_inputs(h, w):
                    got = aiod_amd.rgb16_to_yuv(img.astype(np.uint16), layout, matrix, full, 8)
                    assert np.array_equal(got, aiod_amd.rgb_to_yuv(img, layout, matrix, full)), ("write", w, h, matrix, full, name)


def test_an_odd_pointer_is_refused_and_nothing_is_written():
    import aiod_amd
    lib = aiod_amd.load_library()
    src = torch.full((4096,), 77, dtype=torch.uint8, device=DEV)
    dst = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    for fn in ("af_yuv_to_rgb16", "af_rgb_to_yuv16"):
        for s, d in ((1, 0), (0, 1)):
            rc = getattr(lib, fn)(0, C.c_void_p(src.data_ptr() + s), 4, 4, 2, 0, 0, 10, C.c_void_p(dst.data_ptr() + d), 1)
            assert rc == -1 and lib.af_last_error(None).decode() == fn + ": uint16 pointers must be 2-byte aligned"      # AF_EINVAL
    assert lib.af_depth_reduce(0, C.c_void_p(src.data_ptr() + 1), 16, 10, C.c_void_p(dst.data_ptr()), 1) == -1
    assert lib.af_last_error(None).decode() == "af_depth_reduce: uint16 pointers must be 2-byte aligned"
    f32 = torch.zeros(64, device=DEV)
    assert lib.af_guided_apply16(0, C.c_void_p(src.data_ptr() + 1), 2, 3, 10, C.c_void_p(f32.data_ptr()), C.c_void_p(f32.data_ptr() + 128), 1, 1, C.c_void_p(dst.data_ptr()), 1) == -1
    assert lib.af_last_error(None).decode() == "af_guided_apply16: uint16 pointers must be 2-byte aligned"
    assert lib.af_guided_apply16(0, C.c_void_p(src.data_ptr()), 2, 3, 17, C.c_void_p(f32.data_ptr()), C.c_void_p(f32.data_ptr() + 128), 1, 1, C.c_void_p(dst.data_ptr()), 1) == -1
    assert lib.af_last_error(None).decode() == "af_guided_apply16: bits must be 8..16"
    assert not dst.any().item() and (src == 77).all().item()
    img = R.rgb_inputs(3, 5, 10)[2][1]
    assert np.array_equal(aiod_amd.rgb16_to_yuv(img, "420mpeg2", "bt709", False, 10), R.rgb_to_yuv(img, "420mpeg2", "bt709", False, 10))      # and the library still works


# ---- the depth reduction ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [10, 16])
def test_reduce_depth_of_every_value(bits):
    import aiod_amd
    m = R.maxv(bits)
    v = np.concatenate([np.arange(m + 1), np.arange(m + 1)[:3]]).astype(np.uint16)      # every value; a count that is no multiple of a thread's 8
    assert v.size % 8 == 3
    want = R.reduce_depth(v, bits)
    assert np.array_equal(aiod_amd.reduce_depth(v, bits), want)                                                  # host pointers
    t = dev16(v)
    got = aiod_amd.reduce_depth_device(t, bits)
    assert got.dtype == torch.uint8 and got.shape == t.shape and np.array_equal(got.cpu().numpy(), want)         # device pointers: the vector path and its tail
    off = dev16(np.concatenate([[0], v]).astype(np.uint16))[1:]                                                   # 2 bytes off: element by element
    assert off.data_ptr() % 16 == 2
    assert np.array_equal(aiod_amd.reduce_depth_device(off, bits).cpu().numpy(), want)
    if bits == 10:                                                                                                # above M reads as M
        above = np.arange(65536, dtype=np.uint16)
        assert np.array_equal(aiod_amd.reduce_depth_device(dev16(above), bits).cpu().numpy(), R.reduce_depth(above, bits))
    for count in (2047, 2048, 2049):                                                                              # around the 2048 samples of a workgroup
        part = np.resize(v, count)                                                                                # v, cut or repeated to the count
        assert np.array_equal(aiod_amd.reduce_depth(part, bits), R.reduce_depth(part, bits))
        assert np.array_equal(aiod_amd.reduce_depth_device(dev16(part), bits).cpu().numpy(), R.reduce_depth(part, bits))
    img = v[:3 * 5 * 7].reshape(5, 7, 3)
    assert aiod_amd.reduce_depth(img, bits).shape == (5, 7, 3)
    assert np.array_equal(aiod_amd.reduce_depth(np.arange(256, dtype=np.uint16), 8), np.arange(256, dtype=np.uint8))      # the identity at 8 bits


# ---- the deep apply --------------------------------------------------------------------------------------------------------------
APPLY = {"same": (5, 7, 5, 7), "ratio": (13, 17, 5, 7), "one": (2, 3, 1, 1), "vec": (12, 16, 6, 8), "wide": (9, 516, 3, 129),
         "w8": (5, 8, 3, 2), "w8_one": (5, 8, 1, 1), "w7": (5, 7, 3, 2), "w7_one": (5, 7, 1, 1)}      # H, W, h, w


def _apply_case(name, bits, kind):
    H, W, h, w = APPLY[name]
    rng = np.random.default_rng(sum(map(ord, name)) + bits)
    full = rng.integers(0, DT.maxv(bits) + 1, (H, W, 3)).astype(np.uint16)
    if kind == "random":
        a = rng.uniform(-0.5, 0.5, (h, w, 3)).astype(np.float32)
        b = rng.uniform(-40, 40, (h, w, 3)).astype(np.float32)
    else:                                                     # fields that clip at 0 and at M, and a NaN, which becomes 0
        a = np.zeros((h, w, 3), np.float32)
        b = np.where(rng.integers(0, 2, (h, w, 3)) == 1, 300, -300).astype(np.float32)
        b[0, 0, 1] = np.nan
    return full, a, b


@pytest.fixture(scope="module")
def apply_reference():
    """The restatement of every apply case, computed once and never written to."""
    out = {}
    for name in APPLY:
        for bits in (10, 16):
            for kind in ("random", "clip"):
                full, a, b = _apply_case(name, bits, kind)
                o = DT.apply16(full, bits, a, b)
                for arr in (full, a, b, o):
                    arr.setflags(write=False)
                out[name, bits, kind] = (full, a, b, o)
    return out


@pytest.mark.parametrize("name", list(APPLY))
def test_apply16_equals_the_restatement(apply_reference, name):
    import aiod_amd
    for bits in (10, 16):
        for kind in ("random",) if name.endswith("_one") else ("random", "clip"):      # the added 1x1 planes clip one way per channel: random fields only
            full, a, b, want = apply_reference[name, bits, kind]
            host = aiod_amd.guided_apply16(full, bits, a, b)
            assert host.dtype == np.uint16 and np.array_equal(host, want), (name, bits, kind, int((host != want).sum()))
            dev = aiod_amd.guided_apply16_device(dev16(full), bits, torch.from_numpy(np.array(a)).to(DEV), torch.from_numpy(np.array(b)).to(DEV))
            assert dev.dtype == torch.uint16 and np.array_equal(host16(dev), want), (name, bits, kind, "device")
            if kind == "clip":
                assert want.min() == 0 and (want.max() == DT.maxv(bits) or name == "one") and want[0, 0, 1] == 0


def test_apply16_off_the_vector_alignment(apply_reference):
    """W a multiple of 4 but the frame 2 bytes off an 8-byte boundary: the same samples sample by sample."""
    import aiod_amd
    for name in ("vec", "wide", "w8", "w8_one"):
        full, a, b, want = apply_reference[name, 10, "random"]
        assert full.shape[1] % 4 == 0
        tf = dev16(np.concatenate([[0], full.reshape(-1)]).astype(np.uint16))[1:].view(full.shape)
        assert tf.data_ptr() % 8 == 2 and tf.is_contiguous()
        out = aiod_amd.guided_apply16_device(tf, 10, torch.from_numpy(np.array(a)).to(DEV), torch.from_numpy(np.array(b)).to(DEV))
        assert np.array_equal(host16(out), want), name


def test_apply16_identities_and_the_8_bit_kernel():
    import aiod_amd
    rng = np.random.default_rng(9)
    zero = np.zeros((5, 7, 3), np.float32)
    for bits in (9, 10, 12, 14, 16):                          # abar = bbar = 0 returns F
        full = rng.integers(0, DT.maxv(bits) + 1, (13, 17, 3)).astype(np.uint16)
        assert np.array_equal(aiod_amd.guided_apply16(full, bits, zero, zero), full)
    full = rng.integers(37 * 257, 65536 - 60 * 257, (13, 16, 3)).astype(np.uint16)      # 16 bits, abar = 0, bbar = c: F + 257 c where nothing clips
    for c in (-37, 1, 60):
        out = aiod_amd.guided_apply16(full, 16, zero, np.full((5, 7, 3), c, np.float32))
        assert np.array_equal(out.astype(np.int64), full.astype(np.int64) + 257 * c)
    for name in ("ratio", "same", "one", "wide", "r32"):      # 8 bits on widened bytes: af_guided_apply's bytes
        f8, i, p, r = G.make_case(name)
        a, b = aiod_amd.guided_coeffs(i, p, radius=r, eps=G.EPS)
        assert np.array_equal(aiod_amd.guided_apply16(f8.astype(np.uint16), 8, a, b), aiod_amd.guided_apply(f8, a, b)), name


def test_depth_transfer_equals_the_restatement():
    import aiod_amd
    rng = np.random.default_rng(11)
    for sf, sp in (((24, 20), (24, 20)), ((20, 15), (9, 7))):
        for bits in (10, 16):
            full = rng.integers(0, DT.maxv(bits) + 1, sf + (3,)).astype(np.uint16)
            i, p = (rng.integers(0, 256, sp + (3,), dtype=np.uint8) for _ in range(2))
            want = DT.transfer16(full, bits, i, p, 2, G.EPS)
            assert np.array_equal(aiod_amd.depth_transfer(full, bits, i, p, radius=2, eps=G.EPS), want)
            dev = aiod_amd.depth_transfer_device(dev16(full), bits, torch.from_numpy(i).to(DEV), torch.from_numpy(p).to(DEV), radius=2, eps=G.EPS)
            assert np.array_equal(host16(dev), want)
            assert np.array_equal(aiod_amd.depth_transfer(full, bits, i, i, radius=2, eps=G.EPS), full)      # P == I returns F


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------
H, W, DOWN, SEED, N, DEPTH = 130, 197, 4, 11, 3, 10
SHORT = {"samples_batch": 1024, "iters_num": 31, "evaluate_every": 30, "pretrain_iter_number": 3, "stop_global_rigidity": 15}


@pytest.fixture(scope="module")
def clip():
    """The deep clip, 4 * frame + seeded noise in 0..3 at 10 bits, its reduction, and the runner: made once."""
    import aiod_amd
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    weights = PB.synthetic_weights()
    cfg = dict(REFERENCE_CONFIG, **SHORT)
    frames = PB.synthetic_clip(N, H, W, seed=5)
    rng = np.random.default_rng(17)
    deep = [(4 * f.astype(np.uint16) + rng.integers(0, 4, f.shape).astype(np.uint16)).astype(np.uint16) for f in frames]
    red = [aiod_amd.reduce_depth(f, DEPTH) for f in deep]
    assert all(np.array_equal(r, R.reduce_depth(f, DEPTH)) for r, f in zip(red, deep))

    def run(clip_, run_kw=None, **kw):
        return aiod_amd.Deflicker(*weights, config=cfg, down=DOWN, seed=SEED, **kw).run(clip_, **(run_kw or {}))
    return {"deep": deep, "red": red, "run": run}


def test_deep_route_is_the_plain_run_of_the_reduced_frames_carried_to_the_deep_frames(clip):
    import aiod_amd
    deep, red, run = clip["deep"], clip["red"], clip["run"]
    res = run(deep, run_kw={"bits": DEPTH})
    assert res["final"].shape == (N, H, W, 3) and res["final"].dtype == np.uint16
    assert res["depth"] == {"bits": DEPTH, "radius": aiod_amd.DEFAULT_RADIUS, "eps": aiod_amd.DEFAULT_EPS} and "proxy" not in res
    assert {"depth", "transfer"} <= set(res["seconds"]) and res["flow_size"] == [H, W]
    plain = run(red)
    assert plain["final"].dtype == np.uint8 and "depth" not in plain and "transfer" not in plain["seconds"]
    for i in range(N):
        expect = aiod_amd.depth_transfer(deep[i], DEPTH, red[i], plain["final"][i], radius=aiod_amd.DEFAULT_RADIUS, eps=aiod_amd.DEFAULT_EPS)
        assert np.array_equal(res["final"][i], expect), (i, int((res["final"][i] != expect).sum()))
    assert any(not np.array_equal(res["final"][i], deep[i]) for i in range(N))      # the run did change the frames
    assert res["final"].max() <= 1023
    # one (N, H, W, 3) uint16 CUDA tensor in: the same samples, as a tensor
    t = run(dev16(np.stack(deep)), run_kw={"bits": DEPTH})
    assert t["final"].is_cuda and t["final"].dtype == torch.uint16 and np.array_equal(host16(t["final"]), res["final"])


def test_deep_route_with_a_proxy_is_the_plain_run_of_the_shrunk_reduced_frames(clip):
    import aiod_amd
    from aiod_amd.preprocess_optical_flow import shrink_size
    deep, red, run = clip["deep"], clip["red"], clip["run"]
    edge, radius = 195, 5
    h, w = shrink_size(H, W, edge)
    res = run(deep, run_kw={"bits": DEPTH, "fidelity": True}, proxy_long_edge=edge, proxy_radius=radius)
    assert res["final"].shape == (N, H, W, 3) and res["final"].dtype == np.uint16
    assert res["depth"] == {"bits": DEPTH, "radius": radius, "eps": aiod_amd.DEFAULT_EPS}
    assert res["proxy"] == {"size": [h, w], "radius": radius, "eps": aiod_amd.DEFAULT_EPS} and res["flow_size"] == [h, w]
    assert {"depth", "proxy", "transfer", "fidelity"} <= set(res["seconds"])
    small = [aiod_amd.resize_area(f, h, w) for f in red]
    plain = run(small)
    for i in range(N):
        expect = aiod_amd.depth_transfer(deep[i], DEPTH, small[i], plain["final"][i], radius=radius, eps=aiod_amd.DEFAULT_EPS)
        assert np.array_equal(res["final"][i], expect), (i, int((res["final"][i] != expect).sum()))
    assert any(not np.array_equal(res["final"][i], deep[i]) for i in range(N))
    # the fidelity report: the 8-bit reduction of the deep finals against the 8-bit full-size input
    fid = res["fidelity"]
    assert fid["bits"] == 8 and fid["size"] == [H, W]
    ref = [aiod_amd.frame_fidelity(aiod_amd.reduce_depth(res["final"][i], DEPTH), red[i]) for i in range(N)]
    want = aiod_amd.summarise(np.concatenate([r["sse"] for r in ref]), np.concatenate([r["ssim"] for r in ref]), H, W)
    assert fid["final_vs_input"] == want


def test_video_depth_keep_writes_the_deep_run_as_a_stream(clip, tmp_path):
    """deflicker.py --video deep.y4m --video_depth keep --video_out out.y4m: the stream's frames are af_rgb_to_yuv16 of what
    run(bits=10) returns for af_yuv_to_rgb16 of the input's payloads, with the input's header."""
    import io
    import json
    import aiod_amd
    from aiod_amd import deflicker
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    paths = PB.write_weights(str(tmp_path / "weights"), PB.synthetic_weights())
    with open(tmp_path / "short.json", "w") as f:
        json.dump(dict(REFERENCE_CONFIG, **SHORT), f)
    stream = R.y4m_bytes(clip["deep"], (30000, 1001), "420jpeg", "bt601", False, DEPTH)
    (tmp_path / "deep.y4m").write_bytes(stream)
    common = ["--config", str(tmp_path / "short.json"), "--down", str(DOWN), "--seed", str(SEED), "--model", paths[0], "--ckpt_filter", paths[1],
              "--ckpt_local", paths[2], "--gpu", "0"]
    assert deflicker.main(["--video", str(tmp_path / "deep.y4m"), "--video_depth", "keep", "--video_out", str(tmp_path / "out.y4m"), "--out", str(tmp_path / "res")] + common) == 0
    raw = (tmp_path / "out.y4m").read_bytes()
    head = b"YUV4MPEG2 W197 H130 F30000:1001 Ip A1:1 C420p10 XYSCSS=420P10 XCOLORRANGE=LIMITED\n"
    assert raw.startswith(head + b"FRAME\n") and len(raw) == len(head) + N * (6 + 2 * R.frame_samples(H, W, "420jpeg"))
    src = aiod_amd.Y4MReader(io.BytesIO(stream), deep=True)
    frames_in = [R.yuv_to_rgb(p, H, W, "420jpeg", "bt601", False, DEPTH) for p in src]
    res = clip["run"](frames_in, run_kw={"bits": DEPTH})
    got = list(aiod_amd.Y4MReader(io.BytesIO(raw), deep=True))
    assert len(got) == N
    for i in range(N):
        assert np.array_equal(got[i], R.rgb_to_yuv(res["final"][i], "420jpeg", "bt601", False, DEPTH)), i
    rec = json.load(open(tmp_path / "res" / "deflicker.json"))
    assert rec["depth"]["bits"] == DEPTH and rec["frames"] == N and rec["yuv_layout"] == "420jpeg" and not (tmp_path / "res" / "final").exists()
    with pytest.raises(SystemExit, match="needs --video_out"):
        deflicker.main(["--video", str(tmp_path / "deep.y4m"), "--video_depth", "keep", "--out", str(tmp_path / "r2")] + common)
